"""GPU tests of the PNG decode path: the batch decoder (include/ssal_enet.h ssal_png_decode_nhwc) against Pillow, and
InputStage(decode="gpu") against decode="cpu" end to end (ranking and evaluation included).  Valid streams only."""
import ctypes

import numpy as np
import pytest

from png_corpus import pillow_decode, pillow_png, photo, png_corpus
from semanticsegmentationactivelearning_amd import _lib, synthetic as syn
from semanticsegmentationactivelearning_amd.tensortools import InputStage, png, tfrecord

pytestmark = pytest.mark.gpu


def _decode_batch(datas, oh, ow, tops=None, lefts=None, channels=4):
    """one launch over every PNG in datas: frame f = datas[f], crop window oh x ow at (top, left), all channels"""
    import torch
    L = _lib.lib()
    streams = [png.parse(d) for d in datas]
    descs, off, payload = [], 0, bytearray()
    for f, s in enumerate(streams):
        top = tops[f] if tops else 0
        left = lefts[f] if lefts else 0
        descs.append([off, s.nbytes, s.width, s.height, s.channels, 0, f, 0, 0, s.channels, top, left, 0, 0, 0, 0])
        z = s.joined()
        payload += z + bytes(-len(z) % 16)
        off = len(payload)
    desc = np.asarray(descs, dtype=np.int64)
    ws_bytes = L.ssal_png_plan(len(descs), desc.ctypes.data_as(ctypes.c_void_p))
    dev = torch.device("cuda")
    pay = torch.from_numpy(np.frombuffer(bytes(payload), dtype=np.uint8).copy()).to(dev)
    d = torch.from_numpy(desc).to(dev)
    image = torch.full((len(datas), oh, ow, channels), 7, dtype=torch.uint8, device=dev)
    status = torch.full((len(datas),), -1, dtype=torch.int32, device=dev)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    vp = ctypes.c_void_p
    _lib.check(L.ssal_png_decode_nhwc(vp(pay.data_ptr()), len(payload), vp(d.data_ptr()), len(descs), len(datas), oh, ow,
                                      channels, None, vp(image.data_ptr()), 0, None, None, None, vp(status.data_ptr()),
                                      vp(ws.data_ptr()), ws_bytes, _lib.stream_ptr()))
    torch.cuda.synchronize()
    return status.cpu().numpy(), image.cpu().numpy(), streams


def test_batch_decode_matches_pillow_mixed_sizes():
    corpus = [d for _, d in png_corpus()]
    want = [pillow_decode(d) for d in corpus]
    # every frame is cropped to the smallest size; offsets vary per frame
    oh = min(w.shape[0] for w in want)
    ow = min(w.shape[1] for w in want)
    rng = np.random.default_rng(0)
    tops = [int(rng.integers(0, w.shape[0] - oh + 1)) for w in want]
    lefts = [int(rng.integers(0, w.shape[1] - ow + 1)) for w in want]
    st, got, streams = _decode_batch(corpus, oh, ow, tops, lefts)
    assert (st == 0).all(), st
    for f, w in enumerate(want):
        c = w.shape[2]
        ref = w[tops[f]:tops[f] + oh, lefts[f]:lefts[f] + ow]
        assert np.array_equal(got[f, :, :, :c], ref), f
        assert (got[f, :, :, c:] == 7).all()  # channels past the stream's own are untouched


def test_batch_decode_many_frames_in_flight():
    datas = [pillow_png(photo(24 + (i % 5), 40 + (i % 7), 3, seed=i)) for i in range(300)]
    st, got, _ = _decode_batch(datas, 24, 40, channels=3)
    assert (st == 0).all()
    for i, d in enumerate(datas):
        assert np.array_equal(got[i], pillow_decode(d)[:24, :40]), i


def test_batch_decode_full_size_frames():
    """1024 x 2048 RGB synthetic frames, encoded as tools/input_bench.py does"""
    datas = [pillow_png(syn.synth_frame_u8(i, 1024, 2048, 3)) for i in range(3)]
    st, got, _ = _decode_batch(datas, 1024, 2048, channels=3)
    assert (st == 0).all()
    for i, d in enumerate(datas):
        assert np.array_equal(got[i], pillow_decode(d)), i


# ---- InputStage(decode="gpu") against decode="cpu" --------------------------------------------------------------------
def _jpeg(arr):
    import io
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(arr).save(b, format="JPEG")
    return b.getvalue()


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    d = tmp_path_factory.mktemp("png_records")
    files = []
    h, w = 48, 64
    for i in range(8):
        img = photo(h, w, 3, seed=100 + i)
        lab = (photo(h, w, 1, seed=200 + i)[:, :, 0] % 21).astype(np.uint8)
        lab[lab == 20] = 255
        nir = photo(h, w, 1, seed=300 + i)[:, :, 0]
        feats = {"image/data": _jpeg(img) if i == 5 else pillow_png(img if i != 2 else
                                                                    np.dstack([img, img[:, :, :1]])),
                 "image/encoding": "png", "image/channels": 3,
                 "label": b"" if i == 3 else pillow_png(lab, mode="P" if i % 2 else None),
                 "nir/data": pillow_png(nir), "height": h, "width": w, "id": "f%d" % i}
        fn = str(d / ("f%d.tfrecord" % i))
        tfrecord.write_tfrecord(fn, [tfrecord.make_example(feats)])
        files.append(fn)
    return files


def _run(files, decode, augment, dtype, modalities=(), batch=3, ahead=4):
    st = InputStage([32, 48], modalities=modalities, seed=11, workers=3, image_dtype=dtype, decode=decode,
                    decode_ahead=ahead)
    aux = np.arange(len(files))
    st.add_dataset_from_placeholders("d", files, aux, batch_size=batch, augment=augment)
    st.init_iterator("d")
    out = []
    for b in st:
        out.append(tuple(x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x) for x in b))
    return out, st


@pytest.mark.parametrize("augment", [False, True])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("modalities", [(), ("nir",)])
def test_input_stage_gpu_matches_cpu(records, augment, dtype, modalities):
    want, _ = _run(records, "cpu", augment, dtype, modalities)
    got, st = _run(records, "gpu", augment, dtype, modalities)
    assert len(got) == len(want) == 3 and len(got[-1][0]) == 2  # partial last batch
    for g, w in zip(got, want):
        assert len(g) == len(w)
        for a, b in zip(g, w):
            assert a.dtype == b.dtype and a.shape == b.shape
            assert np.array_equal(a, b)
    assert st.decode_stats == {"gpu": 7, "fallback": 1}  # the JPEG record
    b = next(iter(_run(records, "gpu", augment, dtype, modalities, ahead=8)[0]))
    assert np.array_equal(b[0], want[0][0])


def test_gpu_batches_are_device_tensors(records):
    st = InputStage([32, 48], seed=0, workers=2, image_dtype=np.uint8, decode="gpu", decode_ahead=3)
    st.add_dataset_from_placeholders("d", records, np.arange(len(records)), batch_size=3, augment=False)
    st.init_iterator("d")
    image, label, mask, idx = st.get_output()
    assert image.is_cuda and label.is_cuda and mask.is_cuda and isinstance(idx, np.ndarray)


def test_rank_and_evaluate_fed_by_gpu_decode(records, enet_c3k19):
    import torch
    from semanticsegmentationactivelearning_amd import active_learning as al
    net, _ = enet_c3k19
    n = len(records)

    def feed(decode, augment):
        st = InputStage([32, 48], seed=5, workers=2, image_dtype=np.uint8, decode=decode, decode_ahead=4,
                        pin_memory=decode == "cpu")
        st.add_dataset_from_placeholders("d", records, np.arange(n), batch_size=3, augment=augment)
        st.init_iterator("d")
        return st

    res = {}
    for decode in ("cpu", "gpu"):
        st = feed(decode, True)
        batches = ((b[0], b[-1]) for b in st)
        low, conf = al.rank_confidence(net, batches, n, np.arange(n), 3, prefetch=2)
        metrics = al.evaluate(net, (b[:3] for b in feed(decode, False)), 19)
        conf_direct = torch.zeros((19, 19), dtype=torch.int64, device="cuda")
        for image, label, mask, _ in feed(decode, False):
            net.evaluate(image, label, mask, confusion=conf_direct)
        torch.cuda.synchronize()
        counts = np.stack([metrics[k] for k in ("TruePositive", "FalsePositive", "FalseNegative", "TrueNegative")])
        res[decode] = (np.asarray(low), np.asarray(conf.cpu() if hasattr(conf, "cpu") else conf), counts,
                       conf_direct.cpu().numpy())
    assert np.array_equal(res["cpu"][0], res["gpu"][0])
    assert np.array_equal(res["cpu"][1], res["gpu"][1])
    assert np.array_equal(res["cpu"][2], res["gpu"][2])
    assert np.array_equal(res["cpu"][3], res["gpu"][3]) and res["gpu"][3].sum() > 0
