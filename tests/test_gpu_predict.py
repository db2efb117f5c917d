"""GPU tests of the fused prediction path: ``ssal_predict_logits_nhwc`` / ``ssal_label_lut`` and
``inference.predict`` against the composed device path (``resize_bilinear`` -> ``score_logits`` -> torch gather), which
they must equal byte for byte, against the numpy restatement on exact ties, and against the CPU oracle."""
import numpy as np
import pytest
import torch
from PIL import Image

import predict_oracle as po
import semanticsegmentationactivelearning_amd as ssal
from helpers import frames
from semanticsegmentationactivelearning_amd import _lib, active_learning as al, inference as inf, synthetic as syn

pytestmark = pytest.mark.gpu

EMB = np.zeros(256, np.uint8)
EMB[:19] = [7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    _lib.lib()
    yield
    torch.cuda.synchronize()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def fused(logits, size, lut=None):
    """ssal_predict_logits_nhwc on a device tensor [N,H,W,K] (contiguous; any 4-byte aligned start)"""
    n, h, w, k = logits.shape
    ch = 0 if lut is None else 1 if lut.dim() == 1 else 3
    out = torch.empty((n,) + tuple(size) + ((3,) if ch == 3 else ()), dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().ssal_predict_logits_nhwc(_lib.dev_ptr(logits), n, h, w, k, size[0], size[1], _lib.dev_ptr(lut), ch,
                                                   _lib.dev_ptr(out), _lib.stream_ptr()))
    return out


def composed(logits, size):
    _, extra = al.score_logits(inf.resize_bilinear(logits, size), "confidence", return_label=True)
    return extra["label"]


@pytest.fixture(scope="module")
def tables():
    return dev(po.id_table()), dev(po.colour_table())


@pytest.mark.parametrize("k", range(2, 33))
def test_equals_the_composed_device_path_exactly(k, tables):
    ids, rgb = tables
    x = dev(po.logits(k))
    for size in po.SIZES:
        label = composed(x, size).long()
        assert torch.equal(fused(x, size), label.to(torch.uint8)), (k, size)
        assert torch.equal(fused(x, size, ids), ids[label]), (k, size)
        assert torch.equal(fused(x, size, rgb), rgb[label]), (k, size)


@pytest.mark.parametrize("k", [3, 4, 19])
def test_ties_go_to_the_lowest_class(k):
    """small integer logits at ratios 1 and 2: every lerp weight is 0 or 0.5, every resized value exact"""
    rng = np.random.default_rng(k)
    h, w = 6, 9
    flat = np.zeros((1, h, w, k), np.float32)
    two = rng.integers(-3, 3, (2, h, w, k)).astype(np.float32)
    a, b = 0, k - 1
    two[0, ..., a] = 4.0
    two[0, ..., b] = 4.0
    for size in ((h, w), (2 * h, 2 * w)):
        assert not fused(dev(flat), size).any()
        got = fused(dev(two), size).cpu().numpy()
        assert (got[0] == a).all()
        assert np.array_equal(got, po.predict(two, size))


@pytest.mark.parametrize("k", [4, 19])
def test_input_view_one_float_into_its_allocation(k, tables):
    ids, rgb = tables
    x = po.logits(k)
    buf = torch.zeros(x.size + 1, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[1:].view(x.shape)
    view.copy_(dev(x))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    for size in po.SIZES:
        label = composed(dev(x), size).long()
        assert torch.equal(fused(view, size), label.to(torch.uint8)), size
        assert torch.equal(fused(view, size, ids), ids[label]), size
        assert torch.equal(fused(view, size, rgb), rgb[label]), size


@pytest.mark.parametrize("k", po.ORACLE_K)
def test_against_the_cpu_oracle(k):
    x = po.logits(k)
    for size in po.SIZES:
        want, sure = po.sure_pixels(x, size)
        got = fused(dev(x), size).cpu().numpy()
        assert sure.mean() > po.SURE_SHARE and (got[sure] == want[sure]).all(), (k, size)


@pytest.mark.parametrize("pixels", [1, 3, 4, 1027, 3 * 256 * 4 + 2])
def test_label_lut_alone(pixels, tables):
    ids, rgb = tables
    L = _lib.lib()
    buf = dev(np.random.default_rng(pixels).integers(0, 32, pixels + 1).astype(np.uint8))
    for label in (buf[:pixels], buf[1:]):  # 4-byte aligned (four pixels per thread) and not (bytes)
        for lut, ch in ((None, 0), (ids, 1), (rgb, 3)):
            out = torch.empty((pixels, 3) if ch == 3 else (pixels,), dtype=torch.uint8, device="cuda")
            _lib.check(L.ssal_label_lut(_lib.dev_ptr(label), pixels, _lib.dev_ptr(lut), ch, _lib.dev_ptr(out), _lib.stream_ptr()))
            assert torch.equal(out, label if lut is None else lut[label.long()]), (pixels, ch)


@pytest.fixture(scope="module")
def icnet19():
    net = ssal.ICNet(19)
    net.build((None, None, None, 3))
    syn.randomize_icnet(net, seed=0)
    return net


def _end_to_end(net):
    x = dev(frames([30, 31], 64, 64, 3))
    assert torch.equal(inf.predict(net, x), inf.predict_labels(net, x))
    assert torch.equal(inf.predict(net, x, size=(96, 80), embedding_reversed=EMB),
                       inf.reverse_embedding(inf.predict_labels(net, x, (96, 80)), EMB))
    cmap = po.colour_table()[:19]
    assert torch.equal(inf.predict(net, x, colormap=cmap), inf.colorize(inf.predict_labels(net, x), cmap))
    assert torch.equal(inf.predict(net, x, embedding_reversed=EMB), inf.reverse_embedding(inf.predict_labels(net, x), EMB))


def test_predict_equals_predict_labels_enet(enet_c3k19):
    _end_to_end(enet_c3k19[0])


def test_predict_equals_predict_labels_icnet(icnet19):
    _end_to_end(icnet19)


def test_run_inference_fused_writes_the_same_pngs(enet_c3k19, tmp_path):
    net = enet_c3k19[0]
    x = frames([30, 31, 32], 64, 64, 3)
    batches = [(x[:2], [b"a", "b"]), (x[2:], ["c"])]  # a second, smaller batch reuses the page-locked buffer
    cmap = np.zeros((256, 3), np.uint8)
    cmap[:19] = po.colour_table()[:19]
    for name, kw in (("ids", {"embedding_reversed": EMB}), ("rgb", {"colormap": cmap}), ("up", {"colormap": cmap, "size": (96, 80)})):
        a = inf.run_inference(net, batches, str(tmp_path / (name + "_composed")), fused=False, **kw)
        b = inf.run_inference(net, batches, str(tmp_path / (name + "_fused")), fused=True, **kw)
        assert [p.split("/")[-1] for p in a] == [p.split("/")[-1] for p in b] == ["a.png", "b.png", "c.png"]
        for pa, pb in zip(a, b):
            ia, ib = np.asarray(Image.open(pa)), np.asarray(Image.open(pb))
            assert ia.shape == ib.shape and ia.shape[:2] == kw.get("size", (64, 64)) and np.array_equal(ia, ib), (name, pa)
