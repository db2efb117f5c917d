"""PNG decode on the GPU against the Pillow path, on the reference's data format (one TFRecord per 1024x2048 RGB frame,
PNG-encoded by Pillow as tools/input_bench.py does): decode-only images/s of InputStage(decode="cpu") with 16 workers
and of InputStage(decode="gpu"), then the end-to-end ranking pass (TFRecords -> decode -> ENet score -> rank) for both,
and the GPU-idle fraction of each end-to-end run (1 - frames / score-only rate / wall time; the score-only rate is
measured on frames resident in HBM).
Usage: python tools/png_decode_bench.py [frames=256] [decode_ahead=128] [workers=16]"""
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from semanticsegmentationactivelearning_amd import synthetic as syn
from semanticsegmentationactivelearning_amd.tensortools import InputStage, tfrecord


def png(arr):
    import io
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(arr).save(b, format="PNG")
    return b.getvalue()


def write_pool(n, h, w, workers):
    from concurrent.futures import ThreadPoolExecutor
    tmp = tempfile.mkdtemp(prefix="ssal_png_pool_")
    uniq = min(n, 32)  # encode 32 distinct frames, reuse them for the rest of the pool
    with ThreadPoolExecutor(workers) as ex:
        datas = list(ex.map(lambda i: png(syn.synth_frame_u8(i, h, w, 3)), range(uniq)))
    for i in range(n):
        feats = {"image/data": datas[i % uniq], "image/encoding": "png", "image/channels": 3, "label": b"",
                 "height": h, "width": w, "id": "frame_%04d" % i}
        tfrecord.write_tfrecord(os.path.join(tmp, "frame_%04d.tfrecord" % i), [tfrecord.make_example(feats)])
    return tmp, sum(len(d) for d in datas) / uniq


def stage_for(decode, h, w, workers, ahead):
    st = InputStage(input_shape=[h, w], workers=workers, image_dtype=np.uint8, decode=decode, decode_ahead=ahead,
                    pin_memory=decode == "cpu", pin_buffers=6)
    return st


def main():
    import torch
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    ahead = int(sys.argv[2]) if len(sys.argv) > 2 else 128
    workers = int(sys.argv[3]) if len(sys.argv) > 3 else 16
    h, w = 1024, 2048
    pool, mb = write_pool(n, h, w, workers)
    print("pool: %d records %dx%d, %.2f MB PNG each" % (n, h, w, mb / 1e6), flush=True)
    import semanticsegmentationactivelearning_amd as ssal
    from semanticsegmentationactivelearning_amd import active_learning as al
    net = ssal.ENet(19)
    net.build((None, None, None, 3))
    syn.randomize_enet(net, seed=0)

    # score-only rate on resident frames (the bench.py setting)
    x = syn.synth_frames_device(0, 8, h, w, 3)
    for _ in range(3):
        net.score(x)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):
        net.score(x)
    torch.cuda.synchronize()
    score_rate = 80 / (time.perf_counter() - t0)
    print("score only (resident uint8->f32 frames, batch 8): %.1f images/s" % score_rate, flush=True)

    for decode in ("cpu", "gpu"):
        st = stage_for(decode, h, w, workers, ahead)
        st.add_dataset("pool", pool, batch_size=8)
        for rep in range(2):  # the first pass warms the page-locked ring, the allocator and the kernels
            st.init_iterator("pool")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cnt = 0
            for b in st:
                cnt += len(b[0])
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        print("decode only, %s: %7.1f images/s  (%s)" % (decode, cnt / dt, st.decode_stats if decode == "gpu" else
                                                         "%d workers" % workers), flush=True)
        for rep in range(2):
            st.init_iterator("pool")
            pos = [0]

            def batches():
                for b in st:
                    k = len(b[0])
                    yield b[0], np.arange(pos[0], pos[0] + k)
                    pos[0] += k

            torch.cuda.synchronize()
            t0 = time.perf_counter()
            al.rank_confidence(net, batches(), n, np.arange(n), min(8, n), measure="entropy", prefetch=2)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        idle = max(0.0, 1.0 - (n / score_rate) / dt)
        print("end to end, %s: TFRecords -> decode -> score -> rank: %7.1f images/s, GPU scorer idle %.0f %%"
              % (decode, n / dt, 100 * idle), flush=True)


if __name__ == "__main__":
    main()
