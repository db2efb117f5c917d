"""Cost of the test-split prediction stage on one MI355X: ENet(19), batch 8, the id table of
Cityscapes, fused route (inference.predict) against the composed one (predict_labels + reverse_embedding) in ONE process
on ONE box, HIP-event timing.

Shapes:
  a   input 512 x 1024, output size 1024 x 2048 (resize + argmax + table: ssal_predict_logits_nhwc)
  b   input 1024 x 2048, size=None (label plane of the fused score kernel + ssal_label_lut)
Rows (ms per batch; a fused row and its composed row are timed as interleaved PAIRS, --repeats pairs of --steps batches each,
so that drift of the box hits both alike; median, min / max, and the per-pair differences fused - composed):
  a_fused / a_composed, b_fused / b_composed         network included
  a_stage_fused / a_stage_composed                   the stage alone on logits that are already there
The new kernels' own time comes from the library's launch profiler in a separate pass and is set against their byte floor:
input read once plus output written once at the HBM rate bench.py's roofline leg uses.  Writes the record to --out.

    python tools/inference_bench.py [--repeats 7] [--steps 5] [--out profiles/r18_inference_bench.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from semanticsegmentationactivelearning_amd import _lib, models, synthetic  # noqa: E402
from semanticsegmentationactivelearning_amd import active_learning as al  # noqa: E402
from semanticsegmentationactivelearning_amd import inference as inf  # noqa: E402

N, K = 8, 19
SHAPE_A = dict(h=512, w=1024, size=(1024, 2048))
SHAPE_B = dict(h=1024, w=2048, size=None)
HBM_GBS = 6300.0  # bench.py MEASURED_HBM_GBS
EMB = np.zeros(256, np.uint8)
EMB[:K] = [7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33]


def window(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "repeats": [float(t) for t in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default="profiles/r18_inference_bench.json")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    net = models.ENet(K)
    net.build((None, None, None, 3))
    synthetic.randomize_enet(net, seed=0)
    xa = synthetic.synth_frames_device(0, N, SHAPE_A["h"], SHAPE_A["w"], 3)
    xb = synthetic.synth_frames_device(0, N, SHAPE_B["h"], SHAPE_B["w"], 3)
    logits_a = net(xa, training=False).clone()
    lut = torch.from_numpy(EMB).cuda()
    oh, ow = SHAPE_A["size"]
    stage_out = torch.empty((N, oh, ow), dtype=torch.uint8, device="cuda")

    def stage_fused():
        _lib.check(_lib.lib().ssal_predict_logits_nhwc(_lib.dev_ptr(logits_a), N, SHAPE_A["h"], SHAPE_A["w"], K, oh, ow,
                                                       _lib.dev_ptr(lut), 1, _lib.dev_ptr(stage_out), _lib.stream_ptr()))
        return stage_out

    def stage_composed():
        _, e = al.score_logits(inf.resize_bilinear(logits_a, (oh, ow)), "confidence", return_label=True)
        return inf.reverse_embedding(e["label"], EMB)

    pairs = {
        "a": (lambda: inf.predict(net, xa, SHAPE_A["size"], embedding_reversed=EMB),
              lambda: inf.reverse_embedding(inf.predict_labels(net, xa, SHAPE_A["size"]), EMB)),
        "b": (lambda: inf.predict(net, xb, None, embedding_reversed=EMB),
              lambda: inf.reverse_embedding(inf.predict_labels(net, xb, None), EMB)),
        "a_stage": (stage_fused, stage_composed),
    }
    out = {"batch": N, "classes": K, "model": "enet", "table": "embedding_reversed (ids)", "shapes": {"a": SHAPE_A, "b": SHAPE_B},
           "steps_per_window": args.steps, "rows_ms_per_batch": {}, "pairs": {}, "same_bytes": {}}
    for name, (fused, composed) in pairs.items():  # warm-up (workspaces, code objects) and the bytes both routes give
        same = torch.equal(fused(), composed())
        fused(), composed()
        torch.cuda.synchronize()
        out["same_bytes"][name] = bool(same)
        print("%-8s fused bytes == composed bytes: %s" % (name, same), flush=True)
    for name, (fused, composed) in pairs.items():
        tf, tc = [], []
        for _ in range(args.repeats):
            tf.append(window(fused, args.steps))
            tc.append(window(composed, args.steps))
        d = [a - b for a, b in zip(tf, tc)]
        out["rows_ms_per_batch"][name + "_fused"], out["rows_ms_per_batch"][name + "_composed"] = stats(tf), stats(tc)
        spread = max(d) - min(d)
        out["pairs"][name] = {"fused_minus_composed_ms": stats(d), "pair_spread_ms": float(spread),
                              "fused_not_slower_beyond_spread": bool(np.median(d) <= spread)}
        print("%-8s fused %8.3f ms [%8.3f, %8.3f]  composed %8.3f ms [%8.3f, %8.3f]  fused - composed median %+8.3f ms, "
              "spread %.3f ms" % (name, np.median(tf), min(tf), max(tf), np.median(tc), min(tc), max(tc), np.median(d), spread),
              flush=True)
    # the new kernels alone, against their byte floor
    floors = {"k_resize_argmax": 4.0 * N * SHAPE_A["h"] * SHAPE_A["w"] * K + N * oh * ow,
              "k_label_lut": 2.0 * N * SHAPE_B["h"] * SHAPE_B["w"]}
    out["kernels"] = {}
    for row, kname in (("a", "k_resize_argmax"), ("b", "k_label_lut")):
        _lib.profile_enable(True)
        for _ in range(5):
            pairs[row][0]()
        torch.cuda.synchronize()
        prof = _lib.profile_collect()
        _lib.profile_enable(False)
        r = prof[kname]
        ms, floor_ms = r["ms"] / r["launches"], floors[kname] / (HBM_GBS * 1e9) * 1e3
        out["kernels"][kname] = {"ms_per_launch": ms, "launches": r["launches"], "floor_bytes": floors[kname],
                                 "hbm_gbs": HBM_GBS, "floor_ms": floor_ms, "time_over_floor": ms / floor_ms,
                                 "all_kernels_of_the_route": prof}
        print("%-16s %.3f ms / launch, byte floor %.3f ms (%.0f MB at %.0f GB/s): %.2f x the floor"
              % (kname, ms, floor_ms, floors[kname] / 1e6, HBM_GBS, ms / floor_ms), flush=True)
    out["knobs"] = _lib.get_knobs()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
