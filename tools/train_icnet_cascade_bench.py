"""Cost of one training step of ICNet's whole cascade head on one MI355X: ICNet(19), batch 8 x 1024 x 2048 float32 frames,
HIP-event timing, everything in ONE process on ONE box.

Rows (ms per batch; median and min / max over --repeats timed windows of --steps batches each, the rows timed in
--repeats interleaved rounds so that drift of the box hits every row alike):
  fusion_step      ICNetFusionTrainer.step(images) -- the yardstick: what training the last fusion stage costs in the same run
  step             ICNetCascadeTrainer.step(images): the frozen branches up to conv5_4_k1 / conv3_1 / conv3_sub1, both fusion
                   blocks and the head on the weights being trained, the gradient kernels, Adam, the copy back to the host and
                   into the handle
  step_features    ICNetCascadeTrainer.step_features on cached features (no trunk)
  grad_features    the gradient alone on cached features (no Adam, no host copy)
  copy             a device-to-device copy of 256 MB (the box's copy rate, read + write, the byte floors are held against)
The per-launch milliseconds come from the library's launch profiler in a separate pass.  k_icnet_cascade_dx and the
256-channel weight-gradient launch are held against their byte floors (every operand read once, every result written once)
and, with --mfma-tflops (the fp32 MFMA rate tools/mfma_peak.py measures on the same box), against their matrix-core floors;
without it those entries say "not yet measured".  Writes the record to --out.

    python tools/train_icnet_cascade_bench.py [--repeats 5] [--steps 10] [--mfma-tflops T] [--out profiles/r21_train_icnet_cascade_bench.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from semanticsegmentationactivelearning_amd import _lib, models, synthetic  # noqa: E402
from semanticsegmentationactivelearning_amd.training import ICNetCascadeTrainer, ICNetFusionTrainer  # noqa: E402

N, H, W, K = 8, 1024, 2048, 19
PIX8, PIX16, PIX32 = (N * (H // d) * (W // d) for d in (8, 16, 32))
# what each launch must move once, and its matrix-core work
FLOORS = {
    "k_icnet_cascade_dx": {"bytes": {"g": PIX8 * 128 * 4, "conv_sub2.kernel": 9 * 128 * 128 * 4, "du": PIX8 * 128 * 4},
                           "flop": 2.0 * PIX8 * 9 * 128 * 128},
    "k_icnet_fusion_wgrad<256>": {"bytes": {"g24": PIX16 * 128 * 4, "conv5_4_k1": PIX32 * 256 * 4, "conv3_1": PIX16 * 256 * 4,
                                            "partials": 64 * 360448 * 4},
                                  "flop": 2.0 * PIX16 * (9 * 256 + 256) * 128},
}
NOT_MEASURED = "not yet measured"


def window(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--mfma-tflops", type=float, default=None)
    ap.add_argument("--out", default="profiles/r21_train_icnet_cascade_bench.json")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    net = models.ICNet(K)
    net.build((None, None, None, 3))
    synthetic.randomize_icnet(net, seed=0)
    x = synthetic.synth_frames_device(0, N, H, W, 3)
    scores, extra = net.score(x, return_label=True)
    labels = extra["label"].clone()
    mask = torch.ones((N, H, W), dtype=torch.float32, device=x.device)
    fusion = ICNetFusionTrainer(net, 5e-4, 0.9, 0.99, l2=2e-4, loginverse_scaling=1.02)
    tr = ICNetCascadeTrainer(net, 5e-4, 0.9, 0.99, l2=2e-4, loginverse_scaling=1.02)
    feats = tr.features(x)
    tr.reinitialize(seed=0)
    src = torch.empty(256 << 20, dtype=torch.uint8, device=x.device)
    dst = torch.empty_like(src)
    rows = {
        "fusion_step": lambda: fusion.step(x, labels, mask),
        "step": lambda: tr.step(x, labels, mask),
        "step_features": lambda: tr.step_features(*feats, labels, mask),
        "grad_features": lambda: tr.gradient_features(*feats, labels, mask),
        "copy": lambda: dst.copy_(src),
    }
    for fn in rows.values():  # warm-up: workspaces, handle pushes, code objects
        fn()
        fn()
    torch.cuda.synchronize()
    runs = {k: [] for k in rows}
    for _ in range(args.repeats):
        for name, fn in rows.items():
            runs[name].append(window(fn, args.steps))
    out = {"batch": [N, H, W, K], "steps_per_window": args.steps, "rows_ms_per_batch": {}}
    for name, v in runs.items():
        out["rows_ms_per_batch"][name] = {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)),
                                          "repeats": v}
        print("%-14s median %8.3f ms  [%8.3f, %8.3f]" % (name, np.median(v), min(v), max(v)), flush=True)
    out["step_over_fusion_step"] = float(np.median(runs["step"]) / np.median(runs["fusion_step"]))
    copy_rate = 2.0 * src.numel() / (np.median(runs["copy"]) * 1e-3)  # bytes read + written per second
    out["copy_rate_GBps"] = copy_rate / 1e9
    _lib.profile_enable(True)
    for _ in range(3):
        tr.step(x, labels, mask)
    torch.cuda.synchronize()
    prof = _lib.profile_collect()
    _lib.profile_enable(False)
    out["kernels_3_steps"] = prof
    for kname, r in sorted(prof.items()):
        print("%-26s %.3f ms / launch, %.3g GFLOP, %.3g MB" % (kname, r["ms"] / r["launches"],
                                                                    r["flops"] / r["launches"] / 1e9,
                                                                    r["bytes"] / r["launches"] / 1e6), flush=True)
    out["floors"] = {}
    for kname, fl in FLOORS.items():
        floor_ms = sum(fl["bytes"].values()) / copy_rate * 1e3
        rec = {"bytes": fl["bytes"], "ms_at_copy_rate": floor_ms, "flop": fl["flop"], "kernel_ms": NOT_MEASURED,
               "times_the_byte_floor": NOT_MEASURED, "tflops": NOT_MEASURED, "mfma_tflops": NOT_MEASURED,
               "ms_at_mfma_rate": NOT_MEASURED, "times_the_mfma_floor": NOT_MEASURED}
        if args.mfma_tflops:
            rec["mfma_tflops"] = args.mfma_tflops
            rec["ms_at_mfma_rate"] = fl["flop"] / (args.mfma_tflops * 1e12) * 1e3
        if kname in prof:
            ms = prof[kname]["ms"] / prof[kname]["launches"]
            rec.update(kernel_ms=ms, times_the_byte_floor=ms / floor_ms, tflops=fl["flop"] / (ms * 1e-3) / 1e12)
            if args.mfma_tflops:
                rec["times_the_mfma_floor"] = ms / rec["ms_at_mfma_rate"]
        out["floors"][kname] = rec
        print("%s: byte floor %.3f ms, %.1f GFLOP, kernel %s ms" % (kname, floor_ms, fl["flop"] / 1e9, rec["kernel_ms"]))
    out["knobs"] = _lib.get_knobs()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
