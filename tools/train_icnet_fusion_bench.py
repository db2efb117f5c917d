"""Cost of one training step of ICNet's last fusion stage on one MI355X: ICNet(19), batch 8 x 1024 x 2048 float32 frames,
HIP-event timing, everything in ONE process on ONE box.

Rows (ms per batch; median and min / max over --repeats timed windows of --steps batches each, the rows timed in
--repeats interleaved rounds so that drift of the box hits every row alike):
  forward          net(x, training=False) -- trunk + the fusion block + conv6_cls + the 4x resize, logits written
  head_step        ICNetHeadTrainer.step(images) -- the yardstick: what training conv6_cls alone costs in the same run
  step             ICNetFusionTrainer.step(images): trunk up to sub24_sum / conv3_sub1, the block and the head on the weights
                   being trained, the gradient kernels, Adam, the copy of the 0.7 MB back to the host and into the handle
  step_features    ICNetFusionTrainer.step_features on cached features (no trunk)
  grad_features    the gradient alone on cached features (no Adam, no host copy)
  copy             a device-to-device copy of 256 MB (the box's copy rate, read + write, the byte floor is held against)
The per-kernel milliseconds come from the library's launch profiler in a separate pass.  k_icnet_fusion_wgrad is held
against its byte floor (sub24_sum, conv3_sub1 and g read once, the partials written once) and, with --mfma-tflops (the fp32
MFMA rate tools/mfma_peak.py measures on the same box), against its matrix-core floor.  Writes the record to --out.

    python tools/train_icnet_fusion_bench.py [--repeats 5] [--steps 10] [--mfma-tflops T] [--out profiles/r20_train_icnet_fusion_bench.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from semanticsegmentationactivelearning_amd import _lib, models, synthetic  # noqa: E402
from semanticsegmentationactivelearning_amd.training import ICNetFusionTrainer, ICNetHeadTrainer  # noqa: E402

N, H, W, K = 8, 1024, 2048, 19
PIX = N * (H // 8) * (W // 8)
# what k_icnet_fusion_wgrad must move once: g, sub24_sum, conv3_sub1 read, 96 split-K partials of 10 x 128 x 128 written
FLOOR_BYTES = {"g": PIX * 128 * 4, "sub24_sum": PIX // 4 * 128 * 4, "conv3_sub1": PIX * 64 * 4, "partials": 96 * 163840 * 4}
WGRAD_FLOP = 2.0 * PIX * (9 * 128 + 64) * 128


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
    ap.add_argument("--out", default="profiles/r20_train_icnet_fusion_bench.json")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    net = models.ICNet(K)
    net.build((None, None, None, 3))
    synthetic.randomize_icnet(net, seed=0)
    x = synthetic.synth_frames_device(0, N, H, W, 3)
    scores, extra = net.score(x, return_label=True)
    labels = extra["label"].clone()
    mask = torch.ones((N, H, W), dtype=torch.float32, device=x.device)
    head = ICNetHeadTrainer(net, 5e-4, 0.9, 0.99, l2=2e-4, loginverse_scaling=1.02)
    tr = ICNetFusionTrainer(net, 5e-4, 0.9, 0.99, l2=2e-4, loginverse_scaling=1.02)
    s24, c3 = tr.features(x)
    tr.reinitialize(seed=0)
    src = torch.empty(256 << 20, dtype=torch.uint8, device=x.device)
    dst = torch.empty_like(src)
    rows = {
        "forward": lambda: net(x, training=False),
        "head_step": lambda: head.step(x, labels, mask),
        "step": lambda: tr.step(x, labels, mask),
        "step_features": lambda: tr.step_features(s24, c3, labels, mask),
        "grad_features": lambda: tr.gradient_features(s24, c3, labels, mask),
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
    copy_rate = 2.0 * src.numel() / (np.median(runs["copy"]) * 1e-3)  # bytes read + written per second
    floor_ms = sum(FLOOR_BYTES.values()) / copy_rate * 1e3
    out["copy_rate_GBps"] = copy_rate / 1e9
    out["wgrad_floor"] = {"bytes": FLOOR_BYTES, "ms_at_copy_rate": floor_ms, "flop": WGRAD_FLOP}
    print("copy rate %.0f GB/s; byte floor of k_icnet_fusion_wgrad %.0f MB = %.3f ms; %.1f GFLOP"
          % (copy_rate / 1e9, sum(FLOOR_BYTES.values()) / 1e6, floor_ms, WGRAD_FLOP / 1e9))
    if args.mfma_tflops:
        out["wgrad_floor"]["mfma_tflops"] = args.mfma_tflops
        out["wgrad_floor"]["ms_at_mfma_rate"] = WGRAD_FLOP / (args.mfma_tflops * 1e12) * 1e3
    _lib.profile_enable(True)
    for _ in range(3):
        tr.step(x, labels, mask)
    torch.cuda.synchronize()
    prof = _lib.profile_collect()
    _lib.profile_enable(False)
    out["kernels_3_steps"] = prof
    for kname, r in sorted(prof.items()):
        print("%-24s %.3f ms / launch, %.3g GFLOP, %.3g MB" % (kname, r["ms"] / r["launches"],
                                                                  r["flops"] / r["launches"] / 1e9,
                                                                  r["bytes"] / r["launches"] / 1e6), flush=True)
    if "k_icnet_fusion_wgrad" in prof:
        r = prof["k_icnet_fusion_wgrad"]
        ms = r["ms"] / r["launches"]
        out["wgrad_floor"]["kernel_ms"] = ms
        out["wgrad_floor"]["times_the_byte_floor"] = ms / floor_ms
        out["wgrad_floor"]["tflops"] = WGRAD_FLOP / (ms * 1e-3) / 1e12
        if args.mfma_tflops:
            out["wgrad_floor"]["times_the_mfma_floor"] = ms / out["wgrad_floor"]["ms_at_mfma_rate"]
    out["knobs"] = _lib.get_knobs()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
