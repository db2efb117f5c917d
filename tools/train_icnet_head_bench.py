"""Cost of one training step of ICNet's output layer on one MI355X: ICNet(19), batch 8 x 1024 x 2048 float32 frames,
HIP-event timing, everything in ONE process on ONE box.

Rows (ms per batch; median and min / max over --repeats timed windows of --steps batches each, the rows timed in
--repeats interleaved rounds so that drift of the box hits every row alike):
  forward          net(x, training=False) -- the yardstick (trunk + conv6_cls + the 4x resize, logits written)
  step             ICNetHeadTrainer.step(images): trunk up to sub12_sum + the head launch + k_icnet_head_grad + finish + Adam
                   + the copy of the 10 KB head back to the host variables and into the handle
  step_features    ICNetHeadTrainer.step_features on cached sub12_sum features (no trunk)
  grad_features    the gradient alone on cached features (pack + head launch + k_icnet_head_grad + finish; no Adam, no host copy)
  copy             a device-to-device copy of 256 MB (the box's copy rate, read + write, the byte floor is held against)
The per-kernel milliseconds come from the library's launch profiler in a separate pass.  Writes the record to --out.

    python tools/train_icnet_head_bench.py [--repeats 5] [--steps 10] [--out profiles/r16_train_icnet_head_bench.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from semanticsegmentationactivelearning_amd import _lib, models, synthetic  # noqa: E402
from semanticsegmentationactivelearning_amd.training import ICNetHeadTrainer  # noqa: E402

N, H, W, K = 8, 1024, 2048, 19
# what k_icnet_head_grad must move: sub12_sum, lq, labels, mask (the partial rows are 10 MB more, written once)
FLOOR_BYTES = {"sub12_sum": N * (H // 8) * (W // 8) * 128 * 4, "lq": N * (H // 4) * (W // 4) * K * 4, "labels": N * H * W,
               "mask": N * H * W * 4}


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
    ap.add_argument("--out", default="profiles/r16_train_icnet_head_bench.json")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    net = models.ICNet(K)
    net.build((None, None, None, 3))
    synthetic.randomize_icnet(net, seed=0)
    x = synthetic.synth_frames_device(0, N, H, W, 3)
    scores, extra = net.score(x, return_label=True)
    labels = extra["label"].clone()
    mask = torch.ones((N, H, W), dtype=torch.float32, device=x.device)
    tr = ICNetHeadTrainer(net, 5e-4, 0.9, 0.99, l2=2e-4, loginverse_scaling=1.02)
    feats = tr.features(x)
    tr.reinitialize(seed=0)
    src = torch.empty(256 << 20, dtype=torch.uint8, device=x.device)
    dst = torch.empty_like(src)
    rows = {
        "forward": lambda: net(x, training=False),
        "step": lambda: tr.step(x, labels, mask),
        "step_features": lambda: tr.step_features(feats, labels, mask),
        "grad_features": lambda: tr.gradient_features(feats, labels, mask),
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
    out["head_grad_floor"] = {"bytes": FLOOR_BYTES, "ms_at_copy_rate": floor_ms}
    print("copy rate %.0f GB/s; byte floor of k_icnet_head_grad %.0f MB = %.3f ms" % (copy_rate / 1e9,
                                                                                    sum(FLOOR_BYTES.values()) / 1e6, floor_ms))
    _lib.profile_enable(True)
    for _ in range(3):
        tr.step(x, labels, mask)
    torch.cuda.synchronize()
    prof = _lib.profile_collect()
    _lib.profile_enable(False)
    out["kernels_3_steps"] = prof
    for kname in ("k_icnet_head_pack", "k_conv1x1_up2_c128", "k_icnet_head_grad", "k_icnet_head_finish", "k_adam"):
        if kname in prof:
            r = prof[kname]
            print("%-20s %.3f ms / launch, %.3g GFLOP, %.3g MB" % (kname, r["ms"] / r["launches"],
                                                                  r["flops"] / r["launches"] / 1e9,
                                                                  r["bytes"] / r["launches"] / 1e6), flush=True)
    if "k_icnet_head_grad" in prof:
        r = prof["k_icnet_head_grad"]
        out["head_grad_floor"]["kernel_ms"] = r["ms"] / r["launches"]
        out["head_grad_floor"]["times_the_floor"] = r["ms"] / r["launches"] / floor_ms
    out["knobs"] = _lib.get_knobs()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
