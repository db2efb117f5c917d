#!/usr/bin/env python
"""ICNet high-resolution-branch training step on one MI355X: ms per batch, median [min, max] of
interleaved windows, for ``ICNetCascadeTrainer.step(images)`` (the yardstick, same run), ``ICNetHighResTrainer.step(images)``,
``step_features`` on cached backbone features, the gradient alone and a 256 MB device copy; then the per-launch times of the
library's launch profiler for every ``k_icnet_highres_*`` kernel with its distance from its byte floor at the copy rate measured
here.  Writes profiles/r24_train_icnet_highres_bench.json.

    python tools/train_icnet_highres_bench.py [--batch 8 --height 1024 --width 2048 --classes 19 --windows 5 --steps 10]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import semanticsegmentationactivelearning_amd as ssal  # noqa: E402
from semanticsegmentationactivelearning_amd import _lib, synthetic as syn  # noqa: E402
from semanticsegmentationactivelearning_amd.training import ICNetCascadeTrainer, ICNetHighResTrainer  # noqa: E402


def _window(fn, steps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--classes", type=int, default=19)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_train_icnet_highres_bench.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    n, h, w, k = a.batch, a.height, a.width, a.classes

    def trainer(cls):
        net = ssal.ICNet(k)
        net.build((None, None, None, 3))
        syn.randomize_icnet(net, seed=0)
        return cls(net, 5e-4, 0.9, 0.99, loginverse_scaling=1.02, l2=2e-4)

    cas, hr = trainer(ICNetCascadeTrainer), trainer(ICNetHighResTrainer)
    x = syn.synth_frames_device(0, n, h, w, 3, dtype=torch.uint8)
    rng = np.random.default_rng(0)
    labels = torch.as_tensor(rng.integers(0, k, (n, h, w)).astype(np.uint8)).cuda()
    mask = torch.ones((n, h, w), dtype=torch.float32, device="cuda")
    feats = hr.features(x)
    src = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    rows = {"ICNetCascadeTrainer.step(images)": lambda: cas.step(x, labels, mask),
            "ICNetHighResTrainer.step(images)": lambda: hr.step(x, labels, mask),
            "ICNetHighResTrainer.step_features": lambda: hr.step_features(*feats, x, labels, mask),
            "ICNetHighResTrainer.gradient_features": lambda: hr.gradient_features(*feats, x, labels, mask),
            "copy 256 MB": lambda: dst.copy_(src)}
    for fn in rows.values():  # warm-up
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in rows}
    for _ in range(a.windows):  # interleaved windows
        for name, fn in rows.items():
            times[name].append(_window(fn, a.steps))
    result = {"batch": [n, h, w], "classes": k, "windows": a.windows, "steps": a.steps, "ms": {}}
    for name, t in times.items():
        result["ms"][name] = {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t))}
        print("%-42s %8.3f ms  [%.3f, %.3f]" % (name, np.median(t), min(t), max(t)))
    copy_gbs = 2.0 * 256 * (1 << 20) / (result["ms"]["copy 256 MB"]["median"] * 1e-3) / 1e9
    result["copy_GBps"] = copy_gbs
    # per-launch times of the new kernels (the launch profiler serialises the launches: one call, not a timing of the step)
    _lib.profile_enable(True)
    hr.gradient_features(*feats, x, labels, mask)
    torch.cuda.synchronize()
    prof = _lib.profile_collect()
    _lib.profile_enable(False)
    result["launches"] = {}
    for name, rec in prof.items():  # {kernel: {"launches", "ms", "flops", "bytes"}}
        if "highres" not in name:
            continue
        entry = dict(rec)
        per_launch = rec["ms"] / max(rec["launches"], 1)
        entry["ms_per_launch"] = per_launch
        if rec.get("bytes"):
            entry["x_byte_floor"] = per_launch * 1e-3 / (rec["bytes"] / max(rec["launches"], 1) / (copy_gbs * 1e9))
        if rec.get("flops"):
            entry["TFLOPs"] = rec["flops"] / max(rec["launches"], 1) / (per_launch * 1e-3) / 1e12
        result["launches"][name] = entry
        print(name, entry)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
