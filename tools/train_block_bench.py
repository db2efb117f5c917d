"""Cost of one last-block training step (Bottleneck5_1 + Final) on one MI355X next to the output-layer
step: ENet(19), batch 8 x 1024 x 2048 float32 frames, HIP-event timing, everything in ONE process on ONE box.

Rows (ms per batch; median and min / max over --repeats timed windows of --steps batches each, the rows timed in
--repeats interleaved rounds so that drift of the box hits every row alike):
  forward                net(x, training=False) -- the yardstick (trunk + Final, logits written)
  final_step             FinalLayerTrainer.step(images)
  block_step             LastBlockTrainer.step(images): trunk up to Bottleneck5_0 + k_tb_head + k_tb_block + finish + Adam + the
                         12.5 KB copy of the packed block back to the host variables
  final_step_features    FinalLayerTrainer.step_features on cached Bottleneck5_1 features
  block_step_features    LastBlockTrainer.step_features on cached Bottleneck5_0 features
The per-kernel milliseconds, FLOP and byte counts come from the library's launch profiler in a separate pass; the HBM
roofline time is bytes / 5 TB/s.  Writes the record to --out.

    python tools/train_block_bench.py [--repeats 5] [--steps 10] [--out profiles/r10_train_block_bench.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from semanticsegmentationactivelearning_amd import _lib, models, synthetic  # noqa: E402
from semanticsegmentationactivelearning_amd.training import FinalLayerTrainer, LastBlockTrainer  # noqa: E402

N, H, W, K = 8, 1024, 2048, 19


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
    ap.add_argument("--out", default="profiles/r10_train_block_bench.json")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    net = models.ENet(K)
    net.build((None, None, None, 3))
    synthetic.randomize_enet(net, seed=0)
    x = synthetic.synth_frames_device(0, N, H, W, 3)
    scores, extra = net.score(x, return_label=True)
    labels = extra["label"].clone()
    mask = torch.ones((N, H, W), dtype=torch.float32, device=x.device)
    net2 = models.ENet(K)  # the two trainers write different variables: a model each, the same start
    net2.build((None, None, None, 3))
    synthetic.randomize_enet(net2, seed=0)
    tr = FinalLayerTrainer(net, 5e-4, 0.9, 0.99, l2=2e-4, loginverse_scaling=1.02)
    tb = LastBlockTrainer(net2, 5e-4, 0.9, 0.99, l2=2e-4, loginverse_scaling=1.02)
    tr.reinitialize(seed=0)
    tb.reinitialize(seed=0)
    net(x, training=False)
    feats = net.endpoint_outputs[0][1].clone()
    feats0 = tb.features(x)  # Bottleneck5_0's output
    rows = {
        "forward": lambda: net(x, training=False),
        "final_step": lambda: tr.step(x, labels, mask),
        "block_step": lambda: tb.step(x, labels, mask),
        "final_step_features": lambda: tr.step_features(feats, labels, mask),
        "block_step_features": lambda: tb.step_features(feats0, labels, mask),
    }
    for fn in rows.values():  # warm-up: workspaces, handle pushes, code objects
        fn()
        fn()
    torch.cuda.synchronize()
    runs = {k: [] for k in rows}
    for _ in range(args.repeats):
        for name, fn in rows.items():
            runs[name].append(window(fn, args.steps))
    out = {"command": "python tools/train_block_bench.py --repeats %d --steps %d" % (args.repeats, args.steps),
           "batch": [N, H, W, K], "steps_per_window": args.steps, "rows_ms_per_batch": {}}
    for name, v in runs.items():
        out["rows_ms_per_batch"][name] = {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)),
                                          "repeats": v}
        print("%-20s median %8.3f ms  [%8.3f, %8.3f]" % (name, np.median(v), min(v), max(v)), flush=True)
    _lib.profile_enable(True)
    for _ in range(3):
        tb.step(x, labels, mask)
    torch.cuda.synchronize()
    prof = _lib.profile_collect()
    _lib.profile_enable(False)
    out["kernels_3_steps"] = prof
    out["hbm_roofline_ms_at_5TBps"] = {}
    for kname in ("k_tb_fold", "k_tb_head", "k_tb_block", "k_tb_finish", "k_adam"):
        if kname in prof:
            r = prof[kname]
            roof = r["bytes"] / r["launches"] / 5e12 * 1e3
            out["hbm_roofline_ms_at_5TBps"][kname] = roof
            print("%-12s %.3f ms / launch, %.3g GFLOP, %.3g MB, HBM roofline %.3f ms" % (
                kname, r["ms"] / r["launches"], r["flops"] / r["launches"] / 1e9, r["bytes"] / r["launches"] / 1e6, roof),
                flush=True)
    out["knobs"] = _lib.get_knobs()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
