"""Cost of one training step of ICNet through conv5_2 (the last two backbone bottlenecks under the pooling depth) on one MI355X:
ICNet(19), batch 8 x 1024 x 2048 float32 frames, HIP-event timing, everything in ONE process on ONE box.

Rows (ms per batch; median and min / max over --repeats timed windows of --steps batches each, the rows timed in
--repeats interleaved rounds so that drift of the box hits every row alike):
  bneck_step             ICNetBottleneckTrainer.step(images) -- the yardstick: the depth above, in the same run
  bneck_step_features    ICNetBottleneckTrainer.step_features on cached features
  bneck_grad_features    ICNetBottleneckTrainer.gradient_features on cached features
  step                   ICNetDeepBottleneckTrainer.step(images): the frozen trunk up to conv5_1 / conv3_1 / conv3_sub1, the
                         six layers of conv5_2 and conv5_3, the pyramid pooling, conv5_4_k1, both fusion blocks and the head on
                         the weights being trained, the gradient kernels, Adam, the copy back to the host and into the handle
  step_features          ICNetDeepBottleneckTrainer.step_features on cached features (no trunk)
  grad_features          the gradient alone on cached features (no Adam, no host copy)
  copy                   a device-to-device copy of 256 MB (the box's copy rate, read + write, the byte floors are held against)
The per-launch milliseconds come from the library's launch profiler in a separate pass: the new kernel against its byte floor
(every operand read once, every result written once) at the copy rate of the same run and against k_icnet_pool_dx, the same GEMM
shape without the two 1024-channel reads of the epilogue, whose time at the copy rate is the margin; the second run of each link
kernel next to the first.  Then section 15's 50-step run at 2 x 64 x 128 for both trainers: final / first loss.  Writes the
record to --out.

    python tools/train_icnet_bneck2_bench.py [--repeats 5] [--steps 10] [--out profiles/r30_train_icnet_bneck2_bench.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from semanticsegmentationactivelearning_amd import _lib, models, synthetic  # noqa: E402
from semanticsegmentationactivelearning_amd.training import ICNetBottleneckTrainer, ICNetDeepBottleneckTrainer  # noqa: E402

N, H, W, K = 8, 1024, 2048, 19
PIX16, PIX32 = (N * (H // d) * (W // d) for d in (16, 32))
# what each launch must move once, and its matrix-core work
FLOORS = {
    "k_icnet_bneck2_dx_red": {"bytes": {"gr": PIX32 * 256 * 4, "conv5_3_1x1_reduce.kernel": 1024 * 256 * 4, "g53": PIX32 * 1024 * 4,
                                        "conv5_2": PIX32 * 1024 * 4, "g52": PIX32 * 1024 * 4}, "flop": 2.0 * PIX32 * 1024 * 256},
    "k_icnet_pool_dx": {"bytes": {"g32": PIX32 * 256 * 4, "conv5_4_k1.kernel": 1024 * 256 * 4, "dsum": PIX32 * 1024 * 4},
                        "flop": 2.0 * PIX32 * 1024 * 256},
    "k_icnet_bneck2_wgrad_i": {"bytes": {"conv5_2_3x3": PIX32 * 256 * 4, "g52": PIX32 * 1024 * 4, "partials": 16 * 257 * 1024 * 4},
                               "flop": 2.0 * PIX32 * 257 * 1024},
}
# the link's launches: conv5_3's run, then conv5_2's
LINK = ("dx_inc", "wgrad3", "finish3", "gamma3", "dx_3x3", "wgrad_r", "finish_r", "gamma_r")
AL = {"hyperparams": {"learning_rate": 0.0005, "learning_rate_decay": 0.0,
                      "optimizer": {"type": "Adam", "kwargs": {"beta1": 0.9, "beta2": 0.99}},
                      "weight_reg": {"L2": 0.0002, "L1": 0.0},
                      "softmax": {"label_smoothing": 0.0, "loginverse_scaling": 1.02, "multiscale": False}}}


def window(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def fifty_steps(cls):
    """section 15's run: 2 x 64 x 128, the model's own labels, 50 steps on cached features -> final / first loss"""
    net = models.ICNet(K)
    net.build((None, None, None, 3))
    synthetic.randomize_icnet(net, seed=0)
    x = synthetic.synth_frames_device(0, 2, 64, 128, 3)
    _, extra = net.score(x, return_label=True)
    labels = extra["label"].clone()
    mask = torch.ones((2, 64, 128), dtype=torch.float32, device=x.device)
    tr = cls.from_params(net, AL)
    feats = tr.features(x)
    tr.reinitialize(seed=0)
    losses = [float(tr.step_features(*feats, labels, mask)) for _ in range(50)]
    return {"first": losses[0], "last": losses[-1], "ratio": losses[-1] / losses[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default="profiles/r30_train_icnet_bneck2_bench.json")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    net = models.ICNet(K)
    net.build((None, None, None, 3))
    synthetic.randomize_icnet(net, seed=0)
    x = synthetic.synth_frames_device(0, N, H, W, 3)
    scores, extra = net.score(x, return_label=True)
    labels = extra["label"].clone()
    mask = torch.ones((N, H, W), dtype=torch.float32, device=x.device)
    pool = ICNetBottleneckTrainer(net, 5e-4, 0.9, 0.99, l2=2e-4, loginverse_scaling=1.02)
    tr = ICNetDeepBottleneckTrainer(net, 5e-4, 0.9, 0.99, l2=2e-4, loginverse_scaling=1.02)
    pfeats = pool.features(x)
    feats = tr.features(x)
    tr.reinitialize(seed=0)
    src = torch.empty(256 << 20, dtype=torch.uint8, device=x.device)
    dst = torch.empty_like(src)
    rows = {
        "bneck_step": lambda: pool.step(x, labels, mask),
        "step": lambda: tr.step(x, labels, mask),
        "bneck_step_features": lambda: pool.step_features(*pfeats, labels, mask),
        "step_features": lambda: tr.step_features(*feats, labels, mask),
        "bneck_grad_features": lambda: pool.gradient_features(*pfeats, labels, mask),
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
        print("%-22s median %8.3f ms  [%8.3f, %8.3f]" % (name, np.median(v), min(v), max(v)), flush=True)
    out["step_over_bneck_step"] = float(np.median(runs["step"]) / np.median(runs["bneck_step"]))
    copy_rate = 2.0 * src.numel() / (np.median(runs["copy"]) * 1e-3)  # bytes read + written per second
    out["copy_rate_GBps"] = copy_rate / 1e9
    _lib.profile_enable(True)
    for _ in range(3):
        tr.step(x, labels, mask)
    torch.cuda.synchronize()
    prof = _lib.profile_collect()
    _lib.profile_enable(False)
    out["kernels_3_steps"] = prof
    out["floors"] = {}
    for kname, fl in FLOORS.items():
        floor_ms = sum(fl["bytes"].values()) / copy_rate * 1e3
        rec = {"bytes": fl["bytes"], "ms_at_copy_rate": floor_ms, "flop": fl["flop"], "kernel_ms": "not yet measured",
               "times_the_byte_floor": "not yet measured", "tflops": "not yet measured"}
        if kname in prof:
            ms = prof[kname]["ms"] / prof[kname]["launches"]
            rec.update(kernel_ms=ms, times_the_byte_floor=ms / floor_ms, tflops=fl["flop"] / (ms * 1e-3) / 1e12)
        out["floors"][kname] = rec
        print("%s: byte floor %.3f ms, %.1f GFLOP, kernel %s ms, x%s the floor"
              % (kname, floor_ms, fl["flop"] / 1e9, rec["kernel_ms"], rec["times_the_byte_floor"]), flush=True)
    per = lambda name: prof[name]["ms"] / prof[name]["launches"] if name in prof else "not yet measured"
    # the margin the new kernel may take over k_icnet_pool_dx: its two further 1024-channel reads at the copy rate
    margin_ms = 2.0 * PIX32 * 1024 * 4 / copy_rate * 1e3
    out["dx_red_against_pool_dx"] = {"k_icnet_bneck2_dx_red_ms": per("k_icnet_bneck2_dx_red"), "k_icnet_pool_dx_ms": per("k_icnet_pool_dx"),
                                     "margin_ms_two_reads_at_copy_rate": margin_ms}
    out["link_first_and_second_run_ms"] = {k_: {"conv5_3": per("k_icnet_bneck_" + k_), "conv5_2": per("k_icnet_bneck2_" + k_)}
                                           for k_ in LINK}
    print("new kernel against k_icnet_pool_dx:", out["dx_red_against_pool_dx"], flush=True)
    print("link, first and second run:", out["link_first_and_second_run_ms"], flush=True)
    out["fifty_steps"] = {"ICNetBottleneckTrainer": fifty_steps(ICNetBottleneckTrainer),
                          "ICNetDeepBottleneckTrainer": fifty_steps(ICNetDeepBottleneckTrainer)}
    print("50 steps, final / first loss:", {k: round(v["ratio"], 6) for k, v in out["fifty_steps"].items()})
    out["knobs"] = _lib.get_knobs()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
