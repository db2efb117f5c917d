"""Cost of one decoder training step (Bottleneck4_0 + Bottleneck4_1 + Bottleneck4_2 + Bottleneck5_0 + Bottleneck5_1 + Final,
DESIGN.md section 22) on one MI355X next to the deep-tail step: ENet(19), batch 8 x 1024 x 2048 float32 frames, HIP-event timing, everything
in ONE process on ONE box.

Rows (ms per batch; median and min / max over --repeats timed windows of --steps batches each, the rows timed in
--repeats interleaved rounds so that drift of the box hits every row alike):
  forward                net(x, training=False) -- the yardstick (trunk + Final, logits written)
  deep_step              DeepTailTrainer.step(images)
  decoder_step           DecoderTrainer.step(images): the encoder up to Bottleneck3_8 + k_td_fold and the scoring path's
                         128-channel upsample kernel + the deep tail's launches (k_tt_block<true> twice) + k_td_block + k_td_res +
                         k_td_finish + Adam + the copy of the packed block back
  deep_step_features     DeepTailTrainer.step_features on cached Bottleneck4_0 features and pooling indices
  decoder_step_features  DecoderTrainer.step_features on cached Bottleneck3_8 features and both sets of pooling indices
The per-kernel milliseconds, FLOP and byte counts (from the code) come from the library's launch profiler in a separate pass;
the HBM roofline time is bytes / 5 TB/s, the distance is ms over that, and "bound" says what the launch waits for.  Writes the record to --out.

    python tools/train_decoder_bench.py [--repeats 5] [--steps 10] [--out profiles/r15_train_decoder_bench.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from semanticsegmentationactivelearning_amd import _lib, models, synthetic  # noqa: E402
from semanticsegmentationactivelearning_amd.training import DecoderTrainer, DeepTailTrainer  # noqa: E402

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
    ap.add_argument("--out", default="profiles/r15_train_decoder_bench.json")
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
    tt = DeepTailTrainer(net, 5e-4, 0.9, 0.99, l2=2e-4, loginverse_scaling=1.02)
    td = DecoderTrainer(net2, 5e-4, 0.9, 0.99, l2=2e-4, loginverse_scaling=1.02)
    tt.reinitialize(seed=0)
    td.reinitialize(seed=0)
    feats40, argmax1 = tt.features(x)  # Bottleneck4_0's output, Bottleneck1_0's pooling indices
    feats38, argmax2, _ = td.features(x)  # Bottleneck3_8's output, Bottleneck2_0's pooling indices
    rows = {
        "forward": lambda: net(x, training=False),
        "deep_step": lambda: tt.step(x, labels, mask),
        "decoder_step": lambda: td.step(x, labels, mask),
        "deep_step_features": lambda: tt.step_features(feats40, argmax1, labels, mask),
        "decoder_step_features": lambda: td.step_features(feats38, argmax2, argmax1, labels, mask),
    }
    for fn in rows.values():  # warm-up: workspaces, handle pushes, code objects
        fn()
        fn()
    torch.cuda.synchronize()
    runs = {k: [] for k in rows}
    for _ in range(args.repeats):
        for name, fn in rows.items():
            runs[name].append(window(fn, args.steps))
    out = {"command": "python tools/train_decoder_bench.py --repeats %d --steps %d" % (args.repeats, args.steps),
           "batch": [N, H, W, K], "steps_per_window": args.steps, "rows_ms_per_batch": {}}
    for name, v in runs.items():
        out["rows_ms_per_batch"][name] = {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)),
                                          "repeats": v}
        print("%-22s median %8.3f ms  [%8.3f, %8.3f]" % (name, np.median(v), min(v), max(v)), flush=True)
    _lib.profile_enable(True)
    for _ in range(3):
        td.step_features(feats38, argmax2, argmax1, labels, mask)
    torch.cuda.synchronize()
    prof = _lib.profile_collect()
    _lib.profile_enable(False)
    out["kernels_3_steps"] = prof
    out["hbm_roofline_ms_at_5TBps"], out["distance_to_byte_floor"] = {}, {}
    out["decoder_over_deep"] = {a: out["rows_ms_per_batch"]["decoder_" + a]["median"] / out["rows_ms_per_batch"]["deep_" + a]["median"]
                                for a in ("step", "step_features")}
    print("decoder / deep: step x%.3f, step_features x%.3f" % (out["decoder_over_deep"]["step"],
                                                               out["decoder_over_deep"]["step_features"]))
    # every launch of the pass, the new kernels first
    first = ("k_td_block", "k_td_res", "k_td_finish", "k_upsample_mfma", "k_tt_block<dx>", "k_tt_finish", "k_ts_block")
    for kname in list(first) + sorted(k for k in prof if k not in first):
        if kname in prof:
            r = prof[kname]
            ms = r["ms"] / r["launches"]
            roof = r["bytes"] / r["launches"] / 5e12 * 1e3
            out["hbm_roofline_ms_at_5TBps"][kname] = roof
            out["distance_to_byte_floor"][kname] = ms / roof if roof > 0 else None
            print("%-22s %.3f ms / launch, %.3g GFLOP, %.3g MB, HBM roofline %.3f ms, x%.1f" % (
                kname, ms, r["flops"] / r["launches"] / 1e9, r["bytes"] / r["launches"] / 1e6, roof,
                ms / roof if roof > 0 else float("nan")), flush=True)
    out["knobs"] = _lib.get_knobs()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
