"""Cost of one SEMI-SUPERVISED training step of the last-block and last-stage trainers on one MI355X:
ENet(19), batch 8 x 1024 x 2048 float32 frames, entropy, images 1, 3, 5, 7 unlabelled, threshold = the median confidence of
the batch.  HIP-event timing, everything in ONE process on ONE box.

Rows, per trainer (ms per batch; median and min / max over --repeats timed windows of --steps batches each, the rows timed in
--repeats interleaved rounds so that drift of the box hits every row alike):
  a_plain_step        step(images, labels, mask): the parent class's supervised step, the cost floor
  b_fused_semi        step(..., labelled, confusion, return_pseudo_pixels): pseudo annotation + metrics in the head kernel
  c_fused_semi_raw    the same with images_raw (a second trunk pass and the target-only launch)
  d_composed          features(images), the model layers' logits, score_logits, training_targets, the plain step
  e_composed_metrics  d plus the training-pass confusion matrix (argmax of the training logits + confusion_mat)
The per-kernel milliseconds of k_tb_head in its forms come from the library's launch profiler in a separate pass.

    python tools/train_deep_semi_bench.py [--repeats 5] [--steps 10] [--out profiles/r12_train_deep_semi_bench.json]
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
from semanticsegmentationactivelearning_amd.tensortools import metrics  # noqa: E402
from semanticsegmentationactivelearning_amd.training import SemiSupervisedBlockTrainer, SemiSupervisedStageTrainer  # noqa: E402

N, H, W, K = 8, 1024, 2048, 19


def window(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def bench(cls, args, x, x_raw):
    net = models.ENet(K)
    net.build((None, None, None, 3))
    synthetic.randomize_enet(net, seed=0)
    _, extra = net.score(x_raw, return_label=True)
    labels = extra["label"].clone()
    mask = torch.ones((N, H, W), dtype=torch.float32, device=x.device)
    sel = torch.tensor([i % 2 == 0 for i in range(N)], device=x.device)  # images 1, 3, 5, 7 are unlabelled
    tr = cls(net, 5e-4, 0.9, 0.99, l2=2e-4, loginverse_scaling=1.02)
    tr.reinitialize(seed=0)
    _, extra = net.score(x, "entropy", return_confidence=True)
    v = extra["confidence"].flatten()
    thr = float(np.median(v[:: (v.numel() // 1000003) | 1].cpu().numpy()))
    del extra, v
    conf = torch.zeros((K, K), dtype=torch.int64, device=x.device)
    stage = cls is SemiSupervisedStageTrainer

    def composed(with_metrics):
        f = tr.features(x)
        a5 = net.Bottleneck5_0(f[0], f[1], training=False) if stage else f
        logits = net.Final(net.Bottleneck5_1(a5, training=False), training=False)
        _, p = al.score_logits(logits, "entropy", thr, return_label=True, return_mask=True)
        lab, mk = al.training_targets(sel, labels, mask, p["label"], p["mask"].float())
        if with_metrics:
            _, pt = al.score_logits(logits, "confidence", 0.0, return_label=True)
            metrics.confusion_mat(lab, pt["label"], K, weights=mk, out=conf)
        return tr.step(x, lab, mk)

    rows = {
        "a_plain_step": lambda: tr.step(x, labels, mask),
        "b_fused_semi": lambda: tr.step(x, labels, mask, labelled=sel, measure="entropy", threshold=thr, confusion=conf,
                                        return_pseudo_pixels=True),
        "c_fused_semi_raw": lambda: tr.step(x, labels, mask, labelled=sel, measure="entropy", threshold=thr,
                                            images_raw=x_raw, confusion=conf, return_pseudo_pixels=True),
        "d_composed": lambda: composed(False),
        "e_composed_metrics": lambda: composed(True),
    }
    for fn in rows.values():  # warm-up: workspaces, handle pushes, code objects
        fn()
        fn()
    torch.cuda.synchronize()
    _, pp = rows["b_fused_semi"]()
    share = float(pp.sum()) / (int((~sel).sum()) * H * W)
    print("%s: threshold %.6g: %.3f of the unlabelled frames' pixels pass it" % (cls.__name__, thr, share), flush=True)
    runs = {k: [] for k in rows}
    for _ in range(args.repeats):
        for name, fn in rows.items():
            runs[name].append(window(fn, args.steps))
    out = {"threshold": thr, "unlabelled": int((~sel).sum()), "pseudo_mask_share": share, "rows_ms_per_batch": {}}
    for name, v in runs.items():
        out["rows_ms_per_batch"][name] = {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)),
                                          "repeats": v}
        print("%-20s median %8.3f ms  [%8.3f, %8.3f]" % (name, np.median(v), min(v), max(v)), flush=True)
    r = out["rows_ms_per_batch"]
    out["b_over_d_median"] = r["b_fused_semi"]["median"] / r["d_composed"]["median"]
    out["b_over_a_median"] = r["b_fused_semi"]["median"] / r["a_plain_step"]["median"]
    out["b_max_below_d_min"] = bool(r["b_fused_semi"]["max"] < r["d_composed"]["min"])
    print("b / d = %.3f (max of b below min of d: %s), b / a = %.3f"
          % (out["b_over_d_median"], out["b_max_below_d_min"], out["b_over_a_median"]), flush=True)
    out["kernels_3_steps"] = {}
    for name in ("a_plain_step", "b_fused_semi", "c_fused_semi_raw"):
        _lib.profile_enable(True)
        for _ in range(3):
            rows[name]()
        torch.cuda.synchronize()
        prof = _lib.profile_collect()
        _lib.profile_enable(False)
        out["kernels_3_steps"][name] = prof
        for kname in ("k_tb_head", "k_tb_head_semi", "k_tb_head_targets", "k_confusion_fold"):
            if kname in prof:
                print("%-18s %-20s %.3f ms / launch" % (name, kname, prof[kname]["ms"] / prof[kname]["launches"]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default="profiles/r12_train_deep_semi_bench.json")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    x_raw = synthetic.synth_frames_device(0, N, H, W, 3)
    x = (x_raw * torch.tensor([0.9, 1.1, 0.8], device=x_raw.device)).contiguous()  # a colour-distorted copy
    out = {"batch": [N, H, W, K], "measure": "entropy", "steps_per_window": args.steps}
    for cls in (SemiSupervisedBlockTrainer, SemiSupervisedStageTrainer):
        out[cls.__name__] = bench(cls, args, x, x_raw)
        torch.cuda.empty_cache()
    out["knobs"] = _lib.get_knobs()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
