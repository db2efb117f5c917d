"""Cost of the validation pass on one MI355X: ENet(19), batch 8 x 1024 x 2048 uint8 frames, HIP-event timing.

Rows (images/s; median and min / max over --repeats timed windows of --steps batches each):
  score       the ranking pass (ENet.score, entropy, score only) -- the yardstick
  evaluate    the fused validation pass (ENet.evaluate: argmax + confusion inside the Final kernel)
  unfused     ENet.score(return_label=True) + tensortools.metrics.confusion_mat on the label plane
each with two label sets: the net's own predictions (every pixel on the diagonal: worst atomic contention) and random
labels with ~10 % void (255).  Then the fused pass over conf_reps (replicas of the confusion accumulator) in {1, 8, 32}
on the diagonal labels, and the per-kernel milliseconds of the evaluation tail against k_final_score<fused 5_1> from the
library's own launch profiler (one chain: the profiler brackets every launch).  Writes the record to --out.

    python tools/eval_bench.py [--repeats 5] [--steps 20] [--out profiles/r06_eval_bench.json]
    python tools/eval_bench.py --once     # one score + one evaluate batch (for a rocprofv3 --kernel-trace --stats run)
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from semanticsegmentationactivelearning_amd import _lib, models, synthetic  # noqa: E402
from semanticsegmentationactivelearning_amd.tensortools import metrics as M  # noqa: E402

N, H, W, K = 8, 1024, 2048, 19


def timed(fn, steps, repeats, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    rates = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        b.synchronize()
        rates.append(N * steps / (a.elapsed_time(b) / 1e3))
    return {"median": float(np.median(rates)), "min": float(min(rates)), "max": float(max(rates)), "all": rates}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "r06_eval_bench.json"))
    args = ap.parse_args()

    torch.cuda.set_device(0)
    net = models.ENet(K)
    net.build((None, H, W, 3))
    synthetic.randomize_enet(net, seed=0)
    x = synthetic.synth_frames_device(0, N, H, W, 3, dtype=torch.uint8)
    _, extra = net.score(x, measure="entropy", return_label=True)
    own = extra["label"].contiguous()
    g = torch.Generator(device="cuda").manual_seed(0)
    rand = torch.randint(0, K, own.shape, dtype=torch.uint8, device="cuda", generator=g)
    rand[torch.rand(own.shape, device="cuda", generator=g) < 0.1] = 255
    label_sets = {"own_predictions": own, "random_10pct_void": rand}
    masks = {name: (lab != 255).to(torch.uint8) for name, lab in label_sets.items()}
    conf = torch.zeros((K, K), dtype=torch.int64, device="cuda")

    if args.once:
        net.score(x, measure="entropy")
        net.evaluate(x, own, masks["own_predictions"], confusion=conf)
        torch.cuda.synchronize()
        print("once: score + evaluate, batch %d x %d x %d" % (N, H, W))
        return

    assert _lib.get_knobs()["defaults"], _lib.get_knobs()
    # correctness of what is timed: the fused matrix equals the unfused one
    for name, lab in label_sets.items():
        a = net.evaluate(x, lab, masks[name])
        _, e = net.score(x, measure="entropy", return_label=True)
        b = M.confusion_mat(lab, e["label"], K, weights=masks[name])
        assert torch.equal(a, b), name

    rec = {"shape": [N, H, W], "classes": K, "frames": "uint8", "steps": args.steps, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0), "knobs": _lib.get_knobs(), "rows": {}}
    rows = rec["rows"]
    rows["score"] = timed(lambda: net.score(x, measure="entropy"), args.steps, args.repeats)
    for name, lab in label_sets.items():
        m = masks[name]
        rows["evaluate/" + name] = timed(lambda: net.evaluate(x, lab, m, confusion=conf), args.steps, args.repeats)

        def unfused():
            _, e = net.score(x, measure="entropy", return_label=True)
            M.confusion_mat(lab, e["label"], K, weights=m, out=conf)
        rows["unfused/" + name] = timed(unfused, args.steps, args.repeats)
    try:
        for reps in (1, 8, 32):
            _lib.set_knob("conf_reps", reps)
            for name in label_sets:
                rows["evaluate/%s/conf_reps=%d" % (name, reps)] = timed(
                    lambda: net.evaluate(x, label_sets[name], masks[name], confusion=conf), args.steps, args.repeats)
    finally:
        _lib.set_knob("conf_reps", 8)
    base = rows["score"]["median"]
    for key, r in rows.items():
        r["vs_score"] = r["median"] / base
        print("%-44s %8.1f images/s  (min %.1f max %.1f)  %.4f x score" % (key, r["median"], r["min"], r["max"],
                                                                           r["vs_score"]))

    # per-kernel milliseconds from the library's launch profiler (one chain while it is on)
    kern = {}
    for name, fn in (("score", lambda: net.score(x, measure="entropy")),
                     ("evaluate/own_predictions", lambda: net.evaluate(x, own, masks["own_predictions"], confusion=conf)),
                     ("evaluate/random_10pct_void", lambda: net.evaluate(x, rand, masks["random_10pct_void"], confusion=conf))):
        fn()
        torch.cuda.synchronize()
        _lib.profile_enable(True)
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        prof = _lib.profile_collect()
        _lib.profile_enable(False)
        kern[name] = {k: v for k, v in prof.items() if "final" in k or "confusion" in k}
        print(name, json.dumps(kern[name]))
    rec["tail_kernels_5_batches"] = kern
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
