"""Cost of ICNet's validation pass on one MI355X: ICNet(19), batch 8 x 1024 x 2048 uint8 frames, HIP-event timing.

Three passes run as INTERLEAVED windows (score, evaluate, composed, score, evaluate, ... : --repeats rounds of --steps batches
per window), so that every ratio is taken inside one process on one device within a few hundred milliseconds:
  score      the ranking pass (ICNet.score, margin, score only) -- the yardstick
  evaluate   the fused validation pass (ICNet.evaluate: argmax + confusion inside the up-sampling kernel, k_upeval)
  composed   ICNet._evaluate_composed: score(confidence, return_label=True) + tensortools.metrics.confusion_mat
with two label sets: the net's own predictions (every pixel on the diagonal: worst atomic contention) and random labels
with ~10 % void (255).  Reported per pass: images/s (median, min, max) and, per round, the paired ratios evaluate / composed
and evaluate / score with their spread.  Then the tail kernels' milliseconds per launch from the library's launch profiler
and k_upeval's distance from its byte floor (1/4-resolution logits + label and mask bytes at the measured HBM rate bench.py
uses).  Writes the record to --out.

    python tools/icnet_eval_bench.py [--repeats 7] [--steps 20] [--out profiles/r19_icnet_eval_bench.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from semanticsegmentationactivelearning_amd import _lib, models, synthetic  # noqa: E402

N, H, W, K = 8, 1024, 2048, 19
MEASURED_HBM_GBS = 6300.0  # bench.py's: best tile-organised copy on this part (profiles/r02_probes.txt)


def window(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return N * steps / (a.elapsed_time(b) / 1e3)


def interleaved(passes, steps, repeats, warmup=3):
    """{name: [images/s per round]}: round r runs one window of every pass, in the given order"""
    for fn in passes.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    rates = {name: [] for name in passes}
    for _ in range(repeats):
        for name, fn in passes.items():
            rates[name].append(window(fn, steps))
    return rates


def summary(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "all": [float(r) for r in v]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "r19_icnet_eval_bench.json"))
    args = ap.parse_args()

    torch.cuda.set_device(0)
    net = models.ICNet(K)
    net.build((None, H, W, 3))
    synthetic.randomize_icnet(net, seed=0)
    x = synthetic.synth_frames_device(0, N, H, W, 3, dtype=torch.uint8)
    _, extra = net.score(x, measure="confidence", return_label=True)
    own = extra["label"].contiguous()
    g = torch.Generator(device="cuda").manual_seed(0)
    rand = torch.randint(0, K, own.shape, dtype=torch.uint8, device="cuda", generator=g)
    rand[torch.rand(own.shape, device="cuda", generator=g) < 0.1] = 255
    label_sets = {"own_predictions": own, "random_10pct_void": rand}
    masks = {name: (lab != 255).to(torch.uint8) for name, lab in label_sets.items()}
    conf = torch.zeros((K, K), dtype=torch.int64, device="cuda")

    assert _lib.get_knobs()["defaults"], _lib.get_knobs()
    for name, lab in label_sets.items():  # what is timed computes the same matrix
        assert torch.equal(net.evaluate(x, lab, masks[name]), net._evaluate_composed(x, lab, masks[name])), name

    rec = {"shape": [N, H, W], "classes": K, "frames": "uint8", "steps": args.steps, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0), "knobs": _lib.get_knobs(), "label_sets": {}}
    for name, lab in label_sets.items():
        m = masks[name]
        rates = interleaved({"score": lambda: net.score(x, measure="margin"),
                             "evaluate": lambda: net.evaluate(x, lab, m, confusion=conf),
                             "composed": lambda: net._evaluate_composed(x, lab, m, confusion=conf)},
                            args.steps, args.repeats)
        row = {p: summary(v) for p, v in rates.items()}
        ev, co, sc = (np.asarray(rates[p]) for p in ("evaluate", "composed", "score"))
        row["evaluate_over_composed_pairs"] = summary(ev / co)
        row["evaluate_over_score_pairs"] = summary(ev / sc)
        rec["label_sets"][name] = row
        for p in ("score", "evaluate", "composed"):
            print("%-20s %-10s %8.1f images/s  (min %.1f max %.1f)" % (name, p, row[p]["median"], row[p]["min"], row[p]["max"]))
        for p in ("evaluate_over_composed_pairs", "evaluate_over_score_pairs"):
            print("%-20s %-30s median %.4f  (min %.4f max %.4f)" % (name, p, row[p]["median"], row[p]["min"], row[p]["max"]))

    # per-launch milliseconds of the tail kernels from the library's launch profiler (one chain while it is on)
    kern, launches = {}, 5
    for name, fn in (("score", lambda: net.score(x, measure="margin")),
                     ("evaluate", lambda: net.evaluate(x, rand, masks["random_10pct_void"], confusion=conf)),
                     ("evaluate_own", lambda: net.evaluate(x, own, masks["own_predictions"], confusion=conf)),
                     ("composed", lambda: net._evaluate_composed(x, rand, masks["random_10pct_void"], confusion=conf))):
        fn()
        torch.cuda.synchronize()
        _lib.profile_enable(True)
        for _ in range(launches):
            fn()
        torch.cuda.synchronize()
        prof = _lib.profile_collect()
        _lib.profile_enable(False)
        kern[name] = {k: v for k, v in prof.items() if "upscore" in k or "upeval" in k or "confusion" in k}
        print(name, json.dumps(kern[name]))
    rec["tail_kernels_%d_batches" % launches] = kern
    floor_bytes = 4.0 * N * (H // 4) * (W // 4) * K + 2.0 * N * H * W  # 1/4-resolution logits + label + mask bytes
    floor_ms = floor_bytes / (MEASURED_HBM_GBS * 1e9) * 1e3
    rec["k_upeval_byte_floor"] = {"bytes": floor_bytes, "hbm_gbs": MEASURED_HBM_GBS, "floor_ms": floor_ms}
    for name in ("evaluate", "evaluate_own"):
        ue = kern[name].get("k_upeval")
        if ue:
            ms = ue["ms"] / ue["launches"]
            rec["k_upeval_byte_floor"][name] = {"ms_per_launch": ms, "times_floor": ms / floor_ms}
            print("k_upeval (%s): %.4f ms per launch = %.2f x its byte floor of %.4f ms" % (name, ms, ms / floor_ms, floor_ms))
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
