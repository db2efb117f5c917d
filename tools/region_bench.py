"""Cost of region-level acquisition on one MI355X: ENet(19), batch 8 x 1024 x 2048 uint8 frames, entropy, HIP-event timing,
everything in ONE process on ONE box.

Rows (images/s; median and min / max over --repeats timed windows of --steps batches each; the rows are timed in
--repeats interleaved rounds so that drift of the box hits every row alike):
  score                 the plain ranking pass (ENet.score, score only) -- the yardstick
  regions/32|128|512    ENet.score_regions, fused route (tile partials of the Final kernel + k_reduce_regions)
  plane/128             the plane route: ENet.score(return_confidence=True) + ssal_region_means_plane
  icnet/score           ICNet.score (margin), batch 8 x 1024 x 2048
  icnet/regions/128     ICNet.score_regions (its only route: the confidence plane + k_region_means_plane)
`regions/128` passes when its median lies within the min-max spread of `score`'s own repeats, or above it.  The per-kernel
milliseconds of k_reduce_regions / k_region_means_plane come from the library's own launch profiler (one chain while it is
on).  Writes the record, every repeat included, to --out.

    python tools/region_bench.py [--repeats 5] [--steps 20] [--out profiles/r07_region_bench.json]
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


def window(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return N * steps / (a.elapsed_time(b) / 1e3)


def timed_interleaved(fns, steps, repeats, warmup=3):
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    rates = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            rates[k].append(window(fn, steps))
    return {k: {"median": float(np.median(r)), "min": float(min(r)), "max": float(max(r)), "all": r} for k, r in rates.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "r07_region_bench.json"))
    args = ap.parse_args()

    torch.cuda.set_device(0)
    assert _lib.get_knobs()["defaults"], _lib.get_knobs()
    net = models.ENet(K)
    net.build((None, H, W, 3))
    synthetic.randomize_enet(net, seed=0)
    x = synthetic.synth_frames_device(0, N, H, W, 3, dtype=torch.uint8)

    # correctness of what is timed: same image scores, and the two routes agree
    s0 = net.score(x, measure="entropy")
    s1, fused = net.score_regions(x, region=128, measure="entropy")
    assert torch.equal(s0, s1)
    _, e = net.score(x, measure="entropy", return_confidence=True)
    plane = _lib.region_means_plane(e["confidence"], 128)
    route_diff = float((fused - plane).abs().max())
    assert route_diff <= 1e-9, route_diff
    del e, plane

    def plane_route():
        _, m = net.score(x, measure="entropy", return_confidence=True)
        _lib.region_means_plane(m["confidence"], 128)

    rec = {"shape": [N, H, W], "classes": K, "frames": "uint8", "measure": "entropy", "steps": args.steps,
           "repeats": args.repeats, "device": torch.cuda.get_device_name(0), "knobs": _lib.get_knobs(),
           "fused_vs_plane_max_abs_diff": route_diff}
    fns = {"score": lambda: net.score(x, measure="entropy")}
    for r in (32, 128, 512):
        fns["regions/%d" % r] = (lambda r=r: net.score_regions(x, region=r, measure="entropy"))
    fns["plane/128"] = plane_route
    rows = rec["rows"] = timed_interleaved(fns, args.steps, args.repeats)
    base = rows["score"]
    for key, r in rows.items():
        r["vs_score"] = r["median"] / base["median"]
    rec["regions_128_within_score_spread"] = bool(rows["regions/128"]["median"] >= base["min"])

    # per-kernel milliseconds (launch profiler: one chain, every launch bracketed)
    kern = {}
    for name, fn in (("regions/128", fns["regions/128"]), ("regions/512", fns["regions/512"]), ("plane/128", plane_route)):
        fn()
        torch.cuda.synchronize()
        _lib.profile_enable(True)
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        prof = _lib.profile_collect()
        _lib.profile_enable(False)
        kern[name] = {k: v for k, v in prof.items() if "region" in k or "final" in k or "reduce" in k}
    rec["tail_kernels_5_batches"] = kern
    del net, x
    torch.cuda.empty_cache()

    # ICNet: its region route is the plane route
    icn = models.ICNet(K)
    icn.build((None, H, W, 3))
    synthetic.randomize_icnet(icn, seed=0)
    xi = synthetic.synth_frames_device(0, N, H, W, 3, dtype=torch.uint8)
    a = icn.score(xi, measure="margin")
    b, _ = icn.score_regions(xi, region=128, measure="margin")
    assert torch.equal(a, b)
    irows = timed_interleaved({"icnet/score": lambda: icn.score(xi, measure="margin"),
                               "icnet/regions/128": lambda: icn.score_regions(xi, region=128, measure="margin")},
                              max(1, args.steps // 2), args.repeats)
    for key, r in irows.items():
        r["vs_icnet_score"] = r["median"] / irows["icnet/score"]["median"]
    rows.update(irows)

    for key, r in rows.items():
        rel = r.get("vs_score", r.get("vs_icnet_score"))
        print("%-22s %8.1f images/s  (min %.1f max %.1f)  %.4f x its plain pass" % (key, r["median"], r["min"], r["max"], rel))
    print("regions/128 within the spread of score: %s" % rec["regions_128_within_score_spread"])
    for name, k in kern.items():
        print(name, json.dumps(k))
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
