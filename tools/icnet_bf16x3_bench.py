"""ICNet's ranking pass in exact fp32 against the opt-in bf16x3 mode on one MI355X: ICNet(19), batch 8 x 1024 x 2048 uint8
frames, margin, one process, HIP-event timing.

  pass      INTERLEAVED windows (exact, bf16x3, exact, ...: --repeats rounds of --steps batches per window): images/s as median
            with min and max, and the paired ratio bf16x3 / exact per round with its spread
  classes   every distinct (kernel, NT, layer shape) class the mode moves to k_igemm_bf16x3, timed exact against split in the same
            run: the layer's convolution through the per-operator hook (random data and weights of the layer's shape; the
            launcher and the kernels are the network's), milliseconds per launch from the library's launch profiler
  agreement over --frames batches of synthetic frames: do the k least confident ids agree (rank_lowest on the scores of both
            modes), and the share of pixels whose label differs.  Recorded, not gated.

    python tools/icnet_bf16x3_bench.py [--repeats 7] [--steps 10] [--out profiles/r25_icnet_bf16x3_bench.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from semanticsegmentationactivelearning_amd import _lib, models, synthetic  # noqa: E402
from semanticsegmentationactivelearning_amd.models.util import conv_ops as cops  # noqa: E402

N, H, W, K = 8, 1024, 2048, 19


def window(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return N * steps / (a.elapsed_time(b) / 1e3)


def summary(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "all": [float(r) for r in v]}


def per_launch(fn, launches=5):
    """{kernel: ms per launch} of the convolution kernels fn launches"""
    fn()
    torch.cuda.synchronize()
    _lib.profile_enable(True)
    for _ in range(launches):
        fn()
    torch.cuda.synchronize()
    prof = _lib.profile_collect()
    _lib.profile_enable(False)
    return {k: v["ms"] / v["launches"] for k, v in prof.items() if k.startswith("k_igemm")}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--frames", type=int, default=4, help="batches of 8 frames for the agreement record")
    ap.add_argument("--topk", type=int, default=8)
    ap.add_argument("--out", default=os.path.join("profiles", "r25_icnet_bf16x3_bench.json"))
    args = ap.parse_args()
    import icnet_split_model as ism  # the list of ICNet's convolutions (tests/)

    torch.cuda.set_device(0)
    net = models.ICNet(K)
    net.build((None, H, W, 3))
    synthetic.randomize_icnet(net, seed=0)
    x = synthetic.synth_frames_device(0, N, H, W, 3, dtype=torch.uint8)
    assert _lib.get_knobs()["defaults"], _lib.get_knobs()
    rec = {"shape": [N, H, W], "classes": K, "frames": "uint8", "measure": "margin", "steps": args.steps, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0), "knobs": _lib.get_knobs()}

    passes = {"exact": lambda: net.score(x, measure="margin"), "bf16x3": lambda: net.score(x, measure="margin", arithmetic="bf16x3")}
    for fn in passes.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    rates = {p: [] for p in passes}
    for _ in range(args.repeats):
        for p, fn in passes.items():
            rates[p].append(window(fn, args.steps))
    rec["pass_images_per_s"] = {p: summary(v) for p, v in rates.items()}
    rec["pass_bf16x3_over_exact_pairs"] = summary(np.asarray(rates["bf16x3"]) / np.asarray(rates["exact"]))
    rec["exact_pass_against_parent"] = "not yet measured"
    for p in passes:
        r = rec["pass_images_per_s"][p]
        print("%-8s %8.1f images/s  (min %.1f max %.1f)" % (p, r["median"], r["min"], r["max"]))
    r = rec["pass_bf16x3_over_exact_pairs"]
    print("bf16x3 / exact per round: median %.4f  (min %.4f max %.4f)" % (r["median"], r["min"], r["max"]))
    spread = (r["max"] - r["min"]) / r["median"]

    # ---- per class ----
    classes = {}
    for c in ism.icnet_convs():
        h, w = H // c["div"], W // c["div"]
        res = c["res"] is not None
        kern, nt = _lib.icnet_conv_dispatch(N, h, w, c["cin"], c["cout"], c["k"], c["stride"], c["dil"], c["up2"], res, "bf16x3")
        if kern != "k_igemm_bf16x3":
            continue
        key = "NT%d %dx%d c%d->%d k%d s%d d%d%s" % (nt, h, w, c["cin"], c["cout"], c["k"], c["stride"], c["dil"], " +res" if res else "")
        classes.setdefault(key, dict(c, h=h, w=w, nt=nt, layers=[]))["layers"].append(c["name"])
    rows = {}
    g = torch.Generator(device="cuda").manual_seed(1)
    for key, c in classes.items():
        xin = torch.randn((N, c["h"], c["w"], c["cin"]), device="cuda", generator=g)
        rng = np.random.default_rng(len(rows))
        kernel = (rng.normal(size=(c["k"], c["k"], c["cin"], c["cout"])) / np.sqrt(c["k"] ** 2 * c["cin"])).astype(np.float32)
        bias = rng.normal(size=c["cout"]).astype(np.float32)
        ho, wo = -(-c["h"] // c["stride"]), -(-c["w"] // c["stride"])
        r_ = torch.randn((N, ho, wo, c["cout"]), device="cuda", generator=g) if c["res"] else None
        ms = {}
        for mode in ("f32", "bf16x3"):
            t = per_launch(lambda: cops.conv_bn_act(xin, kernel, c["stride"], c["dil"], bias=bias, residual=r_, relu=c["relu"],
                                                    arithmetic=mode))
            assert len(t) == 1, t
            ms[mode] = {"kernel": list(t)[0], "ms_per_launch": list(t.values())[0]}
        ratio = ms["bf16x3"]["ms_per_launch"] / ms["f32"]["ms_per_launch"]
        rows[key] = {"layers": c["layers"], "exact": ms["f32"], "bf16x3": ms["bf16x3"], "split_over_exact": ratio,
                     "faster_beyond_window_spread": bool(ratio < 1.0 - spread)}
        print("%-44s x%-2d exact %8.4f ms  split %8.4f ms  ratio %.3f" % (key, len(c["layers"]), ms["f32"]["ms_per_launch"],
                                                                         ms["bf16x3"]["ms_per_launch"], ratio))
        del xin, r_
    rec["classes"] = rows
    rec["window_spread"] = spread

    # ---- agreement with the exact path ----
    se, sm, differ, pixels = [], [], 0, 0
    for b in range(args.frames):
        xb = synthetic.synth_frames_device(b * N, N, H, W, 3, dtype=torch.uint8)
        a, ea = net.score(xb, measure="margin", return_label=True)
        m, em = net.score(xb, measure="margin", return_label=True, arithmetic="bf16x3")
        se.append(a.cpu().numpy())
        sm.append(m.cpu().numpy())
        differ += int((ea["label"] != em["label"]).sum())
        pixels += ea["label"].numel()
    se, sm = np.concatenate(se), np.concatenate(sm)
    top_e, top_m = set(np.argsort(se, kind="stable")[:args.topk].tolist()), set(np.argsort(sm, kind="stable")[:args.topk].tolist())
    rec["agreement"] = {"frames": int(se.size), "topk": args.topk, "topk_ids_equal": top_e == top_m,
                        "max_score_difference": float(np.abs(se - sm).max()), "differing_label_share": differ / pixels}
    print("agreement:", json.dumps(rec["agreement"]))
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
