"""Cost of the semi-supervised training step of ICNet's high-resolution trainer on one MI355X:
ICNet(19), batch 8 x 1024 x 2048 uint8 frames, half of the batch unlabelled, HIP-event timing, everything in ONE process on ONE
box.

Rows (ms per batch; median and min / max over --repeats timed windows of --steps batches each, the rows timed in --repeats
interleaved rounds so that drift of the box hits every row alike):
  a_plain_step          ICNetHighResTrainer.step(images) on a fully annotated batch
  b_semi_step           the semi-supervised trainer's step with labelled / confusion / pseudo pixels (targets from the training
                        logits)
  c_semi_step_raw       the same with images_raw: the backbone, the branch and the head run twice, the target-only launch in
                        between; conv1_sub1 + conv2_sub1 of the undistorted frames as one launch (k_front2<s2>)
  d_composed            net(x_raw) -> al.score_logits(label, mask) -> al.training_targets -> the plain step
  e_composed_conf       (d) plus tensortools.metrics.confusion_mat on the argmax of net(x)
  c2_semi_step_raw_unfused  (c) with bit 0 of the knob "ic_front" cleared: the raw side through the two separate launches
The per-kernel milliseconds come from the library's launch profiler in a separate pass.  Writes the record to --out.

    python tools/train_icnet_highres_semi_bench.py [--repeats 5] [--steps 10] [--out profiles/r26_train_icnet_highres_semi_bench.json]
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
from semanticsegmentationactivelearning_amd.training import ICNetHighResTrainer, SemiSupervisedICNetHighResTrainer  # noqa: E402

N, H, W, K = 8, 1024, 2048, 19
MEASURE = "entropy"
KERNELS = ("k_front2<s2>", "k_conv_first", "k_icnet_head_grad_hw", "k_icnet_head_grad_semi_hw", "k_icnet_head_targets",
           "k_confusion_fold")


def window(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def twin(net0):
    net = models.ICNet(K)
    net.build((None, None, None, 3))
    net.assign_named({v.name: v.numpy() for v in net0.variables})
    return net


def bench(net0, x, x_raw, labels, mask, sel, threshold, args):
    hyper = dict(learning_rate=5e-4, beta1=0.9, beta2=0.99, l2=2e-4, loginverse_scaling=1.02)
    nets = {name: twin(net0) for name in "abcdef"}
    tr = {name: (ICNetHighResTrainer if name in "ade" else SemiSupervisedICNetHighResTrainer)(nets[name], **hyper)
          for name in nets}
    for t in tr.values():
        t.reinitialize(seed=0)
    cm = {name: torch.zeros((K, K), dtype=torch.int64, device=x.device) for name in "bcef"}
    shipped = _lib.get_knobs()["ic_front"]

    def composed(name, with_confusion):
        net, t = nets[name], tr[name]
        _, p = al.score_logits(net(x_raw, training=False), MEASURE, threshold, return_label=True, return_mask=True)
        lab, mk = al.training_targets(sel, labels, mask, p["label"], p["mask"].float())
        if with_confusion:
            _, pt = al.score_logits(net(x, training=False), "confidence", 0.0, return_label=True)
            metrics.confusion_mat(lab, pt["label"], K, weights=mk, out=cm[name])
        return t.step(x, lab, mk)

    def semi_raw(name):
        return tr[name].step(x, labels, mask, labelled=sel, measure=MEASURE, threshold=threshold, images_raw=x_raw,
                             confusion=cm[name], return_pseudo_pixels=True)

    def unfused():
        _lib.set_knob("ic_front", shipped & ~1)
        try:
            return semi_raw("f")
        finally:
            _lib.set_knob("ic_front", shipped)

    rows = {
        "a_plain_step": lambda: tr["a"].step(x, labels, mask),
        "b_semi_step": lambda: tr["b"].step(x, labels, mask, labelled=sel, measure=MEASURE, threshold=threshold,
                                            confusion=cm["b"], return_pseudo_pixels=True),
        "c_semi_step_raw": lambda: semi_raw("c"),
        "d_composed": lambda: composed("d", False),
        "e_composed_conf": lambda: composed("e", True),
        "c2_semi_step_raw_unfused": unfused,
    }
    for fn in rows.values():  # warm-up: workspaces, handle pushes, code objects
        fn()
        fn()
    torch.cuda.synchronize()
    runs = {k: [] for k in rows}
    for _ in range(args.repeats):
        for name, fn in rows.items():
            runs[name].append(window(fn, args.steps))
    out = {"rows_ms_per_batch": {}}
    for name, v in runs.items():
        out["rows_ms_per_batch"][name] = {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)),
                                          "repeats": v}
        print("%-26s median %8.3f ms  [%8.3f, %8.3f]" % (name, np.median(v), min(v), max(v)), flush=True)
    r = out["rows_ms_per_batch"]
    c, d, c2 = r["c_semi_step_raw"], r["d_composed"], r["c2_semi_step_raw_unfused"]
    out["fused_below_composed"] = {"median": c["median"] < d["median"], "spreads_apart": c["max"] < d["min"]}
    out["fused_front_below_unfused"] = {"median": c["median"] < c2["median"], "spreads_apart": c["max"] < c2["min"]}
    print("fused (c) below composed (d): median %s, spreads apart %s" % (c["median"] < d["median"], c["max"] < d["min"]))
    print("fused front (c) below the separate launches (c2): median %s, spreads apart %s"
          % (c["median"] < c2["median"], c["max"] < c2["min"]))
    # the trained variables of (c), (c2) and (e) have taken the same steps on the same targets
    names = ICNetHighResTrainer.variable_names
    var = lambda net, name: getattr(getattr(net, name.split(".")[0]), name.split(".")[1]).numpy()
    for other, key in (("e", "fused_weights_equal_composed_weights"), ("f", "fused_front_weights_equal_unfused_weights")):
        same = all(np.array_equal(var(nets["c"], n), var(nets[other], n)) for n in names)
        out[key] = bool(same and torch.equal(cm["c"], cm[other]))
        print("%s: %s" % (key, out[key]))
    out["kernels_3_steps"] = {}
    for name in ("a_plain_step", "b_semi_step", "c_semi_step_raw", "c2_semi_step_raw_unfused"):
        _lib.profile_enable(True)
        for _ in range(3):
            rows[name]()
        torch.cuda.synchronize()
        prof = _lib.profile_collect()
        _lib.profile_enable(False)
        out["kernels_3_steps"][name] = prof
        for kname in KERNELS:
            if kname in prof:
                p = prof[kname]
                print("%-26s %-26s %.3f ms / launch (%d launches)" % (name, kname, p["ms"] / p["launches"], p["launches"]),
                      flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default="profiles/r26_train_icnet_highres_semi_bench.json")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    net0 = models.ICNet(K)
    net0.build((None, None, None, 3))
    synthetic.randomize_icnet(net0, seed=0)
    x_raw = synthetic.synth_frames_device(0, N, H, W, 3, dtype=torch.uint8)
    x = x_raw.flip(-1).contiguous()  # the distorted frames: the channels reversed
    _, extra = net0.score(x_raw, MEASURE, 0.0, return_label=True, return_confidence=True)
    labels = extra["label"].clone()
    mask = torch.ones((N, H, W), dtype=torch.float32, device=x.device)
    threshold = float(extra["confidence"].flatten()[::1009].float().median())  # about half of the pixels pass
    del extra
    sel = torch.tensor([i % 2 == 0 for i in range(N)], device=x.device)  # half of the batch unlabelled
    out = {"batch": [N, H, W, K], "frames": "uint8", "measure": MEASURE, "threshold": threshold,
           "labelled": [bool(v) for v in sel.tolist()], "steps_per_window": args.steps}
    out.update(bench(net0, x, x_raw, labels, mask, sel, threshold, args))
    out["knobs"] = _lib.get_knobs()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
