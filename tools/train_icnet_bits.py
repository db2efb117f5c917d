#!/usr/bin/env python
"""SHA-256 of the raw bytes of the loss and of every gradient tensor of ICNet's three deep trainers on fixed seeded inputs
(DESIGN.md section 33): what a refactor of their kernels must leave unchanged, bit for bit.  ``gradient_features`` of
``ICNetFusionTrainer``, ``ICNetCascadeTrainer`` and ``ICNetHighResTrainer`` (fp32 and uint8 frame, 3 and 4 input channels) on
the inputs of the tests' own case generators, at the shapes (1, 1, 1), (2, 2, 3) and (1, 3, 5) (each trainer's own unit, as in
its test), max_workgroups 1 and 2, (K, weight, smoothing) = (2, 0, 0) and (19, 1.02, 0.1).

    python tools/train_icnet_bits.py --out profiles/r25_train_icnet_bits.json
    SSAL_LIB_PATH=/path/to/another/libssal_hip.so python tools/train_icnet_bits.py --out other.json
    python tools/train_icnet_bits.py --compare other.json profiles/r25_train_icnet_bits.json

Run each library in a fresh process: the package loads one library per process.
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(1, 1, 1), (2, 2, 3), (1, 3, 5)]
CASES = [(s, mw, k, wl) for s in SHAPES for mw in (1, 2) for k, wl in ((2, (0.0, 0.0)), (19, (1.02, 0.1)))]


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _record(out, tag, loss, gd):
    out[tag + " loss"] = _sha(loss)
    for name in sorted(gd):
        out["%s %s" % (tag, name)] = _sha(gd[name])


def digests():
    import torch

    import test_gpu_train_icnet_cascade as tc   # the tests' case generators and their models' seeded moving statistics
    import test_gpu_train_icnet_fusion as tf
    import test_gpu_train_icnet_highres as th
    from semanticsegmentationactivelearning_amd.training import ICNetCascadeTrainer, ICNetFusionTrainer, ICNetHighResTrainer

    torch.cuda.set_device(0)
    dev = lambda *arrays: [torch.as_tensor(a).cuda() for a in arrays]
    out = {}
    for i, ((n, h, w), mw, k, (weight, ls)) in enumerate(CASES):
        tag = "%dx%dx%d mw=%d K=%d w=%g ls=%g" % (n, h, w, mw, k, weight, ls)
        kw = dict(loginverse_scaling=weight, label_smoothing=ls)

        s24, c3, d, labels, mask = tf._case(9000 + i, n, h, w, k)
        tr = ICNetFusionTrainer(tf._shared_net(k), 1e-3, **kw)
        _record(out, "fusion " + tag, *tr.gradient_features(*dev(s24, c3), labels, mask, params=d, max_workgroups=mw))

        c54, c31, c3, d, labels, mask = tc._case(9100 + i, n, h, w, k)
        tr = ICNetCascadeTrainer(tc._shared_net(k), 1e-3, **kw)
        _record(out, "cascade " + tag, *tr.gradient_features(*dev(c54, c31, c3), labels, mask, params=d, max_workgroups=mw))

        for c_in in (3, 4):
            c54, c31, u8, d, stats, labels, mask = th._case(9200 + i, n, h, w, k, c_in=c_in)
            net = th._shared_net(k, c_in)
            th._set_stats(net, stats)
            tr = ICNetHighResTrainer(net, 1e-3, **kw)
            for kind, frame in (("fp32", th._unit(u8)), ("uint8", u8)):
                _record(out, "highres c_in=%d %s %s" % (c_in, kind, tag),
                        *tr.gradient_features(*dev(c54, c31, frame), labels, mask, params=d, max_workgroups=mw))
    torch.cuda.synchronize()
    return out


def compare(path_a, path_b):
    a, b = (json.load(open(p))["sha256"] for p in (path_a, path_b))
    bad = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    for k in bad:
        print("DIFFERS:", k)
    print("%d digests compared, %d differ" % (len(set(a) | set(b)), len(bad)))
    return 1 if bad or not a else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_train_icnet_bits.json"))
    ap.add_argument("--compare", nargs=2, metavar="JSON", help="compare two result files instead of running")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    out = digests()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"cases": len(CASES), "digests": len(out), "sha256": out}, f, indent=1, sort_keys=True)
    print("wrote %s: %d digests" % (a.out, len(out)))


if __name__ == "__main__":
    main()
