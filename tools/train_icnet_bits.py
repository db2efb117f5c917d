#!/usr/bin/env python
"""What a refactor of ICNet's four trainers must leave unchanged, recorded from fixed seeded inputs (DESIGN.md sections 33 and
38) in three parts:

``sha256``: SHA-256 of the raw bytes of every result.  ``gradient_features`` of ``ICNetHeadTrainer``, ``ICNetFusionTrainer``,
``ICNetCascadeTrainer`` and ``ICNetHighResTrainer`` (fp32 and uint8 frame, 3 and 4 input channels) on the inputs of the tests'
own case generators, at the shapes (1, 1, 1), (2, 2, 3) and (1, 3, 5) (each trainer's own unit, as in its test), max_workgroups
1 and 2, (K, weight, smoothing) = (2, 0, 0) and (19, 1.02, 0.1): the loss and every gradient.  At the same cases, per depth:
one ``step`` from images (the loss and every trained variable after it), and the semi-supervised ``gradient_features`` and
``step`` on a mixed ``labelled`` vector without a raw side and with one (the loss, the gradients or variables, ``confusion``
and the pseudo-pixel counts).  The file holds one digest per call, of the digests of the call's results under their names.

``workspace_bytes``: every ``ssal_icnet_*_workspace_bytes`` query at those shapes, as integers.  (An images entry, here and in
the steps above, gets frames of 32 h x 32 w whatever the depth: the trunk's own unit.)

``refused``: per ``ssal_icnet_*_nhwc`` training entry, a fixed list of calls it refuses, one for each step of its order of
judgement, straight through the C ABI on dummy device pointers (nothing is launched): (return code, ``ssal_last_error``).  An
images entry takes its class count from the handle and judges the frame's size before the depth's limit can be reached, so
"classes out of range" and "feature map beyond the limit" are recorded for the features entries only.

The four depths without semi-supervised entries, ``ICNetPyramidTrainer``, ``ICNetPoolingTrainer``,
``ICNetBottleneckTrainer`` and ``ICNetDeepBottleneckTrainer`` (DESIGN.md sections 39, 41, 42 and 43), are recorded in their plain parts: ``gradient_features``, one ``step``, the two plain size queries, the plain entries'
refusals.  A depth whose trainer the package under test does not have is left out of the file.

    python tools/train_icnet_bits.py --out profiles/r30_train_icnet_bits.json
    SSAL_LIB_PATH=/path/to/another/libssal_hip.so python tools/train_icnet_bits.py --out other.json
    python tools/train_icnet_bits.py --compare other.json profiles/r30_train_icnet_bits.json
    python tools/train_icnet_bits.py --compare other.json profiles/r30_train_icnet_bits.json --depths head,fusion,cascade,highres,pyramid,pool,bneck

``--depths`` restricts a comparison to the entries of those depths: a file written by this tool from an earlier tree (copy the
tool next to that tree's package) has no entry of a depth that tree lacks.

Run each library in a fresh process: the package loads one library per process.  ``--compare`` counts an entry that only one
file has as differing, unless the files are of different formats (``profiles/r25_train_icnet_bits.json`` is of the first, which
held the three deep trainers' plain gradients only, one digest per result): then that file's digests are folded per call in the
same way and the entries both have are compared.
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FORMAT = 2
SECTIONS = ("sha256", "workspace_bytes", "refused")
SHAPES = [(1, 1, 1), (2, 2, 3), (1, 3, 5)]
CASES = [(s, mw, k, wl) for s in SHAPES for mw in (1, 2) for k, wl in ((2, (0.0, 0.0)), (19, (1.02, 0.1)))]
DEPTHS = ("head", "fusion", "cascade", "highres")
PLAIN_DEPTHS = ("pyramid", "pool", "bneck", "bneck2")  # no semi-supervised entries yet
# feature pointers of the features entry (highres: the frame last)
FEATS = {"head": 1, "fusion": 2, "cascade": 3, "highres": 3, "pyramid": 3, "pool": 4, "bneck": 3, "bneck2": 3}
PLAIN_TRAINERS = {"pyramid": "ICNetPyramidTrainer", "pool": "ICNetPoolingTrainer", "bneck": "ICNetBottleneckTrainer",
                  "bneck2": "ICNetDeepBottleneckTrainer"}


def plain_depths():
    """the members of PLAIN_DEPTHS the package under test has"""
    from semanticsegmentationactivelearning_amd import training as T
    return tuple(d for d in PLAIN_DEPTHS if hasattr(T, PLAIN_TRAINERS[d]))


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _record(out, tag, loss, gd):
    out[tag + " loss"] = _sha(loss)
    for name in sorted(gd):
        out["%s %s" % (tag, name)] = _sha(gd[name])


def fold(entries):
    """{"<call> <result>": digest} -> {"<call>": one digest of the call's (result, digest) pairs in name order}: what a file of
    format 2 holds, one line per call (a result's name has no blank in it)"""
    calls = {}
    for key in sorted(entries):
        call, result = key.rsplit(" ", 1)
        calls.setdefault(call, hashlib.sha256()).update(("%s=%s\n" % (result, entries[key])).encode())
    return {call: h.hexdigest() for call, h in calls.items()}


def _trainers():
    from semanticsegmentationactivelearning_amd import training as T
    return {"head": (T.ICNetHeadTrainer, T.SemiSupervisedICNetHeadTrainer),
            "fusion": (T.ICNetFusionTrainer, T.SemiSupervisedICNetFusionTrainer),
            "cascade": (T.ICNetCascadeTrainer, T.SemiSupervisedICNetCascadeTrainer),
            "highres": (T.ICNetHighResTrainer, T.SemiSupervisedICNetHighResTrainer)}


def _semi_records(out, tag, semi_tr, feats, raw_feats, labels, mask, d, mw, k, head):
    """the semi-supervised ``gradient_features`` on a mixed ``labelled`` vector (odd images labelled), without and with a raw
    side (the head's raw side is one tensor, the others' the whole tuple)"""
    import torch
    n = feats[0].shape[0]
    labelled = torch.as_tensor([i % 2 for i in range(n)], dtype=torch.uint8)
    for kind, raw in (("noraw", None), ("raw", raw_feats[0] if head else tuple(raw_feats))):
        conf = torch.zeros((k, k), dtype=torch.int64, device="cuda")
        loss, gd, pp = semi_tr.gradient_features(*feats, labels, mask, params=d, max_workgroups=mw, labelled=labelled,
                                                 features_raw=raw, confusion=conf, return_pseudo_pixels=True)
        _record(out, "%s semi %s" % (tag, kind), loss, gd)
        out["%s semi %s confusion" % (tag, kind)] = _sha(conf)
        out["%s semi %s pseudo_pixels" % (tag, kind)] = _sha(pp)


def _step_records(out, tag, classes, net, seed, n, h, w, k, mw, kw, u8):
    """one ``step`` from images of the plain trainer, then of the semi-supervised one without and with ``images_raw``; the
    model's weights are drawn again before each"""
    import numpy as np
    import torch

    from semanticsegmentationactivelearning_amd import synthetic as syn
    rng = np.random.default_rng(seed)
    c_in = int(net._c_in)
    frames = [rng.integers(0, 256, (n, h, w, c_in), dtype=np.uint8) for _ in range(2)]
    x, x_raw = (torch.as_tensor(f if u8 else f.astype(np.float32) * np.float32(1.0 / 255.0)).cuda() for f in frames)
    labels = torch.as_tensor(rng.integers(0, k, (n, h, w)).astype(np.uint8)).cuda()
    mask = torch.as_tensor((rng.uniform(size=(n, h, w)) > 0.25).astype(np.float32)).cuda()
    labelled = torch.as_tensor([i % 2 for i in range(n)], dtype=torch.uint8)
    for kind, cls, raw in (("plain", classes[0], None), ("semi noraw", classes[1], None), ("semi raw", classes[1], x_raw)):
        if cls is None:
            continue  # a depth without semi-supervised entries
        syn.randomize_icnet(net, seed=5)
        tr = cls(net, 1e-3, measure="entropy", threshold=0.8 * float(np.log(k)), **kw)
        if kind == "plain":
            loss = tr.step(x, labels, mask, max_workgroups=mw)
        else:
            conf = torch.zeros((k, k), dtype=torch.int64, device="cuda")
            loss, pp = tr.step(x, labels, mask, max_workgroups=mw, labelled=labelled, images_raw=raw, confusion=conf,
                               return_pseudo_pixels=True)
            out["%s step %s confusion" % (tag, kind)] = _sha(conf)
            out["%s step %s pseudo_pixels" % (tag, kind)] = _sha(pp)
        _record(out, "%s step %s" % (tag, kind), loss,
                {name: torch.as_tensor(np.asarray(v.numpy())) for name, v in zip(tr.variable_names, tr._vars())})


def digests():
    import numpy as np
    import torch

    import test_gpu_train_icnet_cascade as tc   # the tests' case generators and their models' seeded moving statistics
    import test_gpu_train_icnet_fusion as tf
    import test_gpu_train_icnet_head as thd
    import test_gpu_train_icnet_highres as th

    torch.cuda.set_device(0)
    dev = lambda *arrays: [torch.as_tensor(a).cuda() for a in arrays]
    T = _trainers()
    out = {}
    for i, ((n, h, w), mw, k, (weight, ls)) in enumerate(CASES):
        tag = "%dx%dx%d mw=%d K=%d w=%g ls=%g" % (n, h, w, mw, k, weight, ls)
        kw = dict(loginverse_scaling=weight, label_smoothing=ls)
        semi_kw = dict(kw, measure="entropy", threshold=0.8 * float(np.log(k)))

        x, head, labels, mask = thd._case(8900 + i, n, h, w, k)
        net = thd._shared_net(k)
        _record(out, "head " + tag, *T["head"][0](net, 1e-3, **kw).gradient_features(
            *dev(x), labels, mask, params=thd._params(head, k), max_workgroups=mw))
        _semi_records(out, "head " + tag, T["head"][1](net, 1e-3, **semi_kw), dev(x), dev(thd._case(8950 + i, n, h, w, k)[0]),
                      labels, mask, thd._params(head, k), mw, k, True)

        s24, c3, d, labels, mask = tf._case(9000 + i, n, h, w, k)
        net = tf._shared_net(k)
        _record(out, "fusion " + tag, *T["fusion"][0](net, 1e-3, **kw).gradient_features(
            *dev(s24, c3), labels, mask, params=d, max_workgroups=mw))
        _semi_records(out, "fusion " + tag, T["fusion"][1](net, 1e-3, **semi_kw), dev(s24, c3),
                      dev(*tf._case(9050 + i, n, h, w, k)[:2]), labels, mask, d, mw, k, False)

        c54, c31, c3, d, labels, mask = tc._case(9100 + i, n, h, w, k)
        net = tc._shared_net(k)
        _record(out, "cascade " + tag, *T["cascade"][0](net, 1e-3, **kw).gradient_features(
            *dev(c54, c31, c3), labels, mask, params=d, max_workgroups=mw))
        _semi_records(out, "cascade " + tag, T["cascade"][1](net, 1e-3, **semi_kw), dev(c54, c31, c3),
                      dev(*tc._case(9150 + i, n, h, w, k)[:3]), labels, mask, d, mw, k, False)

        for c_in in (3, 4):
            c54, c31, u8, d, stats, labels, mask = th._case(9200 + i, n, h, w, k, c_in=c_in)
            r54, r31, r8 = th._case(9250 + i, n, h, w, k, c_in=c_in)[:3]
            net = th._shared_net(k, c_in)
            th._set_stats(net, stats)
            tr = T["highres"][0](net, 1e-3, **kw)
            for kind, frame, raw in (("fp32", th._unit(u8), th._unit(r8)), ("uint8", u8, r8)):
                htag = "highres c_in=%d %s %s" % (c_in, kind, tag)
                _record(out, htag, *tr.gradient_features(*dev(c54, c31, frame), labels, mask, params=d, max_workgroups=mw))
                _semi_records(out, htag, T["highres"][1](net, 1e-3, **semi_kw), dev(c54, c31, frame), dev(r54, r31, raw),
                              labels, mask, d, mw, k, False)

        plain = plain_depths()
        if "pyramid" in plain:
            import test_gpu_train_icnet_pyramid as tp
            import icnet_pyramid_train_oracle as ipo
            c53, c31, c3, d, labels, mask = ipo.case(9400 + i, n, h, w, k)
            T["pyramid"] = (getattr(_training(), PLAIN_TRAINERS["pyramid"]), None)
            _record(out, "pyramid " + tag, *T["pyramid"][0](tp._shared_net(k), 1e-3, **kw).gradient_features(
                *dev(c53, c31, c3), labels, mask, params=d, max_workgroups=mw))
        if "pool" in plain:
            import test_gpu_train_icnet_pool as tq
            import icnet_pool_train_oracle as po
            a33, c52, c31, c3, d, labels, mask = po.case(9500 + i, n, h, w, k)
            T["pool"] = (getattr(_training(), PLAIN_TRAINERS["pool"]), None)
            _record(out, "pool " + tag, *T["pool"][0](tq._shared_net(k), 1e-3, **kw).gradient_features(
                *dev(a33, c52, c31, c3), labels, mask, params=d, max_workgroups=mw))
        if "bneck" in plain:
            import test_gpu_train_icnet_bneck as tb
            import icnet_bneck_train_oracle as bo
            c52, c31, c3, d, labels, mask = bo.case(9600 + i, n, h, w, k)
            T["bneck"] = (getattr(_training(), PLAIN_TRAINERS["bneck"]), None)
            _record(out, "bneck " + tag, *T["bneck"][0](tb._shared_net(k), 1e-3, **kw).gradient_features(
                *dev(c52, c31, c3), labels, mask, params=d, max_workgroups=mw))
        if "bneck2" in plain:
            import test_gpu_train_icnet_bneck2 as t2
            import icnet_bneck2_train_oracle as b2
            c51, c31, c3, d, labels, mask = b2.case(9700 + i, n, h, w, k)
            T["bneck2"] = (getattr(_training(), PLAIN_TRAINERS["bneck2"]), None)
            _record(out, "bneck2 " + tag, *T["bneck2"][0](t2._shared_net(k), 1e-3, **kw).gradient_features(
                *dev(c51, c31, c3), labels, mask, params=d, max_workgroups=mw))

        # the images entries, on models of their own (a step writes the trained variables back); frames of 32 h x 32 w for
        # every depth, the trunk's own unit
        for depth in DEPTHS + plain:
            for c_in in ((3, 4) if depth == "highres" else (3,)):
                net = _step_net(k, c_in)
                _step_records(out, "%s c_in=%d %s" % (depth, c_in, tag), T[depth], net, 9300 + i, n, 32 * h, 32 * w, k, mw, kw,
                              c_in == 3)
    torch.cuda.synchronize()
    return out


def _training():
    from semanticsegmentationactivelearning_amd import training
    return training


_STEP_NETS = {}


def _step_net(k, c_in):
    import semanticsegmentationactivelearning_amd as ssal
    if (k, c_in) not in _STEP_NETS:
        net = ssal.ICNet(k)
        net.build((None, None, None, c_in))
        _STEP_NETS[(k, c_in)] = net
    return _STEP_NETS[(k, c_in)]


def workspace_bytes():
    """every training workspace query at SHAPES, K = 2 and 19, c_in = 3"""
    from semanticsegmentationactivelearning_amd import _lib, synthetic as syn
    L = _lib.lib()
    out = {}
    for k in (2, 19):
        net = _step_net(k, 3)
        syn.randomize_icnet(net, seed=5)
        handle = net._sync_handle()
        for depth in DEPTHS + plain_depths():
            for n, h, w in SHAPES:
                tag = "%dx%dx%d K=%d" % (n, h, w, k)
                out["ssal_icnet_%s_grad_workspace_bytes %s" % (depth, tag)] = int(
                    getattr(L, "ssal_icnet_%s_grad_workspace_bytes" % depth)(n, h, w, k))
                out["ssal_icnet_train_%s_workspace_bytes %s" % (depth, tag)] = int(
                    getattr(L, "ssal_icnet_train_%s_workspace_bytes" % depth)(handle, n, 32 * h, 32 * w))
                for raw in (0, 1) if depth in DEPTHS else ():
                    out["ssal_icnet_%s_grad_semi_workspace_bytes %s raw=%d" % (depth, tag, raw)] = int(
                        getattr(L, "ssal_icnet_%s_grad_semi_workspace_bytes" % depth)(n, h, w, k, raw))
                    out["ssal_icnet_train_%s_semi_workspace_bytes %s raw=%d" % (depth, tag, raw)] = int(
                        getattr(L, "ssal_icnet_train_%s_semi_workspace_bytes" % depth)(handle, n, 32 * h, 32 * w, raw))
    return out


def _entry_args(depth, images, semi, handle, P, n, h, w, k):
    """[(name, value)] of one valid call of an entry, in the entry's order; P: the dummy device pointer every pointer gets"""
    stats = [] if depth == "head" else [("stats", P)]
    frame = [("x_is_u8", 0), ("c_in", 3)] if depth == "highres" and not images else []
    semi_rule = [("labelled", P), ("measure", 0), ("threshold", 0.5)] if semi else []
    semi_out = [("confusion", P), ("pseudo_pixels", P)] if semi else []
    tail = [("max_workgroups", 0), ("loss", P), ("grad", P)] + semi_out + [("ws", P), ("ws_bytes", 0), ("stream", None)]
    knobs = [("weight", 0.0), ("label_smoothing", 0.0)] + stats + frame
    if images:
        head = [("net", handle), ("x", P)] + ([("x_raw", P)] if semi else []) + [("x_is_u8", 1), ("n", n), ("h", h), ("w", w)]
        return head + [("labels", P), ("mask", P)] + semi_rule + [("params", P)] + knobs + tail
    feats = [("%s%d" % (side, i), P) for side in (("f", "raw") if semi else ("f",)) for i in range(FEATS[depth])]
    dims = [("n", n), ("h", h), ("w", w), ("classes", k)]
    return feats + dims + [("params", P), ("labels", P), ("mask", P)] + semi_rule + knobs + tail


def refused():
    """(return code, message) of the calls each training entry refuses, in the order it judges them"""
    import torch

    from semanticsegmentationactivelearning_amd import _lib, synthetic as syn
    L = _lib.lib()
    k, (n, h, w) = 19, SHAPES[1]
    net = _step_net(k, 3)
    syn.randomize_icnet(net, seed=5)
    handle = net._sync_handle()
    dummy = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    P = _lib.dev_ptr(dummy)
    beyond = {"head": (1 << 27) + 1, "fusion": (1 << 26) + 1, "cascade": (1 << 25) + 1, "highres": 512,
              "pyramid": (1 << 25) + 1, "pool": (1 << 25) + 1, "bneck": (1 << 25) + 1, "bneck2": (1 << 25) + 1}
    out = {}
    for depth in DEPTHS + plain_depths():
        for images in (False, True):
            for semi in (False, True) if depth in DEPTHS else (False,):
                stem = ("ssal_icnet_train_%s" if images else "ssal_icnet_%s_grad") % depth + ("_semi" if semi else "")
                dims = (n, 32 * h, 32 * w) if images else (n, h, w)
                query = (handle,) + dims if images else dims + (k,)
                need = int(getattr(L, stem + "_workspace_bytes")(*(query + ((1,) if semi else ()))))
                base = dict(_entry_args(depth, images, semi, handle, P, *dims, k), ws_bytes=need)
                order = [name for name, _ in _entry_args(depth, images, semi, handle, P, *dims, k)]
                # (every case must be one the entry refuses, at its workspace check at the latest: the pointers are dummies.
                # A semi entry takes NULL labels when labelled_dev is given, so that case is the plain entries' only.)
                cases = [("bad dims", {"n": 0}), ("negative max_workgroups", {"max_workgroups": -1}),
                         ("NULL loss", {"loss": None}), ("NULL params", {"params": None}),
                         ("workspace one byte short", {"ws_bytes": need - 1})]
                if not semi:
                    cases += [("NULL labels", {"labels": None})]
                if images:
                    cases += [("NULL net", {"net": None}), ("height not a multiple of 32", {"h": 32 * h + 8})]
                else:
                    cases += [("classes out of range", {"classes": 33}), ("classes below range", {"classes": 1}),
                              ("feature map beyond the limit", {"h": beyond[depth], "w": 512 if depth == "highres" else w}),
                              ("NULL features", {"f0": None})]
                    if depth == "highres":
                        cases += [("five input channels", {"c_in": 5})]
                if semi:
                    cases += [("bad measure", {"measure": 3}), ("NULL labels, all labelled", {"labels": None, "labelled": None})]
                    if not images and FEATS[depth] > 1:
                        cases += [("raw pointers given in part", {"raw1": None})]
                for name, change in cases:
                    args = dict(base, **change)
                    rc = int(getattr(L, stem + "_nhwc")(*[args[a] for a in order]))
                    out["%s_nhwc: %s" % (stem, name)] = [rc, L.ssal_last_error().decode("utf-8", "replace") if rc else ""]
    torch.cuda.synchronize()
    return out


def depth_of(key):
    """the depth an entry of any section belongs to"""
    import re
    m = re.match(r"ssal_icnet_(?:train_)?([a-z0-9]+?)_(?:grad|semi|workspace|nhwc)", key)
    return m.group(1) if m else key.split(" ", 1)[0]


def compare(path_a, path_b, depths=None):
    a, b = (json.load(open(p)) for p in (path_a, path_b))
    if depths is not None:
        for f in (a, b):
            for section in SECTIONS:
                f[section] = {k: v for k, v in f.get(section, {}).items() if depth_of(k) in depths}
        print("(entries of the depths %s only)" % ", ".join(depths))
    same_format = a.get("format", 1) == b.get("format", 1)
    total, alone, bad = 0, 0, []
    for section in SECTIONS:
        sa, sb = (f.get(section, {}) for f in (a, b))
        if section == "sha256" and not same_format:  # the file of per-result digests is folded per call like the other
            sa, sb = (fold(s) if f.get("format", 1) == 1 else s for s, f in ((sa, a), (sb, b)))
        keys = set(sa) | set(sb) if same_format else set(sa) & set(sb)
        alone += len(set(sa) ^ set(sb))
        total += len(keys)
        bad += sorted("%s: %s" % (section, k) for k in keys if sa.get(k) != sb.get(k))
    for k in bad:
        print("DIFFERS:", k)
    if not same_format:
        print("(files of different formats: %d entries that only one of them has are not compared)" % alone)
    print("%d entries compared, %d differ" % (total, len(bad)))
    return 1 if bad or not total else 0


def main(default_out=os.path.join(ROOT, "profiles", "r29_train_icnet_bits.json"), parts=None, cases=len(CASES)):
    """``parts``: the (digests, workspace_bytes, refused) functions of a sibling tool (tools/train_enet_bits.py) and ``cases`` its
    case count, else this file's"""
    digests, workspace_bytes, refused = parts or (globals()[name] for name in ("digests", "workspace_bytes", "refused"))
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=default_out)
    ap.add_argument("--results", metavar="JSON", help="also write every result's own digest (a file of format 1, large): two "
                    "such files compare result by result, which names the tensor where a call's digest differs")
    ap.add_argument("--compare", nargs=2, metavar="JSON", help="compare two result files instead of running")
    ap.add_argument("--depths", help="with --compare: a comma-separated list of depths, the only ones compared")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare, depths=a.depths.split(",") if a.depths else None))
    results = digests()
    out = {"sha256": fold(results), "workspace_bytes": workspace_bytes(), "refused": refused()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.results:
        with open(a.results, "w") as f:
            json.dump({"format": 1, "sha256": results}, f, indent=1, sort_keys=True)
    with open(a.out, "w") as f:
        json.dump(dict(out, format=FORMAT, cases=cases, results=len(results)), f, indent=1, sort_keys=True)
    print("wrote %s: %s" % (a.out, ", ".join("%d %s" % (len(out[s]), s) for s in SECTIONS)))


if __name__ == "__main__":
    main()
