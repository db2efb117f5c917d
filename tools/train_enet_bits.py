#!/usr/bin/env python
"""What a refactor of ENet's training entries must leave unchanged, recorded from fixed seeded inputs:
the sibling of tools/train_icnet_bits.py, whose digests, file format, ``--compare`` and ``--results`` it uses.  Six depths:
``FinalLayerTrainer`` (final), ``LastBlockTrainer`` (block), ``LastStageTrainer`` (stage), ``DecoderTailTrainer`` (tail),
``DeepTailTrainer`` (tail2) and ``DecoderTrainer`` (decoder), each with its semi-supervised class (the output layer's trainer
takes the semi-supervised keywords itself).  Three parts:

``sha256``: per depth, ``gradient_features`` on the inputs of its test's own case generator at the feature shapes (1, 1, 1),
(2, 2, 3) and (1, 3, 5), in the depth's own unit (no entry refuses one of them: a shape whose workspace query answers -1 would
be recorded as refused), ``max_workgroups`` 0, 1 and 2 where the entry takes it, (K, weight, smoothing) = (2, 0, 0) and
(19, 1.02, 0.1): the loss and every gradient; the semi-supervised ``gradient_features`` on a mixed ``labelled`` vector without
a raw side and with one: the loss, the gradients, ``confusion`` and the pseudo-pixel counts.  One ``step`` from images, of 2
frames of 16 x 24 (uint8) and of 8 x 8 (fp32), at the same knobs, plain and semi-supervised without and with ``images_raw``:
the loss, the packed weights and Adam's two slots after it, ``confusion`` and the pseudo-pixel counts.  A call that raises is
recorded with its message.

``workspace_bytes``: every ``*_workspace_bytes``, ``*_param_floats``, ``*_features_offset`` and ``*_code_offset`` query of the
section at those shapes and frames, as integers, with one refused shape each (-1).

``refused``: per ``*_nhwc`` training entry, one call for each step of its order of judgement, straight through the C ABI on a
dummy pointer: (return code, ``ssal_last_error``).  Every call carries a workspace size one byte short, so that none can reach
a launch whatever the entry thinks of the rest; the first verdict in the entry's order is what is recorded.  An images entry
takes its class count from the handle and judges the frame before the depth's limit can be reached, so "classes out of
range" and "feature map beyond the limit" are recorded for the features entries only.

    python tools/train_enet_bits.py --out profiles/r28_train_enet_bits.json
    SSAL_LIB_PATH=/path/to/another/libssal_hip.so python tools/train_enet_bits.py --out other.json
    python tools/train_enet_bits.py --compare other.json profiles/r28_train_enet_bits.json
    python tools/train_enet_bits.py --host --out host.json     # what needs no GPU: the features entries' sizes and refusals

Run each library in a fresh process: the package loads one library per process.
"""
import ctypes
import os
import sys

import train_icnet_bits as icb

ROOT = icb.ROOT
SHAPES = icb.SHAPES
FRAMES = [(2, 16, 24), (2, 8, 8)]
LOSSES = ((2, (0.0, 0.0)), (19, (1.02, 0.1)))
DEPTHS = ("final", "block", "stage", "tail", "tail2", "decoder")
# per depth: the C stems of its features / images entries, frame pixels per feature pixel, pooled-index inputs, whether the
# entries take max_workgroups, its test module (the case generator), its plain and semi-supervised trainer classes
SPEC = {
    "final": ("ssal_final_grad", "ssal_enet_train_final", 2, 0, False, "test_gpu_train_final",
              "FinalLayerTrainer", "FinalLayerTrainer"),
    "block": ("ssal_train_block_grad", "ssal_enet_train_block", 2, 0, False, "test_gpu_train_block",
              "LastBlockTrainer", "SemiSupervisedBlockTrainer"),
    "stage": ("ssal_train_stage_grad", "ssal_enet_train_stage", 4, 1, True, "test_gpu_train_stage",
              "LastStageTrainer", "SemiSupervisedStageTrainer"),
    "tail": ("ssal_train_tail_grad", "ssal_enet_train_tail", 4, 1, True, "test_gpu_train_tail",
             "DecoderTailTrainer", "SemiSupervisedTailTrainer"),
    "tail2": ("ssal_train_tail2_grad", "ssal_enet_train_tail2", 4, 1, True, "test_gpu_train_deep_tail",
              "DeepTailTrainer", "SemiSupervisedDeepTailTrainer"),
    "decoder": ("ssal_train_decoder_grad", "ssal_enet_train_decoder", 8, 2, True, "test_gpu_train_decoder",
                "DecoderTrainer", "SemiSupervisedDecoderTrainer"),
}
RAW_KEYS = {0: ("features_raw",), 1: ("features_raw", "argmax1_raw"), 2: ("features_raw", "argmax2_raw", "argmax1_raw")}
HOST_ONLY = False  # --host: no GPU, so no handle: the features entries' queries and refusals only


def _workgroups(depth):
    return (0, 1, 2) if SPEC[depth][4] else (0,)


def _cases(depth, shapes):
    return [(s, mw, k, wl) for s in shapes for mw in _workgroups(depth) for k, wl in LOSSES]


def _tag(shape, mw, k, wl):
    return "%dx%dx%d mw=%d K=%d w=%g ls=%g" % (shape + (mw, k) + wl)


def _call(out, tag, fn, names):
    """``fn()`` -> the results under ``names``; a call that raises is recorded with its message"""
    import torch
    try:
        res = fn()
    except (ValueError, RuntimeError, NotImplementedError, MemoryError) as e:
        out[tag + " raised"] = icb.hashlib.sha256(("%s: %s" % (type(e).__name__, e)).encode()).hexdigest()
        return
    for name, r in zip(names, res if isinstance(res, tuple) else (res,)):
        if isinstance(r, dict):
            for key in sorted(r):
                out["%s %s" % (tag, key)] = icb._sha(r[key])
        else:
            out["%s %s" % (tag, name)] = icb._sha(torch.as_tensor(r))


def _feature_records(out, depth, i, shape, mw, k, wl):
    """the plain ``gradient_features`` and the semi-supervised one without and with a raw side, on the test's own case"""
    import importlib

    import numpy as np
    import torch

    import semanticsegmentationactivelearning_amd as ssal
    from semanticsegmentationactivelearning_amd import training as T
    _, _, _, nam, takes_mw, module, plain, semi = SPEC[depth]
    t = importlib.import_module(module)
    n, h, w = shape
    dev = lambda arrays: tuple(torch.as_tensor(a).cuda() for a in arrays)
    case, raw_case = t._case(8000 + 100 * DEPTHS.index(depth) + i, n, h, w, k), t._case(8050 + 100 * DEPTHS.index(depth) + i, n, h, w, k)
    kw = dict(loginverse_scaling=wl[0], label_smoothing=wl[1], measure="entropy", threshold=0.8 * float(np.log(k)))
    if depth == "final":
        (x, kern, labels, mask), raw = case, dev(raw_case[:1])
        net = ssal.ENet(k)
        net.build((None, None, None, 3))
        call_kw = dict(kernel=kern)
    else:
        x, (labels, mask, params, stats), raw = case[:1 + nam], case[1 + nam:], dev(raw_case[:1 + nam])
        net = t._net_with(k, params, stats)
        call_kw = dict(max_workgroups=mw) if takes_mw else {}
    feats = dev(x if depth != "final" else (x,))
    tag = "%s %s" % (depth, _tag(shape, mw, k, wl))
    _call(out, tag, lambda: getattr(T, plain)(net, 1e-3, **kw).gradient_features(*feats, labels, mask, **call_kw),
          ("loss", "grad"))
    labelled = torch.as_tensor([j % 2 for j in range(n)], dtype=torch.uint8)
    for kind, raw_kw in (("noraw", {}), ("raw", dict(zip(RAW_KEYS[nam], raw)))):
        conf = torch.zeros((k, k), dtype=torch.int64, device="cuda")
        _call(out, "%s semi %s" % (tag, kind), lambda: getattr(T, semi)(net, 1e-3, **kw).gradient_features(
            *feats, labels, mask, labelled=labelled, confusion=conf, return_pseudo_pixels=True, **dict(call_kw, **raw_kw)),
            ("loss", "grad", "pseudo_pixels"))
        out["%s semi %s confusion" % (tag, kind)] = icb._sha(conf)


_STEP_NETS = {}


def _step_net(k):
    import semanticsegmentationactivelearning_amd as ssal
    if k not in _STEP_NETS:
        _STEP_NETS[k] = ssal.ENet(k)
        _STEP_NETS[k].build((None, None, None, 3))
    return _STEP_NETS[k]


def _step_records(out, depth, i, frame, mw, k, wl):
    """one ``step`` from images of the plain trainer, then of the semi-supervised one without and with ``images_raw``; the
    model's weights are drawn again before each"""
    import numpy as np
    import torch

    from semanticsegmentationactivelearning_amd import synthetic as syn, training as T
    n, h, w = frame
    rng = np.random.default_rng(8700 + i)
    frames = [rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8) for _ in range(2)]
    u8 = h > 8
    x, x_raw = (torch.as_tensor(f if u8 else f.astype(np.float32) * np.float32(1.0 / 255.0)).cuda() for f in frames)
    labels = torch.as_tensor(rng.integers(0, k, (n, h, w)).astype(np.uint8)).cuda()
    mask = torch.as_tensor((rng.uniform(size=(n, h, w)) > 0.25).astype(np.float32)).cuda()
    labelled = torch.as_tensor([j % 2 for j in range(n)], dtype=torch.uint8)
    kw = dict(loginverse_scaling=wl[0], label_smoothing=wl[1], measure="entropy", threshold=0.8 * float(np.log(k)))
    call_kw = dict(max_workgroups=mw) if SPEC[depth][4] else {}
    net = _step_net(k)
    tag = "%s step %s" % (depth, _tag(frame, mw, k, wl))
    for kind, cls, raw in (("plain", SPEC[depth][6], None), ("semi noraw", SPEC[depth][7], None), ("semi raw", SPEC[depth][7], x_raw)):
        syn.randomize_enet(net, seed=5)
        tr = getattr(T, cls)(net, 1e-3, **kw)
        conf = torch.zeros((k, k), dtype=torch.int64, device="cuda")
        semi_kw = {} if kind == "plain" else dict(labelled=labelled, images_raw=raw, confusion=conf, return_pseudo_pixels=True)

        def step():
            res = tr.step(x, labels, mask, **dict(call_kw, **semi_kw))
            return (res if isinstance(res, tuple) else (res, torch.zeros(0))) + tuple(tr._dev[s] for s in "wmv")
        _call(out, "%s %s" % (tag, kind), step, ("loss", "pseudo_pixels", "w", "m", "v"))
        out["%s %s confusion" % (tag, kind)] = icb._sha(conf)


def digests():
    import torch
    if HOST_ONLY:
        return {}
    torch.cuda.set_device(0)
    out = {}
    for depth in DEPTHS:
        for i, case in enumerate(_cases(depth, SHAPES)):
            _feature_records(out, depth, i, *case)
        for i, case in enumerate(_cases(depth, FRAMES)):
            _step_records(out, depth, i, *case)
    torch.cuda.synchronize()
    raised = sorted(key for key in out if key.endswith(" raised"))
    print("%d results, %d calls raised%s" % (len(out), len(raised), "".join("\n  " + key for key in raised)))
    return out


def _handle(k):
    from semanticsegmentationactivelearning_amd import synthetic as syn
    net = _step_net(k)
    syn.randomize_enet(net, seed=5)
    return net._sync_handle()


def workspace_bytes():
    """every size and offset query of the section at SHAPES (features) and at FRAMES and 8 h x 8 w (images), K = 2 and 19, and
    one refused shape each"""
    from semanticsegmentationactivelearning_amd import _lib
    L = _lib.lib()
    out = {}

    def put(name, *args):
        out["%s %s" % (name, " ".join(str(a) for a in args if isinstance(a, int)))] = int(getattr(L, name)(*args))
    for depth in DEPTHS:
        feat, img = SPEC[depth][:2]
        if depth != "final":
            for k in (1, 2, 19, 32, 33):
                put(feat.replace("_grad", "_param_floats"), k)
        for k in (2, 19):
            for n, h, w in SHAPES + [(0, 1, 1), (1, 1 << 30, 3)]:
                put(feat + "_workspace_bytes", n, h, w, k)
                for raw in ((0, 1) if depth != "final" else ((),)):
                    put(feat + "_semi_workspace_bytes", n, h, w, k, *((raw,) if depth != "final" else ()))
            if HOST_ONLY:
                continue
            handle = _handle(k)
            for n, h, w in FRAMES + [(n, 8 * h, 8 * w) for n, h, w in SHAPES] + [(1, 12, 8), (0, 8, 8)]:
                tag = (handle, n, h, w)
                out["%s K=%d %d %d %d" % ((img + "_workspace_bytes", k) + tag[1:])] = int(getattr(L, img + "_workspace_bytes")(*tag))
                for raw in (0, 1):
                    out["%s K=%d %d %d %d raw=%d" % ((img + "_semi_workspace_bytes", k) + tag[1:] + (raw,))] = int(
                        getattr(L, img + "_semi_workspace_bytes")(*(tag + (raw,))))
                for query in ([] if depth == "final" else [img + "_features_offset"]) + (
                        [img + "_code_offset"] if depth == "stage" else []):
                    out["%s K=%d %d %d %d" % ((query, k) + tag[1:])] = int(getattr(L, query)(*tag))
    return out


def _entry_args(depth, images, semi, handle, P, n, h, w, k):
    """[(name, value)] of one call of an entry, in the entry's order; P: the dummy pointer every pointer gets"""
    nam, takes_mw = SPEC[depth][3], SPEC[depth][4]
    semi_rule = [("labelled", P), ("measure", 0), ("threshold", 0.5)] if semi else []
    semi_out = [("confusion", P), ("pseudo_pixels", P)] if semi else []
    tail = ([("max_workgroups", 0)] if takes_mw else []) + [("loss", P), ("grad", P)] + semi_out + [
        ("ws", P), ("ws_bytes", 0), ("stream", None)]
    knobs = [("weight", 0.0), ("label_smoothing", 0.0)]
    if images:
        head = [("net", handle), ("x", P)] + ([("x_raw", P)] if semi else []) + [("x_is_u8", 1), ("n", n), ("h", h), ("w", w)]
        return head + [("labels", P), ("mask", P)] + semi_rule + [("params", P)] + knobs + tail
    feats = [("%s%d" % (side, i), P) for side in (("f", "raw") if semi else ("f",)) for i in range(1 + nam)]
    dims = [("n", n), ("h", h), ("w", w), ("classes", k)]
    return feats + dims + [("params", P), ("labels", P), ("mask", P)] + semi_rule + knobs + tail


def refused():
    """(return code, message) of the calls each training entry refuses, in the order it judges them"""
    from semanticsegmentationactivelearning_amd import _lib
    L = _lib.lib()
    k, (n, h, w) = 19, SHAPES[1]
    handle = None if HOST_ONLY else _handle(k)
    P = ctypes.c_void_p(4096)  # never read: every call is refused before a launch (the workspace is one byte short)
    out = {}
    for depth in DEPTHS:
        feat, img, unit, nam, takes_mw = SPEC[depth][:5]
        for images in ((False,) if HOST_ONLY else (False, True)):
            for semi in (False, True):
                stem = (img if images else feat) + ("_semi" if semi else "")
                dims = (n, 8 * h, 8 * w) if images else (n, h, w)
                query = (handle,) + dims if images else dims + (k,)
                need = int(getattr(L, stem + "_workspace_bytes")(*(query + ((1,) if semi and (images or depth != "final") else ()))))
                assert need > 0, (stem, need)
                args = _entry_args(depth, images, semi, handle, P, *dims, k)
                order = [name for name, _ in args]
                base = dict(args, ws_bytes=need - 1)
                cases = [("workspace one byte short", {}), ("bad dims", {"n": 0}), ("NULL loss", {"loss": None}),
                         ("NULL grad", {"grad": None}), ("NULL params", {"params": None}), ("NULL workspace", {"ws": None})]
                if takes_mw:
                    cases += [("negative max_workgroups", {"max_workgroups": -1})]
                if not semi:
                    cases += [("NULL labels", {"labels": None}), ("NULL mask", {"mask": None})]
                if images:
                    cases += [("NULL net", {"net": None}), ("NULL frames", {"x": None}), ("height not a multiple of 8", {"h": 8 * h + 4})]
                else:
                    cases += [("classes out of range", {"classes": 33}), ("classes below range", {"classes": 1}),
                              ("feature map beyond the limit", {"h": 1 << 30}), ("NULL features", {"f0": None})]
                    cases += [("NULL pooled indices %d" % i, {"f%d" % i: None}) for i in range(1, 1 + nam)]
                if semi:
                    cases += [("bad measure", {"measure": 3}), ("NULL labels, all labelled", {"labels": None, "labelled": None}),
                              ("NULL labels, some unlabelled", {"labels": None})]
                    # (a call without any raw pointer needs a smaller workspace, so it is not among these: it could launch)
                    if not images and nam:
                        cases += [("lone raw pointer %d" % i, dict({"raw%d" % j: None for j in range(1 + nam)}, **{"raw%d" % i: P}))
                                  for i in range(1 + nam)]
                for name, change in cases:
                    call = dict(base, **change)
                    rc = int(getattr(L, stem + "_nhwc")(*[call[a] for a in order]))
                    out["%s_nhwc: %s" % (stem, name)] = [rc, L.ssal_last_error().decode("utf-8", "replace") if rc else ""]
                    assert rc != 0, "%s_nhwc: %s was not refused" % (stem, name)
    return out


if __name__ == "__main__":
    if "--host" in sys.argv:
        sys.argv.remove("--host")
        HOST_ONLY = True
    icb.main(os.path.join(ROOT, "profiles", "r28_train_enet_bits.json"), (digests, workspace_bytes, refused),
             sum(len(_cases(d, SHAPES)) + len(_cases(d, FRAMES)) for d in DEPTHS))
