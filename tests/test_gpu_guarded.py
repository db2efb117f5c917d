"""Every entry point on poisoned workspaces and guarded outputs (tests/guarded_alloc.py; DESIGN.md "Poisoned workspaces").

Each case runs once per pattern (0xFF, 0x7F, 0xFE).  Before EVERY call under test (``put.fresh()``) the guards are checked
and the model's cached workspaces are dropped, so the call allocates its workspace under the patch -- every byte the pattern,
at exactly the size its own query returns -- and never sees what an earlier call of the case left there; outputs are poisoned
by construction and the inputs sit between two guards.  Per case:
  1. no guard of any allocation changed, after every call (``check()``),
  2. the three runs give the same bits (compared as bytes: a NaN cannot differ from itself by accident),
  3. "oracle" cases: the result equals the oracle exactly as the entry's own test asserts it (its helpers are reused),
  4. "clean" cases: the result equals the same call outside the harness, bit for bit.
Each case asserts that the call went through the patch: the allocation count, ``is_guarded(net._ws)`` after every call on a
model, and ``is_guarded`` of every output that a wrapper allocates (the trainers' feature entries and the stand-alone
operators have no model workspace: there the outputs and the allocation count carry it).  The sequence tests alone keep one
workspace across calls."""
import numpy as np
import pytest
import torch

import semanticsegmentationactivelearning_amd as ssal
import test_gpu_parity as parity
import test_icnet_gpu as icn
from guarded_alloc import PATTERNS, GuardedAlloc, same_bits
from helpers import frames, make_model, report_diff
from oracle import dropout_oracle as dorc
from oracle import enet_oracle as orc
from oracle import icnet_oracle as ico
from semanticsegmentationactivelearning_amd import _lib, active_learning as al, inference as inf, synthetic as syn, training
from semanticsegmentationactivelearning_amd.models.util import conv_ops as cops
from semanticsegmentationactivelearning_amd.models.util import extra_ops as xops
from semanticsegmentationactivelearning_amd.tensortools import losses, metrics

pytestmark = pytest.mark.gpu
TOL = 1e-4  # north_star: per-pixel confidences within 1e-4 (the bound of the entries' own tests)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    _lib.lib()
    yield
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def icnet19():
    net = ssal.ICNet(19)
    net.build((None, None, None, 3))
    syn.randomize_icnet(net, seed=0)
    return net, syn.icnet_params_dict(net)


def _plain(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).cuda()


def _host(res):
    out = {}
    for k, v in res.items():
        if v is None:
            continue
        out[k] = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    return out


def _same(tag, a, b):
    assert sorted(a) == sorted(b), "%s: results %s / %s" % (tag, sorted(a), sorted(b))
    for k in a:
        if not same_bits(a[k], b[k]):
            x, y = np.ascontiguousarray(a[k]).view(np.uint8).ravel(), np.ascontiguousarray(b[k]).view(np.uint8).ravel()
            if a[k].shape != b[k].shape or a[k].dtype != b[k].dtype:
                raise AssertionError("%s: %s is %s %s / %s %s" % (tag, k, a[k].shape, a[k].dtype, b[k].shape, b[k].dtype))
            bad = np.flatnonzero(x != y)
            first = int(bad[0]) // a[k].dtype.itemsize
            raise AssertionError("%s: %s differs in %d bytes of %d; first at element %s: %r / %r"
                                 % (tag, k, bad.size, x.size, np.unravel_index(first, a[k].shape) if a[k].shape else (),
                                    a[k].ravel()[first], b[k].ravel()[first]))


class _Put:
    """what a body gets: ``put(array)`` places an input (inside a poisoned slab under the harness, a plain copy outside it);
    ``put.fresh()`` goes before EVERY call under test: the guards the previous call could have touched are checked, its
    workspace must have come from the patch, and every cached workspace is dropped, so that the next call allocates its own
    under the patch -- pattern-filled, at exactly the size its own query returns; ``put.adopt(net)`` registers a model the
    body built itself"""

    def __init__(self, g, nets, tag):
        self.g, self.nets, self.tag, self.calls = g, list(nets), tag, 0

    def __call__(self, a):
        return _plain(a) if self.g is None else self.g.guarded_from_numpy(a)

    def adopt(self, net):
        self.nets.append(net)
        return net

    def verify(self):
        if self.g is None:
            return
        self.g.check()
        for i, net in enumerate(self.nets):
            if i < self.fixed or net._ws is not None:  # a model the body built may be used through feature entries only
                assert self.g.is_guarded(net._ws), "%s: call %d: the model's workspace did not come from the patched torch.empty" % (
                    self.tag, self.calls)

    def fresh(self):
        if self.calls:
            self.verify()
        for net in self.nets:
            net._workspaces.clear()
            net._tls.last = (None, None, None, None)
        self.calls += 1


def guarded(body, nets=(), clean=False, tag=""):
    """``body(put) -> {name: tensor}`` under each pattern, then -- with ``clean`` -- outside the harness.  The body calls
    ``put.fresh()`` before every call under test (see ``_Put``).  Outputs whose name does not start with "~" must be
    interiors of guarded slabs.  Returns the (pattern-independent) host results."""
    runs = []
    for pattern in PATTERNS:
        with GuardedAlloc("cuda", pattern) as g:
            put = _Put(g, nets, tag)
            put.fixed = len(put.nets)
            res = body(put)
            assert put.calls > 0 or not put.nets, "%s: the body never called put.fresh()" % tag  # no model: no cached workspace
            assert g.count > 0, "%s: the call allocated nothing through torch.empty / torch.empty_like" % tag
            for k, v in res.items():
                if isinstance(v, torch.Tensor) and v.is_cuda and not k.startswith("~"):
                    assert g.is_guarded(v), "%s: output %r did not come from the patched torch.empty" % (tag, k)
            put.verify()
            runs.append(_host(res))
        for net in put.nets:
            net._workspaces.clear()
            net._tls.last = (None, None, None, None)
    for pattern, r in zip(PATTERNS[1:], runs[1:]):
        _same("%s pattern 0x%02X vs 0x%02X" % (tag, pattern, PATTERNS[0]), r, runs[0])
    if clean:
        put = _Put(None, nets, tag)
        put.fixed = len(put.nets)
        _same("%s guarded vs clean" % tag, runs[0], _host(body(put)))
    return {k.lstrip("~"): v for k, v in runs[0].items()}


# ---- ENet layers -------------------------------------------------------------------------------------------------------------
# one ragged shape per layer name of the parity table: one 8 x 32 tile plus a tail in both axes (odd H and W where the layer
# allows it; the down-sampling layers and Initial need even sizes), and the shapes of test_gpu_bottleneck_phases whose
# dilation phases are unequal, have no rows, or leave tiles empty
def _ragged(net, name):
    kind = type(getattr(net, name)).__name__
    return (18, 38) if kind in ("Initial", "BottleneckDownsample") else (9, 35)


LAYER_CASES = [(name, None, None) for name, _, _ in parity._layer_cases()] + [
    ("Bottleneck2_2", 1, 34), ("Bottleneck2_4", 3, 67), ("Bottleneck2_6", 5, 133), ("Bottleneck2_8", 17, 257)]


def _layer_input(net, name, h, w, seed=16):
    layer = getattr(net, name)
    kind = type(layer).__name__
    cin = {"Initial": 3, "Final": 16}.get(name)
    if cin is None:
        cin = layer.proj_kernel.shape[2]
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(1, h, w, cin)).astype(np.float32)
    if kind == "BottleneckDownsample":
        x[0, :2, :2, :] = 0.25  # an all-equal pooling window: the first element must win
    arg = None
    if kind == "BottleneckUpsample":
        _, arg = orc.maxpool2x2_argmax(rng.normal(size=(1, 2 * h, 2 * w, layer.output_channels)).astype(np.float32))
    return layer, kind, x, arg


def _layer_body(layer, kind, x, arg, **kw):
    def body(put):
        put.fresh()
        if kind == "BottleneckDownsample":
            y, a = layer(put(x), training=False, **kw)
            return {"y": y, "argmax": a}
        if kind == "BottleneckUpsample":
            return {"y": layer(put(x), put(arg), training=False, **kw)}
        if kind == "Final":
            return {"y": layer(put(x))}
        return {"y": layer(put(x), training=False, **kw)}
    return body


def _layer_oracle(P, name, layer, kind, x, arg):
    if kind == "Initial":
        return {"y": orc.initial(P, name, x)}
    if kind == "Bottleneck":
        return {"y": orc.bottleneck(P, name, x, dil=layer.dilation_rate[0], asym=layer.asymmetric)}
    if kind == "BottleneckDownsample":
        y, a = orc.bottleneck_down(P, name, x)
        return {"y": y, "argmax": a}
    if kind == "BottleneckUpsample":
        return {"y": orc.bottleneck_up(P, name, x, arg)}
    return {"y": orc.final(P, name, x)}


@pytest.mark.parametrize("family", [True, False], ids=["mfma", "generic"])
@pytest.mark.parametrize("name,h,w", LAYER_CASES)
def test_enet_layer(enet_c3k19, name, h, w, family):
    net, P = enet_c3k19
    if h is None:
        h, w = _ragged(net, name)
    layer, kind, x, arg = _layer_input(net, name, h, w)
    tag = "%s %dx%d %s" % (name, h, w, "mfma" if family else "generic")
    try:
        _lib.set_kernel_family(family)
        got = guarded(_layer_body(layer, kind, x, arg), nets=(net,), tag=tag)
    finally:
        _lib.set_kernel_family(True)
    for k, want in _layer_oracle(P, name, layer, kind, x, arg).items():
        report_diff("%s %s (bit-exact)" % (tag, k), got[k], want)


@pytest.mark.parametrize("family", [True, False], ids=["mfma", "generic"])
@pytest.mark.parametrize("name", ["Bottleneck4_0", "Bottleneck5_0"])
def test_enet_upsample_layer_scatter_form(enet_c3k19, name, family):
    """arbitrary (unique) indices take the scatter form of the unpooling; pooling-derived ones (test_enet_layer) the gather"""
    net, P = enet_c3k19
    h, w = 9, 35
    layer, kind, x, _ = _layer_input(net, name, h, w)
    cout = layer.output_channels
    arg = np.random.default_rng(19).permutation(4 * h * w * cout)[: h * w * cout].reshape(1, h, w, cout).astype(np.int64)
    try:
        _lib.set_kernel_family(family)
        got = guarded(_layer_body(layer, kind, x, arg), nets=(net,), tag=name + " scatter")
    finally:
        _lib.set_kernel_family(True)
    report_diff(name + " scatter form (bit-exact)", got["y"], orc.bottleneck_up(P, name, x, arg))


@pytest.mark.parametrize("name,h,w", [("Bottleneck2_0", 18, 38), ("Bottleneck2_1", 9, 35), ("Bottleneck2_3", 9, 35),
                                      ("Bottleneck2_8", 17, 257), ("Bottleneck4_0", 9, 35)])
def test_enet_layer_bf16x3_against_its_own_clean_run(enet_c3k19, name, h, w):
    net, _ = enet_c3k19
    layer, kind, x, arg = _layer_input(net, name, h, w)
    got = guarded(_layer_body(layer, kind, x, arg, arithmetic="bf16x3"), nets=(net,), clean=True, tag=name + " bf16x3")
    assert np.isfinite(got["y"]).all()


# ---- ENet, whole network -----------------------------------------------------------------------------------------------------
NET_SHAPES = [(1, 8, 8), (3, 24, 40), (1, 136, 72)]
_ENET_REF = {}


def _enet_ref(P, n, h, w):
    """oracle of one frame set: computed once, shared, never written to"""
    if (n, h, w) not in _ENET_REF:
        x = frames(range(20, 20 + n), h, w, 3)
        ep = {}
        logits = orc.enet_forward(P, x, ep)
        ref = {"x": x, "logits": logits, "argmax1": ep["argmax1"], "argmax2": ep["argmax2"], "b3_8": ep["Bottleneck3_8"],
               "b4_2": ep["Bottleneck4_2"], "b5_1": ep["Bottleneck5_1"]}
        for m in ("entropy", "margin", "confidence"):
            ref[m] = orc.score_logits(logits, m)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _ENET_REF[n, h, w] = ref
    return _ENET_REF[n, h, w]


@pytest.mark.parametrize("n,h,w", NET_SHAPES)
def test_enet_forward_endpoints_and_pooling_argmax(enet_c3k19, n, h, w):
    net, P = enet_c3k19
    ref = _enet_ref(P, n, h, w)

    def body(put):
        put.fresh()
        logits = net(put(ref["x"]), training=False)
        _, b5_1, b4_2, b3_8 = net.endpoint_outputs[-1]
        a1, a2 = net.pooling_argmax()
        return {"logits": logits, "~b5_1": b5_1, "~b4_2": b4_2, "~b3_8": b3_8, "argmax1": a1, "argmax2": a2}
    got = guarded(body, nets=(net,), tag="forward %dx%dx%d" % (n, h, w))
    for k in ("b3_8", "b4_2", "b5_1", "logits", "argmax1", "argmax2"):
        report_diff("%dx%dx%d %s vs C oracle (bit-exact)" % (n, h, w, k), got[k], ref[k])


@pytest.mark.parametrize("measure", ["entropy", "margin", "confidence"])
@pytest.mark.parametrize("n,h,w", NET_SHAPES)
def test_enet_score_forms(enet_c3k19, n, h, w, measure):
    """score with label + mask + confidence, the score-only form (fused ends), the uint8 form, and the saved pooling indices"""
    net, P = enet_c3k19
    ref = _enet_ref(P, n, h, w)
    want_mean, want_conf, want_label = ref[measure]
    thr = float(np.median(want_conf))
    u8 = np.stack([syn.synth_frame_u8(f, h, w, 3) for f in range(20, 20 + n)])
    assert np.array_equal(syn.u8_to_f32(u8), ref["x"])

    def body(put):
        put.fresh()  # the ranking pass first: its fused ends run on a workspace no other form has touched
        only = net.score(put(ref["x"]), measure)
        b1, b2 = net.pooling_argmax()
        put.fresh()
        s, e = net.score(put(ref["x"]), measure, threshold=thr, return_label=True, return_mask=True, return_confidence=True)
        a1, a2 = net.pooling_argmax()
        put.fresh()
        u8_only = net.score(put(u8), measure)
        put.fresh()
        su, eu = net.score(put(u8), measure, threshold=thr, return_label=True, return_confidence=True)
        return {"scores": s, "label": e["label"], "mask": e["mask"], "confidence": e["confidence"], "argmax1": a1, "argmax2": a2,
                "only": only, "only_argmax1": b1, "only_argmax2": b2, "u8": su, "u8_only": u8_only,
                "u8_label": eu["label"], "u8_confidence": eu["confidence"]}
    got = guarded(body, nets=(net,), clean=True, tag="score %s %dx%dx%d" % (measure, n, h, w))
    report_diff("label (bit-exact argmax)", got["label"], want_label)
    report_diff("confidence", got["confidence"], want_conf, exact=False, atol=TOL)
    report_diff("mean", got["scores"], want_mean, exact=False, atol=1e-6)
    assert (got["mask"] == (got["confidence"] >= np.float32(thr))).all()
    for a in ("argmax1", "argmax2"):
        report_diff(a, got[a], ref[a])
        report_diff("score-only " + a, got["only_" + a], ref[a])
    for k in ("only", "u8", "u8_only"):
        assert same_bits(got[k], got["scores"]), "%s form: %r != %r" % (k, got[k], got["scores"])
    assert same_bits(got["u8_label"], got["label"]) and same_bits(got["u8_confidence"], got["confidence"])


@pytest.mark.parametrize("n,h,w", NET_SHAPES)
def test_enet_evaluate_regions_and_predict(enet_c3k19, n, h, w):
    net, P = enet_c3k19
    ref = _enet_ref(P, n, h, w)
    rng = np.random.default_rng(31)
    lab = rng.integers(0, 19, (n, h, w)).astype(np.uint8)
    lab[rng.uniform(size=lab.shape) < 0.05] = 255
    msk = (rng.uniform(size=(n, h, w)) > 0.3).astype(np.uint8)
    emb = np.zeros(256, np.uint8)
    emb[:19] = [7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33]
    cmap = np.random.default_rng(32).integers(0, 256, (19, 3)).astype(np.uint8)
    size = (h + 5, w - 3)

    def body(put):
        def each(call):
            put.fresh()
            return call()
        cm0 = each(lambda: net.evaluate(put(ref["x"]), put(lab)))
        cm = each(lambda: net.evaluate(put(ref["x"]), put(lab), put(msk)))
        s32, r32 = each(lambda: net.score_regions(put(ref["x"]), 32, "entropy"))
        s20, r20, m20 = each(lambda: net.score_regions(put(ref["x"]), (20, 12), "entropy", return_label=True))
        return {"~cm": cm, "~cm0": cm0, "s32": s32, "r32": r32, "s20": s20, "r20": r20, "l20": m20["label"],
                "ids": each(lambda: inf.predict(net, put(ref["x"]))),
                "emb": each(lambda: inf.predict(net, put(ref["x"]), embedding_reversed=emb)),
                "rgb": each(lambda: inf.predict(net, put(ref["x"]), colormap=cmap)),
                "emb_resized": each(lambda: inf.predict(net, put(ref["x"]), size=size, embedding_reversed=emb)),
                "ids_resized": each(lambda: inf.predict(net, put(ref["x"]), size=size))}
    got = guarded(body, nets=(net,), clean=True, tag="evaluate / regions / predict %dx%dx%d" % (n, h, w))
    want_mean, want_conf, want_label = ref["entropy"]
    pred = want_label.astype(np.int64)
    keep = lab < 19
    for k, wt in (("cm", msk.astype(np.int64)), ("cm0", np.ones_like(pred))):
        want = np.bincount((lab[keep].astype(np.int64) * 19 + pred[keep]), weights=wt[keep], minlength=361).reshape(19, 19)
        report_diff("confusion matrix " + k, got[k], want.astype(np.int64))
    report_diff("labels", got["ids"], want_label)
    report_diff("labels of score_regions", got["l20"], want_label)
    report_diff("dataset ids", got["emb"], emb[want_label])
    report_diff("colours", got["rgb"], cmap[want_label])
    assert same_bits(got["emb_resized"], emb[got["ids_resized"]])
    for k in ("s32", "s20"):
        report_diff(k + " mean", got[k], want_mean, exact=False, atol=1e-6)
    for k, (rh, rw) in (("r32", (32, 32)), ("r20", (20, 12))):
        ry, rx = -(-h // rh), -(-w // rw)
        want = np.array([[[want_conf[i, y * rh:(y + 1) * rh, x * rw:(x + 1) * rw].astype(np.float64).mean()
                           for x in range(rx)] for y in range(ry)] for i in range(n)])
        report_diff(k + " region means", got[k], want, exact=False, atol=TOL)


KNOBS = [("fuse_ends", 0), ("img_groups", 1), ("bnk_w8", 0), ("bnk_w8", 1), ("bnk_w8", 2), ("bnk_xcd", 0)]


@pytest.mark.parametrize("knob,value", KNOBS)
def test_enet_knobs_leave_the_bits_alone(enet_c3k19, knob, value):
    net, P = enet_c3k19
    ref = _enet_ref(P, 3, 24, 40)

    def body(put):
        put.fresh()
        only = net.score(put(ref["x"]), "entropy")
        put.fresh()
        s, e = net.score(put(ref["x"]), "entropy", return_label=True, return_confidence=True)
        return {"scores": s, "label": e["label"], "confidence": e["confidence"], "only": only}
    start = _lib.get_knobs()[knob]
    want = guarded(body, nets=(net,), tag="default knobs")
    try:
        _lib.set_knob(knob, value)
        got = guarded(body, nets=(net,), tag="%s=%d" % (knob, value))
    finally:
        _lib.set_knob(knob, start)
    assert _lib.get_knobs()["defaults"] == 1
    _same("%s=%d vs the default knobs" % (knob, value), got, want)
    report_diff("label", got["label"], ref["entropy"][2])


# ---- ICNet operators -----------------------------------------------------------------------------------------------------------
def _table(test_function):
    (mark,) = [m for m in test_function.pytestmark if m.name == "parametrize" and "," in m.args[0]]
    return list(mark.args[1])


@pytest.mark.parametrize("kh,cin,cout,stride,dil,n,h,w,res,relu,up2", _table(icn.test_conv_bn_act_bit_exact))
def test_icnet_conv_bn_act(kh, cin, cout, stride, dil, n, h, w, res, relu, up2):
    rng = np.random.default_rng(kh * 1000 + cin + cout + h)
    x = rng.normal(size=(n, h, w, cin)).astype(np.float32)
    k = (rng.normal(size=(kh, kh, cin, cout)) / np.sqrt(kh * kh * cin)).astype(np.float32)
    use_bias = cout in (19, 5)
    bn = None if use_bias else icn._bn(rng, cout)
    bias = rng.normal(size=cout).astype(np.float32) if use_bias else None
    hh, ww = (2 * h, 2 * w) if up2 else (h, w)
    oh, ow = -(-hh // stride), -(-ww // stride)
    r = rng.normal(size=(n, oh, ow, cout)).astype(np.float32) if res else None

    def body(put):
        return {"y": cops.conv_bn_act(put(x), k, stride, dil, bn=bn, bias=bias, residual=None if r is None else put(r),
                                      relu=relu, upsample2x=up2)}
    got = guarded(body, tag="conv_bn_act")
    report_diff("conv_bn_act", got["y"], icn._oracle_conv(x, k, stride, dil, bn, bias, r, relu, up2))


@pytest.mark.parametrize("cin,h,w", _table(icn.test_first_conv_bit_exact))
def test_icnet_first_conv(cin, h, w):
    rng = np.random.default_rng(cin + h)
    x = rng.uniform(0, 1, size=(2, h, w, cin)).astype(np.float32)
    k = (rng.normal(size=(3, 3, cin, 32)) / 5).astype(np.float32)
    bn = icn._bn(rng, 32)
    got = guarded(lambda put: {"y": cops.conv_bn_act(put(x), k, 2, 1, bn=bn, relu=True)}, tag="first conv")
    report_diff("first conv", got["y"], icn._oracle_conv(x, k, 2, 1, bn, None, None, True, False))


@pytest.mark.parametrize("n,h,w,c", _table(icn.test_max_pool_3x3_s2))
def test_icnet_max_pool_3x3_s2(n, h, w, c):
    x = np.random.default_rng(h).normal(size=(n, h, w, c)).astype(np.float32)
    got = guarded(lambda put: {"y": cops.max_pool_3x3_s2(put(x))}, tag="maxpool")
    report_diff("maxpool", got["y"], ico.maxpool3x3_s2(x))


@pytest.mark.parametrize("n,h,w,c", _table(icn.test_pyramid_pooling))
def test_icnet_pyramid_pooling(n, h, w, c):
    x = np.random.default_rng(w).normal(size=(n, h, w, c)).astype(np.float32)
    got = guarded(lambda put: {"y": cops.pyramid_pooling(put(x))}, tag="ppm")
    report_diff("ppm", got["y"], ico.pyramid_pooling(x))


@pytest.mark.parametrize("measure", ["margin", "entropy", "confidence"])
@pytest.mark.parametrize("n,h,w,k", [(2, 8, 12, 19), (1, 5, 3, 6), (1, 16, 16, 2)])
def test_icnet_upscore(measure, n, h, w, k):
    lq = (np.random.default_rng(k + h).normal(size=(n, h, w, k)) * 4).astype(np.float32)
    want_mean, want_conf, want_label = orc.score_logits(ico.resize_bilinear(lq, 4 * h, 4 * w), measure)
    thr = float(np.median(want_conf))

    def body(put):
        s, e = cops.upscore_logits(put(lq), measure, threshold=thr, return_label=True, return_mask=True, return_confidence=True)
        return {"scores": s, "label": e["label"], "mask": e["mask"], "confidence": e["confidence"],
                "only": cops.upscore_logits(put(lq), measure)}
    got = guarded(body, tag="upscore")
    report_diff("label", got["label"], want_label)
    report_diff("confidence", got["confidence"], want_conf, exact=False, atol=TOL)
    report_diff("mean", got["scores"], want_mean, exact=False, atol=1e-6)
    assert (got["mask"] == (got["confidence"] >= np.float32(thr))).all()
    assert same_bits(got["only"], got["scores"])


# ---- ICNet, whole network ----------------------------------------------------------------------------------------------------
ICNET_SHAPES = [(1, 32, 32), (3, 96, 64)]
_ICNET_REF = {}


def _icnet_ref(P, n, h, w):
    if (n, h, w) not in _ICNET_REF:
        x = frames(list(range(20, 20 + n)), h, w, 3)
        ep = {}
        logits = ico.icnet_forward(P, x, ep)
        ref = {"x": x, "logits": logits, "ep": ep}
        for m in ("margin", "entropy"):
            ref[m] = orc.score_logits(logits, m)
        _ICNET_REF[n, h, w] = ref
    return _ICNET_REF[n, h, w]


def _icnet_body(net, ref, lab, msk, thr):
    def body(put):
        def each(call):
            put.fresh()
            return call()
        only = each(lambda: net.score(put(ref["x"]), "margin"))
        cm = each(lambda: net.evaluate(put(ref["x"]), put(lab), put(msk)))
        s32, r32 = each(lambda: net.score_regions(put(ref["x"]), 32, "entropy"))
        s20, r20, m20 = each(lambda: net.score_regions(put(ref["x"]), (20, 12), "entropy", return_label=True))
        s, e = each(lambda: net.score(put(ref["x"]), "margin", threshold=thr, return_label=True, return_mask=True,
                                      return_confidence=True))
        logits = each(lambda: net(put(ref["x"]), training=False))
        ends = {"~" + nm: net.endpoint(nm).clone() for nm in net.endpoint_names()}
        return dict(ends, logits=logits, scores=s, label=e["label"], mask=e["mask"], confidence=e["confidence"], only=only,
                    s32=s32, r32=r32, s20=s20, r20=r20, l20=m20["label"], **{"~cm": cm})
    return body


def _icnet_planes(n, h, w):
    rng = np.random.default_rng(33)
    lab = rng.integers(0, 19, (n, h, w)).astype(np.uint8)
    lab[rng.uniform(size=lab.shape) < 0.05] = 255
    return lab, (rng.uniform(size=(n, h, w)) > 0.3).astype(np.uint8)


@pytest.mark.parametrize("n,h,w", ICNET_SHAPES)
def test_icnet_forward_score_evaluate_regions(icnet19, n, h, w):
    net, P = icnet19
    ref = _icnet_ref(P, n, h, w)
    want_mean, want_conf, want_label = ref["margin"]
    thr = float(np.median(want_conf))
    lab, msk = _icnet_planes(n, h, w)
    got = guarded(_icnet_body(net, ref, lab, msk, thr), nets=(net,), clean=True, tag="ICNet %dx%dx%d" % (n, h, w))
    names = net.endpoint_names()
    assert len(names) > 60
    for nm in names:
        report_diff("%s (bit-exact)" % nm, got[nm], ref["ep"][nm])
    report_diff("logits vs C oracle (bit-exact)", got["logits"], ref["logits"])
    report_diff("label (bit-exact argmax)", got["label"], want_label)
    report_diff("confidence", got["confidence"], want_conf, exact=False, atol=TOL)
    report_diff("mean", got["scores"], want_mean, exact=False, atol=1e-6)
    assert (got["mask"] == (got["confidence"] >= np.float32(thr))).all()
    assert same_bits(got["only"], got["scores"])
    keep = lab < 19
    want = np.bincount(lab[keep].astype(np.int64) * 19 + want_label[keep], weights=msk[keep].astype(np.int64), minlength=361)
    report_diff("confusion matrix", got["cm"], want.reshape(19, 19).astype(np.int64))
    e_mean, e_conf, _ = ref["entropy"]
    report_diff("labels of score_regions", got["l20"], want_label)
    for k in ("s32", "s20"):
        report_diff(k + " mean", got[k], e_mean, exact=False, atol=1e-6)
    for k, (rh, rw) in (("r32", (32, 32)), ("r20", (20, 12))):
        ry, rx = -(-h // rh), -(-w // rw)
        want = np.array([[[e_conf[i, y * rh:(y + 1) * rh, x * rw:(x + 1) * rw].astype(np.float64).mean()
                           for x in range(rx)] for y in range(ry)] for i in range(n)])
        report_diff(k + " region means", got[k], want, exact=False, atol=TOL)


@pytest.mark.parametrize("knob,value", [("ic_front", 0), ("ic_dual", 0), ("ig_sb", 0), ("ic_groups", 2)])
def test_icnet_knobs_leave_the_bits_alone(icnet19, knob, value):
    net, P = icnet19
    ref = _icnet_ref(P, 3, 96, 64)
    lab, msk = _icnet_planes(3, 96, 64)
    thr = float(np.median(ref["margin"][1]))
    body = _icnet_body(net, ref, lab, msk, thr)
    start = _lib.get_knobs()[knob]
    want = guarded(body, nets=(net,), tag="ICNet default knobs")
    try:
        _lib.set_knob(knob, value)
        got = guarded(body, nets=(net,), tag="ICNet %s=%d" % (knob, value))
    finally:
        _lib.set_knob(knob, start)
    assert _lib.get_knobs()["defaults"] == 1
    _same("ICNet %s=%d vs the default knobs" % (knob, value), got, want)
    report_diff("logits vs C oracle (bit-exact)", got["logits"], ref["logits"])


# ---- stand-alone operators ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", ["entropy", "margin", "confidence"])
@pytest.mark.parametrize("n,h,w,k", [(3, 24, 40, 2), (2, 3, 3, 19), (1, 8, 8, 32), (1, 5, 7, 6)])
def test_score_logits(measure, n, h, w, k):
    lg = (np.random.default_rng(15).normal(size=(n, h, w, k)) * 4).astype(np.float32)
    lg[0, 0, 0, :] = 1.25
    want_mean, want_conf, want_label = orc.score_logits(lg, measure)
    thr = float(np.median(want_conf))

    def body(put):
        s, e = al.score_logits(put(lg), measure, threshold=thr, return_label=True, return_mask=True, return_confidence=True)
        s2, r2 = al.score_logits(put(lg), measure, region=(3, 4))
        return {"scores": s, "label": e["label"], "mask": e["mask"], "confidence": e["confidence"],
                "only": al.score_logits(put(lg), measure), "region_scores": s2, "regions": r2}
    got = guarded(body, clean=True, tag="score_logits")
    assert same_bits(got["region_scores"], got["scores"])  # "the per-image scores keep their bits"
    ry, rx = -(-h // 3), -(-w // 4)
    want_r = np.array([[[want_conf[i, y * 3:(y + 1) * 3, x * 4:(x + 1) * 4].astype(np.float64).mean() for x in range(rx)]
                        for y in range(ry)] for i in range(n)])
    report_diff("region means", got["regions"], want_r, exact=False, atol=TOL)
    report_diff("label (bit-exact argmax)", got["label"], want_label)
    report_diff("confidence", got["confidence"], want_conf, exact=False, atol=TOL)
    assert np.abs(got["confidence"] - want_conf).max() < 5e-6
    report_diff("mean", got["scores"], want_mean, exact=False, atol=1e-6)
    report_diff("mean, score-only form", got["only"], want_mean, exact=False, atol=1e-6)
    assert (got["mask"] == (got["confidence"] >= np.float32(thr))).all()


@pytest.mark.parametrize("weight,ls,k", [(0.0, 0.0, 19), (1.5, 0.05, 19), (1.02, 0.1, 6)])
def test_masked_softmax_cross_entropy(weight, ls, k):
    rng = np.random.default_rng(21)
    lg = (rng.normal(size=(3, 12, 20, k)) * 3).astype(np.float32)
    lab = rng.integers(0, k, size=(3, 12, 20)).astype(np.uint8)
    mask = (rng.uniform(size=(3, 12, 20)) > 0.3).astype(np.float32)
    want = orc.masked_softmax_cross_entropy(lab, lg, mask, k, weight, ls)
    got = guarded(lambda put: {"loss": losses.masked_softmax_cross_entropy(put(lab), put(lg), put(mask), k, weight, ls)},
                  clean=True, tag="xent")
    loss = float(got["loss"].ravel()[0])
    assert abs(loss - want) <= 1e-5 * max(1.0, abs(want)), (loss, want)


@pytest.mark.parametrize("k,n,h,w", [(19, 2, 13, 21), (2, 1, 3, 5), (32, 1, 40, 24)])
def test_confusion_mat_and_region_means(k, n, h, w):
    rng = np.random.default_rng(41)
    lab = rng.integers(0, k, (n, h, w)).astype(np.uint8)
    lab[rng.uniform(size=lab.shape) < 0.05] = 255
    pred = rng.integers(0, k, (n, h, w)).astype(np.uint8)
    wts = rng.integers(0, 3, (n, h, w)).astype(np.uint8)
    plane = rng.uniform(size=(n, h, w)).astype(np.float32)

    def body(put):
        return {"~cm": metrics.confusion_mat(put(lab), put(pred), k, weights=put(wts)),
                "~cm1": metrics.confusion_mat(put(lab), put(pred), k),
                "r": _lib.region_means_plane(put(plane), (5, 7)), "r32": _lib.region_means_plane(put(plane), 32)}
    got = guarded(body, clean=True, tag="confusion / region means")
    keep = lab < k
    key = lab[keep].astype(np.int64) * k + pred[keep]
    report_diff("confusion (weights)", got["cm"], np.bincount(key, weights=wts[keep], minlength=k * k).reshape(k, k).astype(np.int64))
    report_diff("confusion", got["cm1"], np.bincount(key, minlength=k * k).reshape(k, k).astype(np.int64))
    for name, (rh, rw) in (("r", (5, 7)), ("r32", (32, 32))):
        want, _ = _lib.region_reduce_host(plane, h, w, (rh, rw), form="plane")
        report_diff("region means " + name, got[name], want)


@pytest.mark.parametrize("include_batch", [False, True])
def test_max_pool_with_argmax_and_unpool(include_batch):
    rng = np.random.default_rng(12)
    x = rng.uniform(size=(3, 6, 10, 5)).astype(np.float32)
    x[0, :2, :2, 0] = 0.5
    want_y, want_i = orc.maxpool2x2_argmax(x, include_batch=include_batch)

    def body(put):
        y, idx = xops.max_pool_with_argmax(put(x), include_batch_in_index=include_batch)
        return {"y": y, "idx": idx, "up": xops.unpool_2d(y, idx, idx_has_batch=include_batch)}
    got = guarded(body, tag="pool / unpool")
    report_diff("pool", got["y"], want_y)
    report_diff("argmax", got["idx"], want_i)
    report_diff("unpool", got["up"], orc.unpool2d(want_y, want_i, idx_has_batch=include_batch))


@pytest.mark.parametrize("kh,kw,stride,dil,h,w,cin,cout", [(1, 1, 1, 1, 9, 7, 16, 64), (3, 3, 1, 4, 9, 11, 32, 32),
                                                           (5, 1, 1, 1, 12, 10, 32, 32), (1, 5, 1, 1, 12, 10, 32, 32),
                                                           (2, 2, 2, 1, 8, 8, 64, 32), (3, 3, 1, 1, 6, 5, 8, 8),
                                                           (3, 3, 2, 1, 9, 7, 4, 8)])
def test_conv2d_same(kh, kw, stride, dil, h, w, cin, cout):
    rng = np.random.default_rng(10)
    x = rng.normal(size=(2, h, w, cin)).astype(np.float32)
    k = (rng.normal(size=(kh, kw, cin, cout)) * 0.2).astype(np.float32)
    want = orc.conv2d_same(x, k, stride, dil)

    def body(put):
        xd, kd = put(x), put(k)
        y = torch.empty(want.shape, dtype=torch.float32, device="cuda")
        _lib.check(_lib.lib().ssal_conv2d_same(_lib.dev_ptr(xd), 2, h, w, cin, _lib.dev_ptr(kd), kh, kw, cout, stride, dil,
                                               _lib.dev_ptr(y), _lib.stream_ptr()))
        torch.cuda.synchronize()
        return {"y": y}
    report_diff("conv2d", guarded(body, tag="conv2d_same")["y"], want)


@pytest.mark.parametrize("h,w,cin,cout", [(5, 7, 16, 8), (1, 1, 4, 4)])
def test_conv2d_transpose(h, w, cin, cout):
    rng = np.random.default_rng(11)
    x = rng.normal(size=(2, h, w, cin)).astype(np.float32)
    k = (rng.normal(size=(3, 3, cout, cin)) * 0.2).astype(np.float32)
    want = orc.conv2d_transpose_3x3_s2(x, k)

    def body(put):
        xd, kd = put(x), put(k)
        y = torch.empty(want.shape, dtype=torch.float32, device="cuda")
        _lib.check(_lib.lib().ssal_conv2d_transpose_3x3_s2(_lib.dev_ptr(xd), 2, h, w, cin, _lib.dev_ptr(kd), cout,
                                                           _lib.dev_ptr(y), _lib.stream_ptr()))
        torch.cuda.synchronize()
        return {"y": y}
    report_diff("conv2d_transpose", guarded(body, tag="conv2d_transpose")["y"], want)


@pytest.mark.parametrize("c,oh,ow", [(3, 13, 10), (8, 2, 3), (64, 10, 14)])
def test_resize_bilinear(c, oh, ow):
    x = np.random.default_rng(14).normal(size=(2, 5, 7, c)).astype(np.float32)
    got = guarded(lambda put: {"y": inf.resize_bilinear(put(x), (oh, ow))}, clean=True, tag="resize_bilinear")
    # the C oracle's resize (the TF 1.13 mapping of test_resize_bilinear_tf113_legacy_mapping), within that test's bound
    report_diff("resize_bilinear", got["y"], ico.resize_bilinear(x, oh, ow), exact=False, atol=1e-6)


def test_prelu_batch_norm_and_spatial_dropout():
    rng = np.random.default_rng(13)
    x = rng.normal(size=(2, 6, 5, 19)).astype(np.float32)
    a = rng.uniform(-0.5, 0.5, 19).astype(np.float32)
    m, v = rng.normal(0, 0.1, 19).astype(np.float32), rng.uniform(0.5, 1.5, 19).astype(np.float32)
    gm, b = rng.uniform(0.8, 1.2, 19).astype(np.float32), rng.normal(0, 0.1, 19).astype(np.float32)

    def body(put):
        return {"prelu": xops.prelu(put(x), put(a)),
                "bn": xops.batch_norm(put(x), put(m), put(v), put(gm), put(b), training=False)[0],
                "drop": xops.spatial_dropout(put(x + 3.0), 0.5, seed=77)}
    got = guarded(body, tag="prelu / batch_norm / dropout")
    report_diff("prelu", got["prelu"], orc.affine_prelu(x, None, None, a))
    s, t = orc.bn_fold(m, v, gm, b)
    report_diff("batch_norm", got["bn"], orc.affine_prelu(x, s, t, None))
    report_diff("spatial_dropout", got["drop"], dorc.spatial_dropout(x + 3.0, 0.5, seed=77))


@pytest.mark.parametrize("pixels", [1, 3, 4, 1027])
def test_label_lut(pixels):
    """``ssal_label_lut`` alone (test_label_lut_alone's smallest sizes): the 4-byte aligned route with its scalar tail and
    the byte route of an unaligned plane, without a table, with an id table and with a colour table"""
    rng = np.random.default_rng(pixels)
    buf = rng.integers(0, 32, pixels + 1).astype(np.uint8)
    ids = rng.integers(0, 256, 256).astype(np.uint8)
    rgb = rng.integers(0, 256, (256, 3)).astype(np.uint8)

    def body(put):
        L = _lib.lib()
        b, tables = put(buf), {0: None, 1: put(ids), 3: put(rgb)}
        out = {}
        for tag, label in (("aligned", b[:pixels]), ("unaligned", b[1:])):
            assert (label.data_ptr() % 4 == 0) == (tag == "aligned")
            for ch, lut in tables.items():
                y = torch.empty((pixels, 3) if ch == 3 else (pixels,), dtype=torch.uint8, device="cuda")
                _lib.check(L.ssal_label_lut(_lib.dev_ptr(label), pixels, _lib.dev_ptr(lut), ch, _lib.dev_ptr(y), _lib.stream_ptr()))
                out["%s ch=%d" % (tag, ch)] = y
        torch.cuda.synchronize()
        return out
    got = guarded(body, tag="label_lut")
    for tag, label in (("aligned", buf[:pixels]), ("unaligned", buf[1:])):
        report_diff(tag + " ids", got[tag + " ch=0"], label)
        report_diff(tag + " table", got[tag + " ch=1"], ids[label])
        report_diff(tag + " colours", got[tag + " ch=3"], rgb[label])


# ---- a stale workspace that is NOT re-poisoned -----------------------------------------------------------------------------
def _score_all(net, put, x, measure, fresh=lambda: None):
    """the ranking pass first (in the sequence it then follows the OTHER frames' calls), then the form with the maps"""
    fresh()
    only = net.score(put(x), measure)
    fresh()
    s, e = net.score(put(x), measure, return_label=True, return_confidence=True)
    return {"scores": s, "label": e["label"], "confidence": e["confidence"], "only": only}


@pytest.mark.parametrize("model", ["enet", "icnet"])
def test_score_sequence_on_one_stale_workspace(enet_c3k19, icnet19, model):
    """A (3x24x40 / 3x96x64), B (one small frame), C (other frames at A's size), A again on ONE model and stream, the
    workspace allocated once (for A, under the patch) and never poisoned again: each result equals the one computed on a
    fresh pattern-filled workspace"""
    net, _ = enet_c3k19 if model == "enet" else icnet19
    measure = "entropy" if model == "enet" else "margin"
    big, small = ((3, 24, 40), (1, 8, 8)) if model == "enet" else ((3, 96, 64), (1, 32, 32))
    seq = [("A", frames(range(20, 23), big[1], big[2], 3)), ("B", frames([50], small[1], small[2], 3)),
           ("C", frames(range(70, 73), big[1], big[2], 3)), ("A again", frames(range(20, 23), big[1], big[2], 3))]
    fresh = [guarded(lambda put, x=x: _score_all(net, put, x, measure, put.fresh), nets=(net,), tag="fresh " + nm) for nm, x in seq]
    for pattern in PATTERNS:
        with GuardedAlloc("cuda", pattern) as g:
            net._workspaces.clear()
            for (nm, x), want in zip(seq, fresh):
                got = _host(_score_all(net, g.guarded_from_numpy, x, measure))
                assert g.is_guarded(net._ws) and len(net._workspaces) == 1
                g.check()
                _same("%s %s on the stale workspace, pattern 0x%02X" % (model, nm, pattern), got, want)
        net._workspaces.clear()


# ---- trainers ------------------------------------------------------------------------------------------------------------------
AL_PARAMS = {"hyperparams": {"learning_rate": 0.0005, "learning_rate_decay": 0.0,
                             "optimizer": {"type": "Adam", "kwargs": {"beta1": 0.9, "beta2": 0.99}},
                             "weight_reg": {"L2": 0.0002, "L1": 0.0},
                             "softmax": {"label_smoothing": 0.0, "loginverse_scaling": 1.02, "multiscale": False}}}
ENET_TRAINERS = ["FinalLayerTrainer", "LastBlockTrainer", "LastStageTrainer", "DecoderTailTrainer", "DeepTailTrainer",
                 "DecoderTrainer"]
ICNET_TRAINERS = ["ICNetHeadTrainer", "ICNetFusionTrainer", "ICNetCascadeTrainer"]


def _new_net(kind):
    if kind == "enet":
        return make_model(19, 3, seed=0)[0]
    net = ssal.ICNet(19)
    net.build((None, None, None, 3))
    syn.randomize_icnet(net, seed=0)
    return net


def _train_planes(n, h, w, seed=9):
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, 19, (n, h, w)).astype(np.uint8)
    labels[rng.uniform(size=labels.shape) < 0.05] = 255
    return labels, (rng.uniform(size=(n, h, w)) > 0.2).astype(np.float32)


def _weights(tr, net):
    return {"~w:" + v.name: v.numpy().copy() for v in net.variables}


def _trained(tr):
    """{name: host copy} of the variables the trainer updates"""
    if hasattr(tr, "_named"):
        return {"~w:" + nm: var.numpy().copy() for nm, var, _, _ in tr._named()}
    names = tr.variable_names if hasattr(tr, "variable_names") else None
    if names is None:  # FinalLayerTrainer
        return {"~w:Final.kernel": tr.net.Final.kernel.numpy().copy()}
    out = {}
    for nm in names:
        layer, attr = nm.split(".")
        out["~w:" + nm] = getattr(getattr(tr.net, layer), attr).numpy().copy()
    return out


def _assign(net, values):
    for nm, v in values.items():
        layer, attr = nm.split(".")
        getattr(getattr(net, layer), attr).assign(v)


def _ragged_trainer_case(name):
    """the smallest ragged feature case of the trainer's own GPU test at K = 19 (its data, parameters and statistics):
    -> (make_net, feature arrays, labels, mask)"""
    k = 19
    if name == "FinalLayerTrainer":
        import test_gpu_train_final as t
        x, kern, labels, mask = t._case(101, 3, 20, 17, k)

        def make():
            net = ssal.ENet(k)
            net.build((None, None, None, 3))
            net.Final.kernel.assign(kern)
            return net
        return make, (x,), labels, mask
    if name == "LastBlockTrainer":
        import test_gpu_train_block as t
        x, labels, mask, params, stats = t._case(200, 1, 17, 23, k)
        return (lambda: t._net_with(k, params, stats)), (x,), labels, mask
    if name in ("LastStageTrainer", "DecoderTailTrainer", "DeepTailTrainer"):
        if name == "LastStageTrainer":
            import test_gpu_train_stage as t
            seed = t.SEEDS[0]
        elif name == "DecoderTailTrainer":
            import test_gpu_train_tail as t
            seed = t.SEEDS[((1, 9, 12), k)]
        else:
            import test_gpu_train_deep_tail as t
            seed = t.SEEDS[((1, 9, 12), k)]
        x, am, labels, mask, params, stats = t._case(seed, 1, 9, 12, k)
        return (lambda: t._net_with(k, params, stats)), (x, am), labels, mask
    if name == "DecoderTrainer":
        import test_gpu_train_decoder as t
        x, am2, am1, labels, mask, params, stats = t._case(t.SEEDS[((1, 5, 6), k)], 1, 5, 6, k)
        return (lambda: t._net_with(k, params, stats)), (x, am2, am1), labels, mask
    if name == "ICNetHeadTrainer":
        import test_gpu_train_icnet_head as t
        x, head, labels, mask = t._case(1000, 2, 3, 5, k)

        def make():
            net = t._net(k)
            _assign(net, t._params(head, k))
            return net
        return make, (x,), labels, mask
    import test_gpu_train_icnet_cascade as tc
    import test_gpu_train_icnet_fusion as tf
    t = tf if name == "ICNetFusionTrainer" else tc
    *feats, d, labels, mask = t._case(2000, 1, 3, 5, k)

    def make():
        net = t._net(k)
        _assign(net, d)
        rng = np.random.default_rng(77)
        _assign(net, {nm: (rng.uniform(0.5, 2.0, 128) if nm.endswith("variance") else rng.uniform(-0.3, 0.3, 128)).astype(np.float32)
                      for nm in t.STAT_NAMES})
        return net
    return make, tuple(feats), labels, mask


def _grad_dict(grads):
    return grads if isinstance(grads, dict) else {"Final.kernel": grads}


@pytest.mark.parametrize("name", ENET_TRAINERS + ICNET_TRAINERS)
def test_trainer_on_its_smallest_ragged_feature_case(name):
    """``gradient_features`` and one ``step_features`` at the trainer's smallest ragged feature case (no tile of the
    head-gradient and backward kernels is whole), each call on allocations of its own: the loss, every gradient and the
    updated weights.  The feature entries allocate their workspace themselves (training.py), so the loss and the gradients
    must be interiors of guarded slabs; the model's own workspace is not used"""
    make, feats, labels, mask = _ragged_trainer_case(name)
    cls = getattr(training, name)

    def body(put):
        net = put.adopt(make())
        tr = cls(net, 1e-3, loginverse_scaling=1.02, label_smoothing=0.1)
        put.fresh()
        loss, grads = tr.gradient_features(*[put(f) for f in feats], put(labels), put(mask))
        out = {"loss": loss}
        out.update({"g:" + k: v for k, v in _grad_dict(grads).items()})
        put.fresh()
        out["~step_loss"] = tr.step_features(*[put(f) for f in feats], put(labels), put(mask))
        torch.cuda.synchronize()
        out.update(_trained(tr))
        return out
    got = guarded(body, clean=True, tag=name + " ragged")
    assert np.isfinite(got["loss"]).all() and same_bits(got["loss"].ravel()[:1], got["step_loss"].ravel()[:1])
    assert any(np.abs(v).max() > 0 for k, v in got.items() if k.startswith("g:"))
    assert all(np.isfinite(v).all() for k, v in got.items() if k.startswith("g:") or k.startswith("w:"))


@pytest.mark.parametrize("name", ENET_TRAINERS + ICNET_TRAINERS)
def test_trainer_from_the_features_of_frames(name):
    """``features(images)`` (the frozen trunk on the model's workspace), ``gradient_features`` and one ``step_features`` on
    2 x 64 x 128 frames, a fresh model per run: its workspace must come from the patch"""
    kind = "enet" if name in ENET_TRAINERS else "icnet"
    x = frames([0, 1], 64, 128, 3)
    labels, mask = _train_planes(2, 64, 128)

    def body(put):
        net = put.adopt(_new_net(kind))
        tr = getattr(training, name).from_params(net, AL_PARAMS)
        put.fresh()
        if name == "FinalLayerTrainer":
            net(put(x), training=False)
            feats = (net.endpoint_outputs[0][1].clone(),)
        else:
            feats = tr.features(put(x))
            feats = feats if isinstance(feats, tuple) else (feats,)
        assert put.g is None or put.g.is_guarded(net._ws), "%s: the trunk's workspace did not come from the patch" % name
        put.fresh()
        loss, grads = tr.gradient_features(*feats, put(labels), put(mask))
        out = {"loss": loss}
        out.update({"g:" + k: v for k, v in _grad_dict(grads).items()})
        put.fresh()
        out["~step_loss"] = tr.step_features(*feats, put(labels), put(mask))
        torch.cuda.synchronize()
        out.update(_trained(tr))
        return out
    got = guarded(body, clean=True, tag=name)
    assert np.isfinite(got["loss"]).all() and same_bits(got["loss"].ravel()[:1], got["step_loss"].ravel()[:1])
    assert any(np.abs(v).max() > 0 for k, v in got.items() if k.startswith("g:"))


@pytest.mark.parametrize("name", ["SemiSupervisedDecoderTrainer", "SemiSupervisedICNetCascadeTrainer"])
def test_semi_supervised_step_from_images(name):
    """one ``step`` with ``images_raw``, ``confusion=`` and ``return_pseudo_pixels=True``; image 1 is unlabelled (0xFF labels,
    NaN mask): the head kernels write and read pseudo-target byte planes in shared workspace slots of the model's workspace"""
    kind = "enet" if "ICNet" not in name else "icnet"
    measure = "entropy" if kind == "enet" else "margin"
    x_raw = frames([0, 1], 64, 128, 3)
    x = np.ascontiguousarray(x_raw * np.array([0.9, 1.1, 0.8], np.float32))
    labels, mask = _train_planes(2, 64, 128)
    labels[1], mask[1] = 0xFF, np.nan
    probe = _new_net(kind)
    _, p = probe.score(_plain(x_raw), measure, 0.0, return_confidence=True)
    thr = float(np.median(p["confidence"][1].cpu().numpy()))

    def body(put):
        net = put.adopt(_new_net(kind))
        tr = getattr(training, name).from_params(net, AL_PARAMS)
        conf = torch.zeros((19, 19), dtype=torch.int64, device="cuda")
        sel = torch.tensor([True, False]).cuda()
        put.fresh()
        loss, pp = tr.step(put(x), put(labels), put(mask), labelled=sel, measure=measure, threshold=thr, confusion=conf,
                           images_raw=put(x_raw), return_pseudo_pixels=True)
        assert put.g is None or put.g.is_guarded(net._ws), "%s: the step's workspace did not come from the patch" % name
        out = {"loss": loss, "pseudo_pixels": pp, "~confusion": conf, "grad": tr._dev["grad"]}
        torch.cuda.synchronize()
        out.update(_trained(tr))
        return out
    got = guarded(body, clean=True, tag=name)
    assert np.isfinite(got["loss"]).all() and got["pseudo_pixels"][0] == 0 and 0 < got["pseudo_pixels"][1] < 64 * 128
    assert got["confusion"].sum() > 0 and np.isfinite(got["grad"]).all()


def test_decoder_trainer_step_sequence_on_one_stale_workspace():
    """``DecoderTrainer.step`` on two label sets of one shape, one model, the workspace allocated once under the patch: every
    loss and the final weights equal those of a run outside the harness"""
    x = frames([0, 1], 64, 128, 3)
    sets = [_train_planes(2, 64, 128, seed=9), _train_planes(2, 64, 128, seed=10)]

    def run(put):
        net = _new_net("enet")
        tr = training.DecoderTrainer.from_params(net, AL_PARAMS)
        out = {}
        for i, (labels, mask) in enumerate(sets + sets[:1]):
            out["~loss%d" % i] = tr.step(put(x), put(labels), put(mask)).clone()
        torch.cuda.synchronize()
        out.update(_weights(tr, net))
        return net, out
    _, want = run(_plain)
    want = _host(want)
    for pattern in PATTERNS:
        with GuardedAlloc("cuda", pattern) as g:
            net, got = run(g.guarded_from_numpy)
            assert g.count > 0 and g.is_guarded(net._ws) and len(net._workspaces) == 1
            g.check()
            _same("DecoderTrainer.step sequence, pattern 0x%02X" % pattern, _host(got), want)


# ---- PNG decode --------------------------------------------------------------------------------------------------------------
def test_png_decode_batch_on_the_mixed_size_corpus():
    import test_gpu_png as tpng
    from png_corpus import pillow_decode, png_corpus
    corpus = [d for _, d in png_corpus()]
    want = [pillow_decode(d) for d in corpus]
    oh, ow = min(w.shape[0] for w in want), min(w.shape[1] for w in want)  # as test_batch_decode_matches_pillow_mixed_sizes
    rng = np.random.default_rng(0)
    tops = [int(rng.integers(0, w.shape[0] - oh + 1)) for w in want]
    lefts = [int(rng.integers(0, w.shape[1] - ow + 1)) for w in want]
    outs = []
    for pattern in PATTERNS:
        with GuardedAlloc("cuda", pattern) as g:
            st, got, _ = tpng._decode_batch(corpus, oh, ow, tops, lefts)
            assert g.count > 0
            g.check()
            outs.append({"status": np.asarray(st), "frames": np.asarray(got)})
    for o in outs[1:]:
        _same("png decode across patterns", o, outs[0])
    st, got = outs[0]["status"], outs[0]["frames"]
    assert (st == 0).all(), st
    for f, w in enumerate(want):
        c = w.shape[2]
        assert np.array_equal(got[f, :, :, :c], w[tops[f]:tops[f] + oh, lefts[f]:lefts[f] + ow]), "frame %d != Pillow" % f
        assert (got[f, :, :, c:] == 7).all()  # channels past the stream's own are untouched
