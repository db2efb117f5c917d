"""The semi-supervised step of ICNet's fusion and cascade trainers on the MI355X: pseudo annotation and
training metrics inside k_icnet_head_grad<K, true, true>, against the COMPOSITION of code sections 25, 28 and 29 already pin to
their oracles -- the forward path's full-resolution logits under the weights being trained, score_logits with label / mask /
confidence planes, training_targets, the parent trainer's plain gradient / step, the stand-alone confusion op.  The
interpolated logits, pixel_score and everything behind dL/dlogit are the same code on both routes, so the loss and all 8 / 14
gradients are compared bit for bit and the counts exactly."""
import numpy as np
import pytest
import torch

import semanticsegmentationactivelearning_amd as ssal
from semanticsegmentationactivelearning_amd import active_learning as al
from semanticsegmentationactivelearning_amd import inference
from semanticsegmentationactivelearning_amd import synthetic as syn
from semanticsegmentationactivelearning_amd.models.util import conv_ops as cops
from semanticsegmentationactivelearning_amd.tensortools import metrics
from semanticsegmentationactivelearning_amd.training import (ICNetCascadeTrainer, ICNetFusionTrainer,
                                                             SemiSupervisedICNetCascadeTrainer,
                                                             SemiSupervisedICNetFusionTrainer)

pytestmark = pytest.mark.gpu

MEASURES = ("entropy", "margin", "confidence")
KS = (2, 6, 19, 32)
WL = ((0.0, 0.0), (1.02, 0.1))
KINDS = ("fusion", "cascade")
PLAIN = {"fusion": ICNetFusionTrainer, "cascade": ICNetCascadeTrainer}
SEMI = {"fusion": SemiSupervisedICNetFusionTrainer, "cascade": SemiSupervisedICNetCascadeTrainer}
UP = {"fusion": 16, "cascade": 32}  # loss pixels per pixel of the first feature map and axis
BLOCKS = {"fusion": ("conv_sub2", "conv3_sub1_proj"), "cascade": ("conv_sub4", "conv3_1_sub2_proj", "conv_sub2", "conv3_sub1_proj")}
_NETS = {}


def _var(net, name):
    layer, attr = name.split(".")
    return getattr(getattr(net, layer), attr)


def _net(k):
    net = ssal.ICNet(k)
    net.build((None, None, None, 3))
    return net


def _shared_net(k):
    """one model per class count for the gradient cases (they pass the weights as ``params`` and change nothing); its moving
    statistics are drawn once"""
    if k not in _NETS:
        net = _net(k)
        rng = np.random.default_rng(277 + k)
        for layer in BLOCKS["cascade"]:
            _var(net, layer + ".mean").assign(rng.uniform(-0.3, 0.3, 128).astype(np.float32))
            _var(net, layer + ".variance").assign(rng.uniform(0.5, 2.0, 128).astype(np.float32))
        _NETS[k] = net
    return _NETS[k]


def _names(kind):
    return PLAIN[kind].variable_names


def _case(kind, seed, n, h, w, k, labelled):
    """features, the trained variables and the annotation.  The planes of unlabelled images hold 0xFF labels and NaN masks
    (never read); the first labelled image carries label 255 under mask 1 on a few pixels (key >= K^2: dropped from the
    confusion matrix) and a mask value of 2.0 on a few (adds 2)."""
    rng = np.random.default_rng(seed)
    if kind == "fusion":
        feats = [rng.standard_normal((n, h, w, 128)), rng.standard_normal((n, 2 * h, 2 * w, 64))]
    else:
        feats = [rng.standard_normal((n, h, w, 256)), rng.standard_normal((n, 2 * h, 2 * w, 256)),
                 rng.standard_normal((n, 4 * h, 4 * w, 64))]
    feats = tuple(torch.as_tensor((f * 0.7).astype(np.float32)).cuda() for f in feats)
    d = {}
    if kind == "cascade":
        d.update({"conv_sub4.kernel": rng.uniform(-0.03, 0.03, (3, 3, 256, 128)), "conv_sub4.gamma": rng.uniform(0.5, 1.5, 128),
                  "conv_sub4.beta": rng.uniform(-0.3, 0.3, 128),
                  "conv3_1_sub2_proj.kernel": rng.uniform(-0.08, 0.08, (1, 1, 256, 128)),
                  "conv3_1_sub2_proj.gamma": rng.uniform(-1.5, 1.5, 128), "conv3_1_sub2_proj.beta": rng.uniform(-0.3, 0.3, 128)})
    d.update({"conv_sub2.kernel": rng.uniform(-0.04, 0.04, (3, 3, 128, 128)), "conv_sub2.gamma": rng.uniform(0.5, 1.5, 128),
              "conv_sub2.beta": rng.uniform(-0.3, 0.3, 128), "conv3_sub1_proj.kernel": rng.uniform(-0.15, 0.15, (1, 1, 64, 128)),
              "conv3_sub1_proj.gamma": rng.uniform(-1.5, 1.5, 128), "conv3_sub1_proj.beta": rng.uniform(-0.3, 0.3, 128),
              "conv6_cls.kernel": rng.uniform(-0.3, 0.3, (1, 1, 128, k)), "conv6_cls.bias": rng.uniform(-0.5, 0.5, k)})
    d = {name: v.astype(np.float32) for name, v in d.items()}
    up = UP[kind]
    labels = rng.integers(0, k, (n, up * h, up * w)).astype(np.uint8)
    mask = (rng.uniform(size=labels.shape) > 0.25).astype(np.float32)
    first = True
    for i, l in enumerate(labelled):
        if not l:
            labels[i], mask[i] = 0xFF, np.nan
        elif first:
            first = False
            labels[i, 0, :3], mask[i, 0, :3] = 255, 1.0
            labels[i, -1, -3:] = np.arange(3) % k
            mask[i, -1, -3:] = 2.0
    return feats, d, torch.as_tensor(labels).cuda(), torch.as_tensor(mask).cuda()


def _logits(kind, net, feats, d):
    """the full-resolution logits of the forward path under the variables ``d``: its own fused launches, then its 4x resize"""
    bn = lambda layer: (_var(net, layer + ".mean").numpy(), _var(net, layer + ".variance").numpy(), d[layer + ".gamma"],
                        d[layer + ".beta"])
    if kind == "cascade":
        p24 = cops.conv_bn_act(feats[1], d["conv3_1_sub2_proj.kernel"], bn=bn("conv3_1_sub2_proj"), relu=False)
        sub24 = cops.conv_bn_act(feats[0], d["conv_sub4.kernel"], dilation=2, bn=bn("conv_sub4"), residual=p24, relu=True,
                                 upsample2x=True)
    else:
        sub24 = feats[0]
    proj = cops.conv_bn_act(feats[-1], d["conv3_sub1_proj.kernel"], bn=bn("conv3_sub1_proj"), relu=False)
    sub12 = cops.conv_bn_act(sub24, d["conv_sub2.kernel"], dilation=2, bn=bn("conv_sub2"), residual=proj, relu=True,
                             upsample2x=True)
    lq = cops.conv_bn_act(sub12, d["conv6_cls.kernel"], bias=d["conv6_cls.bias"], relu=False, upsample2x=True)
    return inference.resize_bilinear(lq, (4 * lq.shape[1], 4 * lq.shape[2]))


def _other(feats, lo, hi):
    """features that differ from ``feats``: every channel scaled by its own factor"""
    return tuple((f * torch.linspace(lo, hi, f.shape[-1], device="cuda")).contiguous() for f in feats)


def _pack(kind, gd):
    return torch.cat([gd[n].reshape(-1) for n in _names(kind)])


def _sel(labelled, n):
    return torch.ones(n, dtype=torch.bool, device="cuda") if labelled is None else torch.as_tensor(
        np.asarray(labelled, dtype=bool)).cuda()


def _median_threshold(kind, net, feats_raw, d, measure, labelled):
    """the median of the yardstick's confidence over the unlabelled pixels"""
    _, p = al.score_logits(_logits(kind, net, feats_raw, d), measure, 0.0, return_confidence=True)
    sel = _sel(labelled, feats_raw[0].shape[0])
    return float(np.median(p["confidence"][~sel].cpu().numpy()))


def _composed(kind, net, tr, feats, feats_raw, d, labels, mask, labelled, measure, threshold, mw=0):
    """(loss, packed gradient, confusion, pseudo pixels, confidence plane, mask trained on) of the composed step"""
    n, h, w, _ = feats[0].shape
    k, up = net.classes, UP[kind]
    sel = _sel(labelled, n)
    _, p = al.score_logits(_logits(kind, net, feats_raw, d), measure, threshold, return_label=True, return_mask=True,
                           return_confidence=True)
    if labels is None:
        labels = torch.zeros((n, up * h, up * w), dtype=torch.uint8, device="cuda")
        mask = torch.zeros((n, up * h, up * w), dtype=torch.float32, device="cuda")
    lab, mk = al.training_targets(sel, labels, mask, p["label"], p["mask"].float())
    loss, gd = tr.gradient_features(*feats, lab, mk, params=d, max_workgroups=mw)
    _, pt = al.score_logits(_logits(kind, net, feats, d), "confidence", 0.0, return_label=True)  # the first maximum
    conf = metrics.confusion_mat(lab, pt["label"], k, weights=mk)
    pp = p["mask"].to(torch.int64).sum(dim=(1, 2)) * (~sel).to(torch.int64)
    return loss, _pack(kind, gd), conf, pp, p["confidence"], mk


def _fused(kind, net, tr, feats, feats_raw, d, labels, mask, labelled, measure, threshold, mw=0):
    k = net.classes
    conf = torch.zeros((k, k), dtype=torch.int64, device="cuda")
    loss, gd, pp = tr.gradient_features(*feats, labels, mask, params=d, max_workgroups=mw, labelled=labelled, measure=measure,
                                        threshold=threshold, features_raw=feats_raw, confusion=conf, return_pseudo_pixels=True)
    return loss, _pack(kind, gd), conf, pp


def _assert_same(name, got, want):
    loss, grad, conf, pp = got[:4]
    wloss, wgrad, wconf, wpp = want[:4]
    print("%s: loss %.17g / %.17g, confusion sum %d / %d, pseudo pixels %s / %s"
          % (name, float(loss[0]), float(wloss[0]), int(conf.sum()), int(wconf.sum()), pp.tolist(), wpp.tolist()))
    assert torch.equal(loss, wloss), "%s: loss %r != %r" % (name, float(loss[0]), float(wloss[0]))
    assert torch.equal(grad.view(torch.int32), wgrad.view(torch.int32)), "%s: %d of %d gradient entries differ" % (
        name, int((grad.view(torch.int32) != wgrad.view(torch.int32)).sum()), grad.numel())
    assert torch.equal(conf, wconf), "%s: confusion differs in %d entries" % (name, int((conf != wconf).sum()))
    assert torch.equal(pp, wpp), "%s: pseudo pixels %s != %s" % (name, pp.tolist(), wpp.tolist())


def _assert_mixed_masks(name, want, labelled, n, threshold):
    """0.3 - 0.7 of the unlabelled pixels pass the threshold; at least 0.05 of the labelled pixels carry mask 0"""
    sel = _sel(labelled, n)
    if bool((~sel).any()):
        share = float((want[4][~sel] >= threshold).float().mean())
        print("%s: threshold %.9g lets %.3f of the unlabelled pixels pass" % (name, threshold, share))
        assert 0.3 <= share <= 0.7, name + ": the threshold does not give a mixed pseudo mask"
    if bool(sel.any()):
        zeros = float((want[5][sel] == 0).float().mean())
        print("%s: %.3f of the labelled pixels carry mask 0" % (name, zeros))
        assert zeros >= 0.05, name + ": the labelled images have no masked-out pixels"


def _trainers(kind, k, wl):
    net = _shared_net(k)
    return net, PLAIN[kind](net, 1e-3, loginverse_scaling=wl[0], label_smoothing=wl[1]), SEMI[kind](
        net, 1e-3, loginverse_scaling=wl[0], label_smoothing=wl[1])


def _run_case(kind, name, seed, shape, k, measure, labelled, wl, mw=0, no_planes=False):
    n, h, w = shape
    marks = [1] * n if labelled is None else labelled
    feats, d, labels, mask = _case(kind, seed, n, h, w, k, marks)
    net, tr0, tr1 = _trainers(kind, k, wl)
    thr = _median_threshold(kind, net, feats, d, measure, labelled) if (labelled is not None and not all(labelled)) else 0.5
    if no_planes:
        labels = mask = None
    want = _composed(kind, net, tr0, feats, feats, d, labels, mask, labelled, measure, thr, mw)
    got = _fused(kind, net, tr1, feats, None, d, labels, mask, labelled, measure, thr, mw)
    _assert_mixed_masks(name, want, labelled, n, thr)
    _assert_same(name, got, want)
    return got, want


# `labelled` of the main sweep on 2 x 2 x 3: not given (confusion only), all labelled, mixed, all unlabelled (no planes)
PATTERNS = (("not given", None, False), ("all", [1, 1], False), ("mixed", [1, 0], False), ("none", [0, 0], True))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("kind", KINDS)
def test_main_sweep_matches_composition(kind, k, measure):
    """2 x 2 x 3 (N x h16 x w16 for the fusion, N x h32 x w32 for the cascade trainer: several tiles of every kernel, two
    images): bitwise loss and gradients, equal confusion matrix and pseudo-pixel counts; (weight, label smoothing) alternates
    over the cases; the seed is a fixed function of the case"""
    base = 4 * (len(MEASURES) * KS.index(k) + MEASURES.index(measure))
    pixels = UP[kind] ** 2 * 6
    for j, (pname, labelled, no_planes) in enumerate(PATTERNS):
        case = base + j
        name = "%s K=%d %s labelled=%s w=%g ls=%g" % ((kind, k, measure, pname) + WL[case % 2])
        got, _ = _run_case(kind, name, 17000 + 100 * KINDS.index(kind) + case, (2, 2, 3), k, measure, labelled, WL[case % 2],
                           no_planes=no_planes)
        if labelled is None or all(labelled):
            assert got[3].tolist() == [0, 0]
        if pname == "mixed":
            assert got[3][0].item() == 0 and 0 < got[3][1].item() < pixels


# the other shapes sections 28 and 29 found small enough to still break the tiling (N x h x w of the first feature map,
# max_workgroups), K = 19; a batch of one image has no mixed `labelled`: it runs unlabelled (the side the new code is on) and
# labelled (the confusion keys)
OTHER = [("fusion", (1, 1, 1), 0), ("fusion", (1, 3, 5), 1), ("fusion", (1, 3, 5), 2),
         ("cascade", (1, 1, 1), 0), ("cascade", (1, 3, 2), 1), ("cascade", (1, 3, 2), 2)]


@pytest.mark.parametrize("kind,shape,mw", OTHER)
@pytest.mark.parametrize("labelled", [[0], [1]])
def test_other_shapes_match_composition(kind, shape, mw, labelled):
    case = 2 * OTHER.index((kind, shape, mw)) + labelled[0]
    measure = MEASURES[case % 3]
    name = "%s %s mw=%d labelled=%s %s" % (kind, shape, mw, labelled, measure)
    got, _ = _run_case(kind, name, 18000 + case, shape, 19, measure, labelled, WL[case % 2], mw)
    if labelled[0]:
        assert got[3][0].item() == 0 and int(got[2].sum()) > 0
    else:
        assert 0 < got[3][0].item() < UP[kind] ** 2 * shape[1] * shape[2]


def _class_count_seed(kind, k, draw=None):
    return 19300 + 100 * KINDS.index(kind) + k + 1000 * (RESEED.get((kind, k), 0) if draw is None else draw)


# On a 1 x 1 map the clamped taps of the two resizes make a quarter of an image's 256 / 1024 logits one constant vector, so a
# quarter of its confidences is one value; where that value is the median, the median lets up to 0.75 of the pixels pass.  The
# seed is a condition on the YARDSTICK alone: (kind, K) -> the first draw (seed + 1000 draw) at which its confidence planes
# give 0.3 - 0.7 with and without the raw side; every other class count keeps draw 0.
RESEED = {("fusion", 16): 1, ("fusion", 29): 1}


@pytest.mark.parametrize("kind", KINDS)
def test_every_class_count_with_and_without_a_raw_side(kind):
    """all 31 instantiations of k_icnet_head_grad<K, true, true>, as the training launch on its own logits and behind the
    target-only launch whose plane it reads, on two images of the smallest feature map with mixed `labelled` (the measure
    cycles with K)"""
    for k in range(2, 33):
        measure, wl, labelled = MEASURES[k % 3], WL[k % 2], [k % 2, 1 - k % 2]
        feats, d, labels, mask = _case(kind, _class_count_seed(kind, k), 2, 1, 1, k, labelled)
        feats_raw = _other(feats, 1.2, 0.85)
        net, tr0, tr1 = _trainers(kind, k, wl)
        for raw in (None, feats_raw):
            name = "%s K=%d %s raw=%s" % (kind, k, measure, raw is not None)
            src = feats if raw is None else raw
            thr = _median_threshold(kind, net, src, d, measure, labelled)
            want = _composed(kind, net, tr0, feats, src, d, labels, mask, labelled, measure, thr)
            _assert_mixed_masks(name, want, labelled, 2, thr)
            _assert_same(name, _fused(kind, net, tr1, feats, raw, d, labels, mask, labelled, measure, thr), want)


@pytest.mark.parametrize("kind", KINDS)
def test_threshold_between_two_images(kind):
    """3 x 1 x 1 with features constant over every image and conv_sub2 reduced to its centre tap (on these maps every
    off-centre tap of the first dilated convolution is padding anyway): an image's logits are constant, so all its pixels
    share one confidence.  Images 0 and 2 are unlabelled, the threshold is the mean of their two confidences: one image passes
    whole, the other fails whole."""
    k, labelled, measure = 19, [0, 1, 0], "entropy"
    feats, d, labels, mask = _case(kind, 19000 + KINDS.index(kind), 3, 1, 1, k, labelled)
    feats = tuple(f[:, :1, :1, :].expand_as(f).contiguous() for f in feats)
    centre = d["conv_sub2.kernel"][1, 1].copy()
    d["conv_sub2.kernel"][:] = 0.0
    d["conv_sub2.kernel"][1, 1] = centre
    net, tr0, tr1 = _trainers(kind, k, WL[1])
    _, p = al.score_logits(_logits(kind, net, feats, d), measure, 0.0, return_confidence=True)
    c = p["confidence"].cpu().numpy().astype(np.float64)
    assert c[0].min() == c[0].max() and c[2].min() == c[2].max() and c[0, 0, 0] != c[2, 0, 0]
    thr = 0.5 * (c[0, 0, 0] + c[2, 0, 0])
    want = _composed(kind, net, tr0, feats, feats, d, labels, mask, labelled, measure, thr)
    got = _fused(kind, net, tr1, feats, None, d, labels, mask, labelled, measure, thr)
    _assert_same("3x1x1 " + kind, got, want)
    assert sorted(got[3].tolist()) == [0, 0, UP[kind] ** 2] and got[3][1].item() == 0


def _host(kind, net):
    return np.concatenate([_var(net, n).numpy().reshape(-1) for n in _names(kind)])


def _flat_state(kind, tr):
    st = tr.state
    return [np.concatenate([st[s][n].reshape(-1) for n in _names(kind)]) for s in ("m", "v")]


HYPER = dict(learning_rate=5e-4, beta1=0.9, beta2=0.99, loginverse_scaling=1.02, label_smoothing=0.1, l2=2e-4)


@pytest.mark.parametrize("kind", KINDS)
def test_raw_features_differ_from_training_features(kind):
    """the pseudo annotation comes from features_raw, the gradient from the training features: gradient_features against the
    composition, then step_features against the composed plain step"""
    k, labelled, measure = 19, [0, 1], MEASURES[KINDS.index(kind) + 1]
    feats_raw, d, labels, mask = _case(kind, 19100 + KINDS.index(kind), 2, 2, 3, k, labelled)
    feats = _other(feats_raw, 0.8, 1.25)
    net, tr0, tr1 = _trainers(kind, k, WL[1])
    thr = _median_threshold(kind, net, feats_raw, d, measure, labelled)
    want = _composed(kind, net, tr0, feats, feats_raw, d, labels, mask, labelled, measure, thr)
    got = _fused(kind, net, tr1, feats, feats_raw, d, labels, mask, labelled, measure, thr)
    _assert_mixed_masks("features_raw " + kind, want, labelled, 2, thr)
    _assert_same("features_raw " + kind, got, want)
    one_pass = _fused(kind, net, tr1, feats, None, d, labels, mask, labelled, measure, thr)
    assert not torch.equal(one_pass[1], got[1]), "the raw features made no difference: the case shows nothing"
    _assert_same("features_raw is features", _fused(kind, net, tr1, feats, feats, d, labels, mask, labelled, measure, thr),
                 one_pass)
    _assert_same("features_raw == features (copies: the target launch)",
                 _fused(kind, net, tr1, feats, tuple(f.clone() for f in feats), d, labels, mask, labelled, measure, thr),
                 one_pass)
    # step_features: twin models under the same variables and statistics
    net_a, net_b = _net(k), _net(k)
    for twin in (net_a, net_b):
        for layer in BLOCKS["cascade"]:
            for attr in ("mean", "variance"):
                _var(twin, "%s.%s" % (layer, attr)).assign(_var(net, "%s.%s" % (layer, attr)).numpy())
        for name, v in d.items():
            _var(twin, name).assign(v)
    tr_a, tr_b = SEMI[kind](net_a, **HYPER), PLAIN[kind](net_b, **HYPER)
    conf_a = torch.zeros((k, k), dtype=torch.int64, device="cuda")
    la, ppa = tr_a.step_features(*feats, labels, mask, labelled=labelled, measure=measure, threshold=thr,
                                 features_raw=feats_raw, confusion=conf_a, return_pseudo_pixels=True)
    sel = _sel(labelled, 2)
    _, p = al.score_logits(_logits(kind, net, feats_raw, d), measure, thr, return_label=True, return_mask=True)
    lab, mk = al.training_targets(sel, labels, mask, p["label"], p["mask"].float())
    lb = tr_b.step_features(*feats, lab, mk)
    assert float(la).hex() == float(lb).hex()
    assert np.array_equal(_host(kind, net_a), _host(kind, net_b))
    assert all(np.array_equal(a, b) for a, b in zip(_flat_state(kind, tr_a), _flat_state(kind, tr_b)))
    assert torch.equal(conf_a, want[2]) and torch.equal(ppa, want[3])


@pytest.fixture(scope="module")
def icnet19():
    net = _net(19)
    syn.randomize_icnet(net, seed=0)
    return net


def _twin(net0):
    net = _net(19)
    net.assign_named({v.name: v.numpy() for v in net0.variables})
    return net


def _frames_case(u8=False):
    """2 x 64 x 128 frames, image 1 unlabelled; the training frames are the undistorted ones with the channels reversed"""
    x_raw = syn.synth_frames_device(3, 2, 64, 128, 3, dtype=torch.uint8 if u8 else None)
    x = x_raw.flip(-1).contiguous()
    rng = np.random.default_rng(21)
    labels = rng.integers(0, 19, (2, 64, 128)).astype(np.uint8)
    mask = (rng.uniform(size=(2, 64, 128)) > 0.2).astype(np.float32)
    labels[1], mask[1] = 0xFF, np.nan
    return x, x_raw, torch.as_tensor(labels).cuda(), torch.as_tensor(mask).cuda(), torch.tensor([True, False]).cuda()


def _composed_step(net, tr, x, x_raw, labels, mask, sel, measure, thr, conf):
    """net(x_raw) -> score_logits -> training_targets -> the plain step (+ the stand-alone confusion op on net(x))"""
    _, p = al.score_logits(net(x_raw, training=False), measure, thr, return_label=True, return_mask=True)
    lab, mk = al.training_targets(sel, labels, mask, p["label"], p["mask"].float())
    _, pt = al.score_logits(net(x, training=False), "confidence", 0.0, return_label=True)
    metrics.confusion_mat(lab, pt["label"], net.classes, weights=mk, out=conf)
    pp = p["mask"].to(torch.int64).sum(dim=(1, 2)) * (~sel).to(torch.int64)
    return tr.step(x, lab, mk), pp


def _frame_threshold(net, x_raw, measure):
    _, p = al.score_logits(net(x_raw, training=False), measure, 0.0, return_confidence=True)
    return float(np.median(p["confidence"][1].cpu().numpy()))


@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_images_raw_equals_features_raw_and_composition(icnet19, kind, u8):
    """step(images, images_raw=...) == step_features(*features(images), features_raw=features(images_raw)) bit for bit, and both
    equal the composed step; images_raw is images == no raw side"""
    x, x_raw, labels, mask, sel = _frames_case(u8)
    nets = [_twin(icnet19) for _ in range(3)]
    tr_a, tr_b = (SEMI[kind](n, **HYPER) for n in nets[:2])
    tr_c = PLAIN[kind](nets[2], **HYPER)
    for tr in (tr_a, tr_b, tr_c):
        tr.reinitialize(seed=4)
    thr = _frame_threshold(nets[2], x_raw, "margin")
    feats, feats_raw = tr_b.features(x), tr_b.features(x_raw)
    assert not any(torch.equal(a, b) for a, b in zip(feats, feats_raw))
    conf = [torch.zeros((19, 19), dtype=torch.int64, device="cuda") for _ in range(3)]
    for step in range(2):
        la, ppa = tr_a.step(x, labels, mask, labelled=sel, measure="margin", threshold=thr, images_raw=x_raw,
                            confusion=conf[0], return_pseudo_pixels=True)
        lb, ppb = tr_b.step_features(*feats, labels, mask, labelled=sel, measure="margin", threshold=thr,
                                     features_raw=feats_raw, confusion=conf[1], return_pseudo_pixels=True)
        lc, ppc = _composed_step(nets[2], tr_c, x, x_raw, labels, mask, sel, "margin", thr, conf[2])
        print("%s step %d: loss %.17g / %.17g / %.17g, pseudo pixels %s"
              % (kind, step, float(la), float(lb), float(lc), ppa.tolist()))
        assert float(la).hex() == float(lb).hex() == float(lc).hex(), "loss differs at step %d" % step
        for other in nets[1:]:
            assert np.array_equal(_host(kind, nets[0]), _host(kind, other)), "weights differ at step %d" % step
        assert torch.equal(ppa, ppb) and torch.equal(ppa, ppc) and ppa[0].item() == 0 and 0 < ppa[1].item() < 64 * 128
        assert torch.equal(conf[0], conf[1]) and torch.equal(conf[0], conf[2])
    net_d, net_e = _twin(icnet19), _twin(icnet19)
    tr_d, tr_e = SEMI[kind](net_d, **HYPER), SEMI[kind](net_e, **HYPER)
    ld = tr_d.step(x, labels, mask, labelled=sel, threshold=0.3, images_raw=x)
    le = tr_e.step(x, labels, mask, labelled=sel, threshold=0.3)
    assert float(ld).hex() == float(le).hex() and np.array_equal(_host(kind, net_d), _host(kind, net_e))


@pytest.mark.parametrize("kind", KINDS)
def test_twin_nets_five_steps(icnet19, kind):
    """five fused steps on one net, five composed steps on its twin (mixed `labelled`, images_raw given): all trained tensors,
    m, v, loss, confusion and pseudo pixels equal after every step"""
    x, x_raw, labels, mask, sel = _frames_case()
    net_a, net_b = _twin(icnet19), _twin(icnet19)
    tr_a, tr_b = SEMI[kind](net_a, **HYPER), PLAIN[kind](net_b, **HYPER)
    tr_a.reinitialize(seed=5)
    tr_b.reinitialize(seed=5)
    thr = _frame_threshold(net_b, x_raw, "entropy")
    conf_a = torch.zeros((19, 19), dtype=torch.int64, device="cuda")
    conf_b = torch.zeros_like(conf_a)
    start = _host(kind, net_a)
    for step in range(5):
        la, ppa = tr_a.step(x, labels, mask, labelled=sel, measure="entropy", threshold=thr, images_raw=x_raw,
                            confusion=conf_a, return_pseudo_pixels=True)
        lb, ppb = _composed_step(net_b, tr_b, x, x_raw, labels, mask, sel, "entropy", thr, conf_b)
        print("%s step %d: loss %.17g / %.17g, pseudo pixels %s (%.3f of the frame)"
              % (kind, step, float(la), float(lb), ppa.tolist(), ppa[1].item() / (64 * 128)))
        assert float(la).hex() == float(lb).hex(), "loss differs at step %d" % step
        assert np.array_equal(_host(kind, net_a), _host(kind, net_b)), "weights differ at step %d" % step
        assert all(np.array_equal(a, b) for a, b in zip(_flat_state(kind, tr_a), _flat_state(kind, tr_b))), \
            "Adam slots differ at step %d" % step
        assert torch.equal(ppa, ppb) and ppa[0].item() == 0
        assert torch.equal(conf_a, conf_b), "confusion differs at step %d" % step
    assert tr_a.state["t"] == tr_b.state["t"] == 5 and int(conf_a.sum()) > 0
    assert not np.array_equal(start, _host(kind, net_a))


@pytest.mark.parametrize("kind", KINDS)
def test_determinism_and_bookkeeping(kind):
    """two calls give the same bits; the confusion matrix accumulates across two calls; labelled images get 0 pseudo pixels;
    a call with no semi keyword gives the parent class' bits"""
    k, labelled = 19, [0, 1]
    feats, d, labels, mask = _case(kind, 19200 + KINDS.index(kind), 2, 2, 3, k, labelled)
    feats2 = _other(feats, 1.1, 1.1)
    net, tr0, tr1 = _trainers(kind, k, WL[1])
    thr = _median_threshold(kind, net, feats2, d, "entropy", labelled)
    a = _fused(kind, net, tr1, feats, feats2, d, labels, mask, labelled, "entropy", thr)
    b = _fused(kind, net, tr1, feats, feats2, d, labels, mask, labelled, "entropy", thr)
    _assert_same("second call", b, a)
    assert a[3][1].item() == 0 and a[3][0].item() > 0
    conf = a[2].clone()
    tr1.gradient_features(*feats, labels, mask, params=d, labelled=labelled, threshold=thr, features_raw=feats2,
                          confusion=conf)
    assert torch.equal(conf, 2 * a[2]) and int(a[2].sum()) > 0
    fl, _, labels_l, mask_l = _case(kind, 19210 + KINDS.index(kind), 2, 2, 3, k, [1, 1])
    l0, g0 = tr0.gradient_features(*fl, labels_l, mask_l, params=d, max_workgroups=1)
    l1, g1 = tr1.gradient_features(*fl, labels_l, mask_l, params=d, max_workgroups=1)
    assert torch.equal(l0, l1) and torch.equal(_pack(kind, g0), _pack(kind, g1))
    l2, g2 = tr1.gradient_features(*fl, labels_l, mask_l, params=d, max_workgroups=1,
                                   labelled=torch.ones(2, dtype=torch.bool))
    assert torch.equal(l0, l2) and torch.equal(_pack(kind, g0), _pack(kind, g2))
