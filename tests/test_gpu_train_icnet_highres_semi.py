"""The semi-supervised step of ICNet's high-resolution trainer on the MI355X: pseudo annotation and
training metrics inside k_icnet_head_grad<K, true, true> behind the branch being trained, against the COMPOSITION of code
sections 25, 30 and 32 already pin to their oracles -- the forward path's full-resolution logits under the weights being
trained, score_logits with label / mask / confidence planes, training_targets, ``ICNetHighResTrainer``'s plain gradient / step,
the stand-alone confusion op.  The interpolated logits, pixel_score and everything behind dL/dlogit are the same code on both
routes, so the loss and all 23 gradients are compared bit for bit and the counts exactly.  Shapes are N x h32 x w32: 1 x 1 x 1 is
one 32 x 32 frame."""
import numpy as np
import pytest
import torch

import semanticsegmentationactivelearning_amd as ssal
from semanticsegmentationactivelearning_amd import _lib
from semanticsegmentationactivelearning_amd import active_learning as al
from semanticsegmentationactivelearning_amd import inference
from semanticsegmentationactivelearning_amd import synthetic as syn
from semanticsegmentationactivelearning_amd.models.util import conv_ops as cops
from semanticsegmentationactivelearning_amd.tensortools import metrics
from semanticsegmentationactivelearning_amd.training import ICNetHighResTrainer, SemiSupervisedICNetHighResTrainer

import icnet_highres_train_oracle as iho3
from guarded_alloc import PATTERNS as POISON, GuardedAlloc, same_bits
from helpers import frames

pytestmark = pytest.mark.gpu

MEASURES = ("entropy", "margin", "confidence")
KS = (2, 6, 19, 32)
WL = ((0.0, 0.0), (1.02, 0.1))
NAMES = iho3.NAMES
STAT_NAMES = tuple("%s.%s" % (l, a) for l in iho3.LAYERS for a in ("mean", "variance")) + (
    "conv_sub4.mean", "conv_sub4.variance", "conv3_1_sub2_proj.mean", "conv3_1_sub2_proj.variance",
    "conv_sub2.mean", "conv_sub2.variance", "conv3_sub1_proj.mean", "conv3_sub1_proj.variance")
MAX_DRAWS = 6
_NETS = {}


def _var(net, name):
    layer, attr = name.split(".")
    return getattr(getattr(net, layer), attr)


def _net(k, c_in=3):
    net = ssal.ICNet(k)
    net.build((None, None, None, c_in))
    return net


def _shared_net(k, c_in=3):
    """one model per class and channel count for the gradient cases (they pass the weights as ``params``; only the moving
    statistics are assigned, per case)"""
    if (k, c_in) not in _NETS:
        _NETS[(k, c_in)] = _net(k, c_in)
    return _NETS[(k, c_in)]


def _set_stats(net, stats):
    for name, v in zip(STAT_NAMES, np.split(stats, np.cumsum(iho3.STAT_WIDTHS)[:-1])):
        _var(net, name).assign(v)


def _case(seed, n, h, w, k, labelled, c_in=3):
    """((conv5_4_k1, conv3_1, uint8 frames) on the device, weights, stats, labels, mask) of icnet_highres_train_oracle.case.
    The planes of unlabelled images hold 0xFF labels and NaN masks (never read); the first labelled image carries label 255
    under mask 1 on a few pixels (key >= K^2: dropped from the confusion matrix) and a mask value of 2.0 on a few (adds 2)."""
    c54, c31, u8, d, stats, labels, mask = iho3.case(seed, n, h, w, k, c_in=c_in)
    labels, mask = np.array(labels), np.array(mask)
    first = True
    for i, l in enumerate(labelled):
        if not l:
            labels[i], mask[i] = 0xFF, np.nan
        elif first:
            first = False
            labels[i, 0, :3], mask[i, 0, :3] = 255, 1.0
            labels[i, -1, -3:] = np.arange(3) % k
            mask[i, -1, -3:] = 2.0
    d = {name: np.ascontiguousarray(v, dtype=np.float32) for name, v in d.items()}
    feats = tuple(torch.as_tensor(a).cuda() for a in (c54, c31, u8))
    return feats, d, stats, torch.as_tensor(labels).cuda(), torch.as_tensor(mask).cuda()


def _unit(x):
    """the frames as launch_conv_first reads them"""
    return x.to(torch.float32) * np.float32(1.0 / 255.0) if x.dtype == torch.uint8 else x


def _logits(net, feats, d):
    """the full-resolution logits of the forward path under the variables ``d``: its own launches, then its 4x resize"""
    bn = lambda layer: (_var(net, layer + ".mean").numpy(), _var(net, layer + ".variance").numpy(), d[layer + ".gamma"],
                        d[layer + ".beta"])
    a = _unit(feats[2])
    for layer in iho3.LAYERS:
        a = cops.conv_bn_act(a, d[layer + ".kernel"], stride=2, bn=bn(layer), relu=True)
    p24 = cops.conv_bn_act(feats[1], d["conv3_1_sub2_proj.kernel"], bn=bn("conv3_1_sub2_proj"), relu=False)
    sub24 = cops.conv_bn_act(feats[0], d["conv_sub4.kernel"], dilation=2, bn=bn("conv_sub4"), residual=p24, relu=True,
                             upsample2x=True)
    proj = cops.conv_bn_act(a, d["conv3_sub1_proj.kernel"], bn=bn("conv3_sub1_proj"), relu=False)
    sub12 = cops.conv_bn_act(sub24, d["conv_sub2.kernel"], dilation=2, bn=bn("conv_sub2"), residual=proj, relu=True,
                             upsample2x=True)
    lq = cops.conv_bn_act(sub12, d["conv6_cls.kernel"], bias=d["conv6_cls.bias"], relu=False, upsample2x=True)
    return inference.resize_bilinear(lq, (4 * lq.shape[1], 4 * lq.shape[2]))


def _other(feats, lo, hi):
    """inputs that differ from ``feats``: every feature channel scaled by its own factor, the frames' channels reversed and
    mirrored left to right"""
    c54, c31, x = feats
    scale = lambda f: (f * torch.linspace(lo, hi, f.shape[-1], device="cuda")).contiguous()
    return scale(c54), scale(c31), x.flip(-1).flip(2).contiguous()


def _pack(gd):
    return torch.cat([gd[n].reshape(-1) for n in NAMES])


def _sel(labelled, n):
    return torch.ones(n, dtype=torch.bool, device="cuda") if labelled is None else torch.as_tensor(
        np.asarray(labelled, dtype=bool)).cuda()


def _median_threshold(net, feats_raw, d, measure, labelled):
    """the median of the yardstick's confidence over the unlabelled pixels, and the share of them it lets pass"""
    _, p = al.score_logits(_logits(net, feats_raw, d), measure, 0.0, return_confidence=True)
    c = p["confidence"][~_sel(labelled, feats_raw[0].shape[0])].cpu().numpy()
    thr = float(np.median(c))
    return thr, float((c >= np.float32(thr)).mean())


def _composed(net, tr, feats, feats_raw, d, labels, mask, labelled, measure, threshold, mw=0):
    """(loss, packed gradient, confusion, pseudo pixels, confidence plane, mask trained on) of the composed step"""
    n, h, w, _ = feats[0].shape
    k = net.classes
    sel = _sel(labelled, n)
    _, p = al.score_logits(_logits(net, feats_raw, d), measure, threshold, return_label=True, return_mask=True,
                           return_confidence=True)
    if labels is None:
        labels = torch.zeros((n, 32 * h, 32 * w), dtype=torch.uint8, device="cuda")
        mask = torch.zeros((n, 32 * h, 32 * w), dtype=torch.float32, device="cuda")
    lab, mk = al.training_targets(sel, labels, mask, p["label"], p["mask"].float())
    loss, gd = tr.gradient_features(*feats, lab, mk, params=d, max_workgroups=mw)
    _, pt = al.score_logits(_logits(net, feats, d), "confidence", 0.0, return_label=True)  # the first maximum
    conf = metrics.confusion_mat(lab, pt["label"], k, weights=mk)
    pp = p["mask"].to(torch.int64).sum(dim=(1, 2)) * (~sel).to(torch.int64)
    return loss, _pack(gd), conf, pp, p["confidence"], mk


def _fused(net, tr, feats, feats_raw, d, labels, mask, labelled, measure, threshold, mw=0):
    k = net.classes
    conf = torch.zeros((k, k), dtype=torch.int64, device="cuda")
    loss, gd, pp = tr.gradient_features(*feats, labels, mask, params=d, max_workgroups=mw, labelled=labelled, measure=measure,
                                        threshold=threshold, features_raw=feats_raw, confusion=conf, return_pseudo_pixels=True)
    return loss, _pack(gd), conf, pp


def _assert_same(name, got, want):
    loss, grad, conf, pp = got[:4]
    wloss, wgrad, wconf, wpp = want[:4]
    print("%s: loss %.17g / %.17g, confusion sum %d / %d, pseudo pixels %s / %s"
          % (name, float(loss[0]), float(wloss[0]), int(conf.sum()), int(wconf.sum()), pp.tolist(), wpp.tolist()))
    assert torch.equal(loss, wloss), "%s: loss %r != %r" % (name, float(loss[0]), float(wloss[0]))
    gi, wi = grad.view(torch.int32), wgrad.view(torch.int32)
    if not torch.equal(gi, wi):
        off = iho3.offsets(int(conf.shape[0]), (grad.numel() - iho3.floats(int(conf.shape[0]), 3)) // 288 + 3)
        bad = [n for n, (lo, hi) in off.items() if not torch.equal(gi[lo:hi], wi[lo:hi])]
        raise AssertionError("%s: %d of %d gradient entries differ, in %s" % (name, int((gi != wi).sum()), grad.numel(), bad))
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


def _trainers(net, wl):
    return (ICNetHighResTrainer(net, 1e-3, loginverse_scaling=wl[0], label_smoothing=wl[1]),
            SemiSupervisedICNetHighResTrainer(net, 1e-3, loginverse_scaling=wl[0], label_smoothing=wl[1]))


def _drawn_case(name, seed, shape, k, measure, labelled, c_in=3, raw=None):
    """the case of ``seed`` and the threshold: the median of the yardstick's confidence over the unlabelled pixels.  On a
    one-cell map the clamped taps of the resizes make a quarter of an image's confidences one value; where
    the median then lets more than 0.7 (or fewer than 0.3) of them pass, the next draw (seed + 1000) is taken.  The draw is a
    condition on the YARDSTICK's planes alone and is printed; maps of more than one cell keep draw 0."""
    n, h, w = shape
    marks = [1] * n if labelled is None else labelled
    net = _shared_net(k, c_in)
    for draw in range(MAX_DRAWS if h * w == 1 else 1):
        feats, d, stats, labels, mask = _case(seed + 1000 * draw, n, h, w, k, marks, c_in)
        _set_stats(net, stats)
        if all(marks):
            return net, feats, d, labels, mask, 0.5
        src = feats if raw is None else raw(feats)
        thr, share = _median_threshold(net, src, d, measure, labelled)
        if 0.3 <= share <= 0.7:
            break
    print("%s: draw %d (seed %d)" % (name, draw, seed + 1000 * draw))
    return net, feats, d, labels, mask, thr


def _run_case(name, seed, shape, k, measure, labelled, wl, mw=0, no_planes=False, c_in=3):
    net, feats, d, labels, mask, thr = _drawn_case(name, seed, shape, k, measure, labelled, c_in)
    tr0, tr1 = _trainers(net, wl)
    if no_planes:
        labels = mask = None
    want = _composed(net, tr0, feats, feats, d, labels, mask, labelled, measure, thr, mw)
    got = _fused(net, tr1, feats, None, d, labels, mask, labelled, measure, thr, mw)
    _assert_mixed_masks(name, want, labelled, shape[0], thr)
    _assert_same(name, got, want)
    return got, want


# `labelled` of the main sweep on 2 x 2 x 3: not given (confusion only), all labelled, mixed, all unlabelled (no planes)
PATTERNS = (("not given", None, False), ("all", [1, 1], False), ("mixed", [1, 0], False), ("none", [0, 0], True))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("measure", MEASURES)
def test_main_sweep_matches_composition(k, measure):
    """2 x 2 x 3 (frames of 64 x 96: several tiles of every kernel, two images): bitwise loss and gradients, equal confusion
    matrix and pseudo-pixel counts; (weight, label smoothing) alternates over the cases; the seed is a fixed function of the
    case"""
    base = 4 * (len(MEASURES) * KS.index(k) + MEASURES.index(measure))
    for j, (pname, labelled, no_planes) in enumerate(PATTERNS):
        case = base + j
        name = "K=%d %s labelled=%s w=%g ls=%g" % ((k, measure, pname) + WL[case % 2])
        got, _ = _run_case(name, 37000 + case, (2, 2, 3), k, measure, labelled, WL[case % 2], no_planes=no_planes)
        if labelled is None or all(labelled):
            assert got[3].tolist() == [0, 0]
        if pname == "mixed":
            assert got[3][0].item() == 0 and 0 < got[3][1].item() < 64 * 96


# the smallest map the resizes' clamped taps allow, and the shapes where section 32's grids stride over partial tiles and
# k_front2's 8 x 16 tile is partial in both directions; a batch of one image has no mixed `labelled`: it runs unlabelled (the
# side the new code is on) and labelled (the confusion keys)
OTHER = [((1, 1, 1), 1), ((1, 1, 1), 2), ((1, 3, 2), 1), ((1, 3, 2), 2), ((1, 3, 5), 1), ((1, 3, 5), 2)]


@pytest.mark.parametrize("shape,mw", OTHER)
@pytest.mark.parametrize("labelled", [[0], [1]])
def test_small_shapes_and_grids_match_composition(shape, mw, labelled):
    case = 2 * OTHER.index((shape, mw)) + labelled[0]
    measure = MEASURES[case % 3]
    name = "%s mw=%d labelled=%s %s" % (shape, mw, labelled, measure)
    got, _ = _run_case(name, 38000 + case, shape, 19, measure, labelled, WL[case % 2], mw)
    if labelled[0]:
        assert got[3][0].item() == 0 and int(got[2].sum()) > 0
    else:
        assert 0 < got[3][0].item() < 32 * 32 * shape[1] * shape[2]


def test_four_channel_frames_and_uint8_against_fp32():
    """C_in = 4 without a raw side (launch_conv_first's four-channel kernel, k_icnet_highres_wgrad1<4>), then uint8 against fp32
    frames on both sides of a call with a raw side, for both channel counts (k_front2<3 / 4, uint8_t / float, 2>): the same bits"""
    _run_case("C_in=4", 38100, (1, 3, 5), 19, "margin", [0], WL[1], mw=2, c_in=4)
    k, labelled, measure = 19, [0, 1], "entropy"
    for c_in in (3, 4):
        raw = lambda f: _other(f, 1.2, 0.85)
        name = "uint8 / fp32 C_in=%d" % c_in
        net, feats, d, labels, mask, thr = _drawn_case(name, 38110 + c_in, (2, 1, 2), k, measure, labelled, c_in, raw=raw)
        feats_raw = raw(feats)
        tr0, tr1 = _trainers(net, WL[1])
        want = _composed(net, tr0, feats, feats_raw, d, labels, mask, labelled, measure, thr)
        _assert_mixed_masks(name, want, labelled, 2, thr)
        g8 = _fused(net, tr1, feats, feats_raw, d, labels, mask, labelled, measure, thr)
        f32 = lambda f: (f[0], f[1], _unit(f[2]))
        g32 = _fused(net, tr1, f32(feats), f32(feats_raw), d, labels, mask, labelled, measure, thr)
        _assert_same(name + " uint8", g8, want)
        _assert_same(name + " fp32", g32, want)
        with pytest.raises(ValueError, match="dtype of images"):
            _fused(net, tr1, feats, f32(feats_raw), d, labels, mask, labelled, measure, thr)


def test_threshold_between_two_images():
    """3 x 1 x 1 with logits constant over every image: constant backbone features, conv_sub2 reduced to its centre tap (on
    these maps every off-centre tap of the first dilated convolution is padding anyway) and a branch whose output is constant
    (conv3_sub1's kernel zero: conv3_sub1 = relu(shift), whatever the frame).  Images 0 and 2 are unlabelled, the threshold is
    the mean of their two confidences: one image passes whole, the other fails whole."""
    k, labelled, measure = 19, [0, 1, 0], "entropy"
    feats, d, stats, labels, mask = _case(39000, 3, 1, 1, k, labelled)
    feats = tuple(f[:, :1, :1, :].expand_as(f).contiguous() for f in feats[:2]) + (feats[2],)
    centre = d["conv_sub2.kernel"][1, 1].copy()
    d["conv_sub2.kernel"][:] = 0.0
    d["conv_sub2.kernel"][1, 1] = centre
    d["conv3_sub1.kernel"][:] = 0.0
    net = _shared_net(k)
    _set_stats(net, stats)
    tr0, tr1 = _trainers(net, WL[1])
    _, p = al.score_logits(_logits(net, feats, d), measure, 0.0, return_confidence=True)
    c = p["confidence"].cpu().numpy().astype(np.float64)
    assert c[0].min() == c[0].max() and c[2].min() == c[2].max() and c[0, 0, 0] != c[2, 0, 0]
    thr = 0.5 * (c[0, 0, 0] + c[2, 0, 0])
    want = _composed(net, tr0, feats, feats, d, labels, mask, labelled, measure, thr)
    got = _fused(net, tr1, feats, None, d, labels, mask, labelled, measure, thr)
    _assert_same("3x1x1", got, want)
    assert sorted(got[3].tolist()) == [0, 0, 32 * 32] and got[3][1].item() == 0
    # ... and through the target launch (copies of the inputs as the raw side)
    _assert_same("3x1x1 raw", _fused(net, tr1, feats, tuple(f.clone() for f in feats), d, labels, mask, labelled, measure, thr),
                 want)


def _host(net):
    return np.concatenate([_var(net, n).numpy().reshape(-1) for n in NAMES])


def _flat_state(tr):
    st = tr.state
    return [np.concatenate([st[s][n].reshape(-1) for n in NAMES]) for s in ("m", "v")]


HYPER = dict(learning_rate=5e-4, beta1=0.9, beta2=0.99, loginverse_scaling=1.02, label_smoothing=0.1, l2=2e-4)


def test_raw_side_through_features():
    """the pseudo annotation comes from features_raw -- the raw backbone features AND the raw frames, through the branch under
    the variables given as ``params`` (they differ from the model's committed ones) -- the gradient from the training inputs:
    gradient_features against the composition, then step_features against the composed plain step"""
    k, labelled, measure = 19, [0, 1], "margin"
    raw = lambda f: _other(f, 0.8, 1.25)
    net, feats, d, labels, mask, thr = _drawn_case("features_raw", 39100, (2, 2, 3), k, measure, labelled, raw=raw)
    feats_raw = raw(feats)
    assert not np.array_equal(d["conv2_sub1.kernel"], _var(net, "conv2_sub1.kernel").numpy())
    tr0, tr1 = _trainers(net, WL[1])
    want = _composed(net, tr0, feats, feats_raw, d, labels, mask, labelled, measure, thr)
    got = _fused(net, tr1, feats, feats_raw, d, labels, mask, labelled, measure, thr)
    _assert_mixed_masks("features_raw", want, labelled, 2, thr)
    _assert_same("features_raw", got, want)
    one_pass = _fused(net, tr1, feats, None, d, labels, mask, labelled, measure, thr)
    assert not torch.equal(one_pass[1], got[1]), "the raw inputs made no difference: the case shows nothing"
    # the raw FRAMES alone matter: the raw branch really runs, on them
    frames_only = _fused(net, tr1, feats, feats[:2] + (feats_raw[2],), d, labels, mask, labelled, measure, thr)
    assert not torch.equal(frames_only[1], one_pass[1]) and not torch.equal(frames_only[1], got[1])
    # ... under the trained variables: the composition with the model's committed branch gives other targets
    d_model = dict(d, **{n: _var(net, n).numpy() for n in iho3.BRANCH})
    _, p_model = al.score_logits(_logits(net, feats_raw, d_model), measure, thr, return_label=True)
    _, p_train = al.score_logits(_logits(net, feats_raw, d), measure, thr, return_label=True)
    assert not torch.equal(p_model["label"], p_train["label"])
    _assert_same("features_raw is features", _fused(net, tr1, feats, feats, d, labels, mask, labelled, measure, thr), one_pass)
    _assert_same("features_raw == features (copies: the target launch)",
                 _fused(net, tr1, feats, tuple(f.clone() for f in feats), d, labels, mask, labelled, measure, thr), one_pass)
    # step_features: twin models under the same variables and statistics
    net_a, net_b = _net(k), _net(k)
    for twin in (net_a, net_b):
        for name in STAT_NAMES:
            _var(twin, name).assign(_var(net, name).numpy())
        for name, v in d.items():
            _var(twin, name).assign(v)
    tr_a, tr_b = SemiSupervisedICNetHighResTrainer(net_a, **HYPER), ICNetHighResTrainer(net_b, **HYPER)
    conf_a = torch.zeros((k, k), dtype=torch.int64, device="cuda")
    la, ppa = tr_a.step_features(*feats, labels, mask, labelled=labelled, measure=measure, threshold=thr,
                                 features_raw=feats_raw, confusion=conf_a, return_pseudo_pixels=True)
    sel = _sel(labelled, 2)
    _, p = al.score_logits(_logits(net, feats_raw, d), measure, thr, return_label=True, return_mask=True)
    lab, mk = al.training_targets(sel, labels, mask, p["label"], p["mask"].float())
    lb = tr_b.step_features(*feats, lab, mk)
    assert float(la).hex() == float(lb).hex()
    assert np.array_equal(_host(net_a), _host(net_b))
    assert all(np.array_equal(a, b) for a, b in zip(_flat_state(tr_a), _flat_state(tr_b)))
    assert torch.equal(conf_a, want[2]) and torch.equal(ppa, want[3])


@pytest.fixture
def shipped_front():
    shipped = _lib.get_knobs()["ic_front"]
    yield shipped
    _lib.set_knob("ic_front", shipped)


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 3, 5)])
@pytest.mark.parametrize("u8", [True, False])
def test_fused_front_against_the_unfused_route(shipped_front, shape, u8):
    """the same raw-side call with conv1_sub1 + conv2_sub1 of the undistorted frames as one k_front2 launch (the shipped
    setting) and as the two separate launches (bit 0 of the knob "ic_front" cleared): loss, the 23 gradients, the confusion
    matrix and the pseudo pixels bit-equal -- and equal to the composition"""
    k, labelled, measure = 19, [0], MEASURES[shape[1] % 3]
    raw = lambda f: _other(f, 1.2, 0.85)
    name = "front %s u8=%s" % (shape, u8)
    net, feats, d, labels, mask, thr = _drawn_case(name, 39200 + shape[1], shape, k, measure, labelled, raw=raw)
    if not u8:
        feats = feats[:2] + (_unit(feats[2]),)
    feats_raw = raw(feats)
    tr0, tr1 = _trainers(net, WL[1])
    out = {}
    for front in (shipped_front, shipped_front & ~1):
        _lib.set_knob("ic_front", front)
        route = _lib.icnet_highres_raw_route(3, *shape)
        assert route == ("fused" if front & 1 else "unfused")
        out[route] = _fused(net, tr1, feats, feats_raw, d, labels, mask, labelled, measure, thr, mw=2)
    _lib.set_knob("ic_front", shipped_front)
    assert sorted(out) == ["fused", "unfused"]
    _assert_same(name + ": fused front against the separate launches", out["fused"], out["unfused"])
    want = _composed(net, tr0, feats, feats_raw, d, labels, mask, labelled, measure, thr, mw=2)
    _assert_mixed_masks(name, want, labelled, 1, thr)
    _assert_same(name, out["fused"], want)
    assert 0 < out["fused"][3][0].item() < 32 * 32 * shape[1] * shape[2]


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
    c = p["confidence"][1].cpu().numpy()
    thr = float(np.median(c))
    assert 0.3 <= float((c >= np.float32(thr)).mean()) <= 0.7
    return thr


@pytest.mark.parametrize("u8", [False, True])
def test_images_raw_equals_features_raw_and_composition(icnet19, u8):
    """step(images, images_raw=) == step_features(*features(images), images, features_raw=(*features(images_raw), images_raw))
    bit for bit, and both equal the composed step; images_raw is images == no raw side"""
    x, x_raw, labels, mask, sel = _frames_case(u8)
    nets = [_twin(icnet19) for _ in range(3)]
    tr_a, tr_b = (SemiSupervisedICNetHighResTrainer(n, **HYPER) for n in nets[:2])
    tr_c = ICNetHighResTrainer(nets[2], **HYPER)
    for tr in (tr_a, tr_b, tr_c):
        tr.reinitialize(seed=4)
    thr = _frame_threshold(nets[2], x_raw, "margin")
    feats, feats_raw = tr_b.features(x), tr_b.features(x_raw)
    assert not any(torch.equal(a, b) for a, b in zip(feats, feats_raw))
    conf = [torch.zeros((19, 19), dtype=torch.int64, device="cuda") for _ in range(3)]
    for step in range(2):
        la, ppa = tr_a.step(x, labels, mask, labelled=sel, measure="margin", threshold=thr, images_raw=x_raw,
                            confusion=conf[0], return_pseudo_pixels=True)
        lb, ppb = tr_b.step_features(*feats, x, labels, mask, labelled=sel, measure="margin", threshold=thr,
                                     features_raw=feats_raw + (x_raw,), confusion=conf[1], return_pseudo_pixels=True)
        lc, ppc = _composed_step(nets[2], tr_c, x, x_raw, labels, mask, sel, "margin", thr, conf[2])
        print("step %d: loss %.17g / %.17g / %.17g, pseudo pixels %s" % (step, float(la), float(lb), float(lc), ppa.tolist()))
        assert float(la).hex() == float(lb).hex() == float(lc).hex(), "loss differs at step %d" % step
        for other in nets[1:]:
            assert np.array_equal(_host(nets[0]), _host(other)), "weights differ at step %d" % step
        assert torch.equal(ppa, ppb) and torch.equal(ppa, ppc) and ppa[0].item() == 0 and 0 < ppa[1].item() < 64 * 128
        assert torch.equal(conf[0], conf[1]) and torch.equal(conf[0], conf[2])
    net_d, net_e = _twin(icnet19), _twin(icnet19)
    tr_d, tr_e = SemiSupervisedICNetHighResTrainer(net_d, **HYPER), SemiSupervisedICNetHighResTrainer(net_e, **HYPER)
    ld = tr_d.step(x, labels, mask, labelled=sel, threshold=0.3, images_raw=x)
    le = tr_e.step(x, labels, mask, labelled=sel, threshold=0.3)
    assert float(ld).hex() == float(le).hex() and np.array_equal(_host(net_d), _host(net_e))


def test_twin_nets_five_steps(icnet19):
    """five fused steps on one net, five composed steps on its twin (mixed `labelled`, images_raw given): all 23 trained tensors,
    m, v, loss, confusion and pseudo pixels equal after every step"""
    x, x_raw, labels, mask, sel = _frames_case()
    net_a, net_b = _twin(icnet19), _twin(icnet19)
    tr_a, tr_b = SemiSupervisedICNetHighResTrainer(net_a, **HYPER), ICNetHighResTrainer(net_b, **HYPER)
    tr_a.reinitialize(seed=5)
    tr_b.reinitialize(seed=5)
    thr = _frame_threshold(net_b, x_raw, "entropy")
    conf_a = torch.zeros((19, 19), dtype=torch.int64, device="cuda")
    conf_b = torch.zeros_like(conf_a)
    start = _host(net_a)
    for step in range(5):
        la, ppa = tr_a.step(x, labels, mask, labelled=sel, measure="entropy", threshold=thr, images_raw=x_raw,
                            confusion=conf_a, return_pseudo_pixels=True)
        lb, ppb = _composed_step(net_b, tr_b, x, x_raw, labels, mask, sel, "entropy", thr, conf_b)
        print("step %d: loss %.17g / %.17g, pseudo pixels %s (%.3f of the frame)"
              % (step, float(la), float(lb), ppa.tolist(), ppa[1].item() / (64 * 128)))
        assert float(la).hex() == float(lb).hex(), "loss differs at step %d" % step
        assert np.array_equal(_host(net_a), _host(net_b)), "weights differ at step %d" % step
        assert all(np.array_equal(a, b) for a, b in zip(_flat_state(tr_a), _flat_state(tr_b))), \
            "Adam slots differ at step %d" % step
        assert torch.equal(ppa, ppb) and ppa[0].item() == 0
        assert torch.equal(conf_a, conf_b), "confusion differs at step %d" % step
    assert tr_a.state["t"] == tr_b.state["t"] == 5 and int(conf_a.sum()) > 0
    assert not np.array_equal(start, _host(net_a))
    assert len(NAMES) == 23 and all(not np.array_equal(_var(net_a, n).numpy(), _var(icnet19, n).numpy()) for n in NAMES)


def test_determinism_and_bookkeeping():
    """two calls give the same bits; the confusion matrix accumulates across two calls; labelled images get 0 pseudo pixels;
    a call with no semi keyword gives the parent class' bits"""
    k, labelled = 19, [0, 1]
    raw = lambda f: _other(f, 1.1, 1.1)
    net, feats, d, labels, mask, thr = _drawn_case("bookkeeping", 39300, (2, 2, 3), k, "entropy", labelled, raw=raw)
    feats2 = raw(feats)
    tr0, tr1 = _trainers(net, WL[1])
    a = _fused(net, tr1, feats, feats2, d, labels, mask, labelled, "entropy", thr)
    b = _fused(net, tr1, feats, feats2, d, labels, mask, labelled, "entropy", thr)
    _assert_same("second call", b, a)
    assert a[3][1].item() == 0 and a[3][0].item() > 0
    conf = a[2].clone()
    tr1.gradient_features(*feats, labels, mask, params=d, labelled=labelled, threshold=thr, features_raw=feats2, confusion=conf)
    assert torch.equal(conf, 2 * a[2]) and int(a[2].sum()) > 0
    fl, _, stats, labels_l, mask_l = _case(39310, 2, 2, 3, k, [1, 1])
    _set_stats(net, stats)
    tr0, tr1 = _trainers(net, WL[1])
    l0, g0 = tr0.gradient_features(*fl, labels_l, mask_l, params=d, max_workgroups=1)
    l1, g1 = tr1.gradient_features(*fl, labels_l, mask_l, params=d, max_workgroups=1)
    assert torch.equal(l0, l1) and torch.equal(_pack(g0), _pack(g1))
    l2, g2 = tr1.gradient_features(*fl, labels_l, mask_l, params=d, max_workgroups=1, labelled=torch.ones(2, dtype=torch.bool))
    assert torch.equal(l0, l2) and torch.equal(_pack(g0), _pack(g2))


def _run_entries(make_net, x, x_raw, labels, mask, sel, thr):
    """the semi features entry with a raw side (gradient), then two steps through the semi images entry with images_raw"""
    net = make_net()
    tr = SemiSupervisedICNetHighResTrainer(net, **HYPER)
    feats, feats_raw = tr.features(x), tr.features(x_raw)
    net._workspaces.clear()
    conf = torch.zeros((19, 19), dtype=torch.int64, device="cuda")
    loss, gd, pp = tr.gradient_features(*feats, x, labels, mask, labelled=sel, measure="margin", threshold=thr,
                                        features_raw=feats_raw + (x_raw,), confusion=conf, return_pseudo_pixels=True)
    out = {"loss": loss.cpu().numpy(), "grad": _pack(gd).cpu().numpy(), "pp": pp.cpu().numpy()}
    steps = [tr.step(x, labels, mask, labelled=sel, measure="margin", threshold=thr, images_raw=x_raw, confusion=conf,
                     return_pseudo_pixels=True) for _ in range(2)]
    torch.cuda.synchronize()
    out["steps"] = np.array([float(s[0]) for s in steps])
    out["step_pp"] = np.stack([s[1].cpu().numpy() for s in steps])
    out["confusion"] = conf.cpu().numpy()
    out["weights"] = _host(net)
    return out


@pytest.mark.parametrize("pattern", POISON, ids=["0xFF", "0x7F", "0xFE"])
def test_entries_on_poisoned_workspaces_with_guarded_outputs(icnet19, pattern):
    """tests/test_gpu_guarded.py's pattern over the two new entries: every workspace byte poisoned before the call, every
    output between guard bands -- the same bits as on plain allocations, no guard touched"""
    def make_net():
        return _twin(icnet19)
    x_host = frames([3, 4], 64, 128, 3)
    raw_host = np.ascontiguousarray(x_host[:, :, ::-1, ::-1])
    rng = np.random.default_rng(9)
    labels = rng.integers(0, 19, (2, 64, 128)).astype(np.uint8)
    mask = (rng.uniform(size=(2, 64, 128)) > 0.2).astype(np.float32)
    labels[1], mask[1] = 0xFF, np.nan
    sel = np.array([1, 0], np.uint8)
    thr = _frame_threshold(icnet19, torch.as_tensor(raw_host).cuda(), "margin")
    want = _run_entries(make_net, torch.as_tensor(x_host).cuda(), torch.as_tensor(raw_host).cuda(), labels, mask, sel, thr)
    assert 0 < want["pp"][1] < 64 * 128 and want["pp"][0] == 0
    with GuardedAlloc("cuda", pattern) as g:
        got = _run_entries(make_net, g.guarded_from_numpy(x_host), g.guarded_from_numpy(raw_host), labels, mask, sel, thr)
        g.check()
        assert g.count > 0
    for key in want:
        assert same_bits(got[key], want[key]), key
