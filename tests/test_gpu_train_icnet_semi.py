"""The semi-supervised step of ICNet's output-layer trainer on the MI355X: pseudo annotation and
training metrics inside k_icnet_head_grad<K, true>, against the COMPOSITION of code the parent already pins to the oracles --
the forward path's full-resolution logits, score_logits with label / mask / confidence planes, training_targets,
ICNetHeadTrainer's plain gradient / step, the stand-alone confusion op.  The interpolated logits, pixel_score and the gradient
arithmetic are the same code on both routes, so loss, dKernel and dBias are compared bit for bit and the counts exactly."""
import numpy as np
import pytest
import torch

import semanticsegmentationactivelearning_amd as ssal
from semanticsegmentationactivelearning_amd import active_learning as al
from semanticsegmentationactivelearning_amd import inference
from semanticsegmentationactivelearning_amd import synthetic as syn
from semanticsegmentationactivelearning_amd.models.util import conv_ops as cops
from semanticsegmentationactivelearning_amd.tensortools import metrics
from semanticsegmentationactivelearning_amd.training import ICNetHeadTrainer, SemiSupervisedICNetHeadTrainer

pytestmark = pytest.mark.gpu

MEASURES = ("entropy", "margin", "confidence")
KS = (2, 6, 19, 32)
WL = ((0.0, 0.0), (1.02, 0.1))
_NETS = {}


def _net(k):
    net = ssal.ICNet(k)
    net.build((None, None, None, 3))
    return net


def _shared_net(k):
    """one model per class count for the gradient cases (they pass the head as ``params`` and change nothing)"""
    if k not in _NETS:
        _NETS[k] = _net(k)
    return _NETS[k]


def _params(head, k):
    return {"conv6_cls.kernel": head[:128 * k].reshape(1, 1, 128, k), "conv6_cls.bias": head[128 * k:]}


def _pack(gd):
    return torch.cat([gd["conv6_cls.kernel"].reshape(-1), gd["conv6_cls.bias"].reshape(-1)])


def _logits(x, head, k):
    """the full-resolution logits of the forward path under ``head``: its fused 2x + 1x1 launch, then its 4x resize"""
    lq = cops.conv_bn_act(x, head[:128 * k].reshape(1, 1, 128, k), bias=head[128 * k:], relu=False, upsample2x=True)
    return inference.resize_bilinear(lq, (4 * lq.shape[1], 4 * lq.shape[2]))


def _case(seed, n, h, w, k, labelled):
    """features (x ~ N(0, 1)), head (kernel U(+-0.2), bias U(+-0.5)) and annotation.  The planes of unlabelled images hold 0xFF
    labels and NaN masks (never read); the first labelled image carries label 255 under mask 1 on a few pixels (key >= K^2:
    dropped from the confusion matrix) and a mask value of 2.0 on a few (adds 2)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, h, w, 128)).astype(np.float32)
    head = np.concatenate([rng.uniform(-0.2, 0.2, 128 * k), rng.uniform(-0.5, 0.5, k)]).astype(np.float32)
    labels = rng.integers(0, k, (n, 8 * h, 8 * w)).astype(np.uint8)
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
    return torch.as_tensor(x).cuda(), head, torch.as_tensor(labels).cuda(), torch.as_tensor(mask).cuda()


def _sel(labelled, n):
    return torch.ones(n, dtype=torch.bool, device="cuda") if labelled is None else torch.as_tensor(
        np.asarray(labelled, dtype=bool)).cuda()


def _median_threshold(x_raw, head, k, measure, labelled):
    """the median of the yardstick's confidence over the unlabelled pixels"""
    _, p = al.score_logits(_logits(x_raw, head, k), measure, 0.0, return_confidence=True)
    sel = _sel(labelled, x_raw.shape[0])
    return float(np.median(p["confidence"][~sel].cpu().numpy()))


def _composed(k, tr, x, x_raw, head, labels, mask, labelled, measure, threshold, mw=0):
    """(loss, packed gradient, confusion, pseudo pixels, confidence plane) of the composed step"""
    n, h, w, _ = x.shape
    sel = _sel(labelled, n)
    _, p = al.score_logits(_logits(x_raw, head, k), measure, threshold, return_label=True, return_mask=True,
                           return_confidence=True)
    if labels is None:
        labels = torch.zeros((n, 8 * h, 8 * w), dtype=torch.uint8, device="cuda")
        mask = torch.zeros((n, 8 * h, 8 * w), dtype=torch.float32, device="cuda")
    lab, mk = al.training_targets(sel, labels, mask, p["label"], p["mask"].float())
    loss, gd = tr.gradient_features(x, lab, mk, params=_params(head, k), max_workgroups=mw)
    _, pt = al.score_logits(_logits(x, head, k), "confidence", 0.0, return_label=True)  # the first maximum
    conf = metrics.confusion_mat(lab, pt["label"], k, weights=mk)
    pp = p["mask"].to(torch.int64).sum(dim=(1, 2)) * (~sel).to(torch.int64)
    return loss, _pack(gd), conf, pp, p["confidence"], mk


def _fused(k, tr, x, x_raw, head, labels, mask, labelled, measure, threshold, mw=0):
    conf = torch.zeros((k, k), dtype=torch.int64, device="cuda")
    loss, gd, pp = tr.gradient_features(x, labels, mask, params=_params(head, k), max_workgroups=mw, labelled=labelled,
                                        measure=measure, threshold=threshold, features_raw=x_raw, confusion=conf,
                                        return_pseudo_pixels=True)
    return loss, _pack(gd), conf, pp


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


def _run_case(name, seed, shape, k, measure, labelled, wl, mw=0, no_planes=False):
    n, h, w = shape
    marks = [1] * n if labelled is None else labelled
    x, head, labels, mask = _case(seed, n, h, w, k, marks)
    tr0 = ICNetHeadTrainer(_shared_net(k), 1e-3, loginverse_scaling=wl[0], label_smoothing=wl[1])
    tr1 = SemiSupervisedICNetHeadTrainer(_shared_net(k), 1e-3, loginverse_scaling=wl[0], label_smoothing=wl[1])
    thr = _median_threshold(x, head, k, measure, labelled) if (labelled is not None and not all(labelled)) else 0.5
    if no_planes:
        labels = mask = None
    want = _composed(k, tr0, x, x, head, labels, mask, labelled, measure, thr, mw)
    got = _fused(k, tr1, x, None, head, labels, mask, labelled, measure, thr, mw)
    _assert_mixed_masks(name, want, labelled, n, thr)
    _assert_same(name, got, want)
    return got, want


# `labelled` of the main sweep on 2 x 3 x 5: not given (confusion only), all labelled, mixed, all unlabelled (no planes)
PATTERNS = (("not given", None, False), ("all", [1, 1], False), ("mixed", [1, 0], False), ("none", [0, 0], True))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("measure", MEASURES)
def test_main_sweep_matches_composition(k, measure):
    """2 x 3 x 5 (two tiles across, both partial, two images): bitwise loss, dKernel and dBias, equal confusion matrix and
    pseudo-pixel counts; (weight, label smoothing) alternates over the cases; the seed is a fixed function of the case"""
    base = 4 * (len(MEASURES) * KS.index(k) + MEASURES.index(measure))
    for j, (pname, labelled, no_planes) in enumerate(PATTERNS):
        case = base + j
        name = "K=%d %s labelled=%s w=%g ls=%g" % ((k, measure, pname) + WL[case % 2])
        got, _ = _run_case(name, 7000 + case, (2, 3, 5), k, measure, labelled, WL[case % 2], no_planes=no_planes)
        if labelled is None or all(labelled):
            assert got[3].tolist() == [0, 0]
        if pname == "mixed":
            assert got[3][0].item() == 0 and 0 < got[3][1].item() < 24 * 40


# the other shapes section 23 found small enough to still break the tiling (N x h8 x w8, max_workgroups), K = 19; a batch of
# one image has no mixed `labelled`: it runs unlabelled (the side the new code is on) and labelled (the confusion keys)
OTHER = [((1, 5, 3), 0, [0]), ((1, 3, 9), 1, [0]), ((1, 3, 9), 2, [0]), ((1, 5, 3), 0, [1]), ((1, 3, 9), 1, [1]),
         ((1, 3, 9), 2, [1])]


@pytest.mark.parametrize("shape,mw,labelled", OTHER)
@pytest.mark.parametrize("measure", MEASURES)
def test_other_shapes_match_composition(shape, mw, labelled, measure):
    case = 3 * OTHER.index((shape, mw, labelled)) + MEASURES.index(measure)
    name = "%s mw=%d labelled=%s %s" % (shape, mw, labelled, measure)
    got, _ = _run_case(name, 8000 + case, shape, 19, measure, labelled, WL[case % 2], mw)
    if labelled[0]:
        assert got[3][0].item() == 0 and int(got[2].sum()) > 0
    else:
        assert 0 < got[3][0].item() < 64 * shape[1] * shape[2]


def test_every_class_count_of_the_semi_and_the_target_launch():
    """all 31 instantiations of k_icnet_head_grad<K, true>, as the training launch on its own logits and as the target-only
    launch + the training launch that reads its plane, on 2 x 3 x 5 with mixed `labelled` (the measure cycles with K)"""
    for k in range(2, 33):
        measure, wl, labelled = MEASURES[k % 3], WL[k % 2], [k % 2, 1 - k % 2]
        x, head, labels, mask = _case(9300 + k, 2, 3, 5, k, labelled)
        x_raw = (x * torch.linspace(1.2, 0.85, 128, device="cuda")).contiguous()
        tr0 = ICNetHeadTrainer(_shared_net(k), 1e-3, loginverse_scaling=wl[0], label_smoothing=wl[1])
        tr1 = SemiSupervisedICNetHeadTrainer(_shared_net(k), 1e-3, loginverse_scaling=wl[0], label_smoothing=wl[1])
        for raw in (None, x_raw):
            name = "K=%d %s raw=%s" % (k, measure, raw is not None)
            thr = _median_threshold(x if raw is None else raw, head, k, measure, labelled)
            want = _composed(k, tr0, x, x if raw is None else raw, head, labels, mask, labelled, measure, thr)
            _assert_mixed_masks(name, want, labelled, 2, thr)
            _assert_same(name, _fused(k, tr1, x, raw, head, labels, mask, labelled, measure, thr), want)


@pytest.mark.parametrize("measure", MEASURES)
def test_one_pixel_feature_maps_threshold_between_two_images(measure):
    """3 x 1 x 1: a 1 x 1 feature map makes an image's logits constant, so all its 64 pixels share one confidence.  Images 0 and
    2 are unlabelled, the threshold is the mean of their two confidences: one image passes whole, the other fails whole."""
    k, labelled = 19, [0, 1, 0]
    wl = WL[MEASURES.index(measure) % 2]
    x, head, labels, mask = _case(9000 + MEASURES.index(measure), 3, 1, 1, k, labelled)
    tr0 = ICNetHeadTrainer(_shared_net(k), 1e-3, loginverse_scaling=wl[0], label_smoothing=wl[1])
    tr1 = SemiSupervisedICNetHeadTrainer(_shared_net(k), 1e-3, loginverse_scaling=wl[0], label_smoothing=wl[1])
    _, p = al.score_logits(_logits(x, head, k), measure, 0.0, return_confidence=True)
    c = p["confidence"].cpu().numpy().astype(np.float64)
    assert c[0].min() == c[0].max() and c[2].min() == c[2].max() and c[0, 0, 0] != c[2, 0, 0]
    thr = 0.5 * (c[0, 0, 0] + c[2, 0, 0])
    want = _composed(k, tr0, x, x, head, labels, mask, labelled, measure, thr)
    got = _fused(k, tr1, x, None, head, labels, mask, labelled, measure, thr)
    _assert_same("3x1x1 " + measure, got, want)
    assert sorted(got[3].tolist()) == [0, 0, 64] and got[3][1].item() == 0


@pytest.mark.parametrize("measure", MEASURES)
def test_raw_features_differ_from_training_features(measure):
    """the pseudo annotation comes from features_raw, the gradient from the training features: gradient_features against the
    composition, then step_features against the composed plain step"""
    k, labelled, shape = 19, [0, 1], (2, 3, 5)
    x_raw, head, labels, mask = _case(9100 + MEASURES.index(measure), 2, 3, 5, k, labelled)
    x = (x_raw * torch.linspace(0.8, 1.25, 128, device="cuda")).contiguous()
    tr0 = ICNetHeadTrainer(_shared_net(k), 1e-3, loginverse_scaling=1.02, label_smoothing=0.1)
    tr1 = SemiSupervisedICNetHeadTrainer(_shared_net(k), 1e-3, loginverse_scaling=1.02, label_smoothing=0.1)
    thr = _median_threshold(x_raw, head, k, measure, labelled)
    want = _composed(k, tr0, x, x_raw, head, labels, mask, labelled, measure, thr)
    got = _fused(k, tr1, x, x_raw, head, labels, mask, labelled, measure, thr)
    _assert_mixed_masks("features_raw " + measure, want, labelled, 2, thr)
    _assert_same("features_raw " + measure, got, want)
    one_pass = _fused(k, tr1, x, None, head, labels, mask, labelled, measure, thr)
    assert not torch.equal(one_pass[1], got[1]), "the raw features made no difference: the case shows nothing"
    _assert_same("features_raw is features", _fused(k, tr1, x, x, head, labels, mask, labelled, measure, thr), one_pass)
    _assert_same("features_raw == features (a copy: the target launch)",
                 _fused(k, tr1, x, x.clone(), head, labels, mask, labelled, measure, thr), one_pass)
    # step_features: twin models under the same head
    net_a, net_b = _net(k), _net(k)
    for net in (net_a, net_b):
        net.conv6_cls.kernel.assign(head[:128 * k].reshape(1, 1, 128, k))
        net.conv6_cls.bias.assign(head[128 * k:])
    hyper = dict(learning_rate=5e-4, beta1=0.9, beta2=0.99, loginverse_scaling=1.02, label_smoothing=0.1, l2=2e-4)
    tr_a, tr_b = SemiSupervisedICNetHeadTrainer(net_a, **hyper), ICNetHeadTrainer(net_b, **hyper)
    conf_a = torch.zeros((k, k), dtype=torch.int64, device="cuda")
    la, ppa = tr_a.step_features(x, labels, mask, labelled=labelled, measure=measure, threshold=thr, features_raw=x_raw,
                                 confusion=conf_a, return_pseudo_pixels=True)
    sel = _sel(labelled, 2)
    _, p = al.score_logits(_logits(x_raw, head, k), measure, thr, return_label=True, return_mask=True)
    lab, mk = al.training_targets(sel, labels, mask, p["label"], p["mask"].float())
    lb = tr_b.step_features(x, lab, mk)
    assert float(la).hex() == float(lb).hex()
    assert np.array_equal(net_a.conv6_cls.kernel.numpy(), net_b.conv6_cls.kernel.numpy())
    assert np.array_equal(net_a.conv6_cls.bias.numpy(), net_b.conv6_cls.bias.numpy())
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


HYPER = dict(learning_rate=5e-4, beta1=0.9, beta2=0.99, loginverse_scaling=1.02, label_smoothing=0.1, l2=2e-4)


def _frames_case(u8=False):
    """2 x 64 x 128 frames, image 1 unlabelled; the training frames are the undistorted ones with the channels reversed"""
    x_raw = syn.synth_frames_device(3, 2, 64, 128, 3, dtype=torch.uint8 if u8 else None)
    x = x_raw.flip(-1).contiguous()
    rng = np.random.default_rng(21)
    labels = rng.integers(0, 19, (2, 64, 128)).astype(np.uint8)
    mask = (rng.uniform(size=(2, 64, 128)) > 0.2).astype(np.float32)
    labels[1], mask[1] = 0xFF, np.nan
    return x, x_raw, torch.as_tensor(labels).cuda(), torch.as_tensor(mask).cuda(), torch.tensor([True, False]).cuda()


def _head_of(net):
    return net.conv6_cls.kernel.numpy().copy(), net.conv6_cls.bias.numpy().copy()


def _flat_state(tr):
    st = tr.state
    return [np.concatenate([st[s]["conv6_cls.kernel"].reshape(-1), st[s]["conv6_cls.bias"]]) for s in ("m", "v")]


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
def test_images_raw_equals_features_raw_and_composition(icnet19, u8):
    """step(images, images_raw=...) == step_features(features(images), features_raw=features(images_raw)) bit for bit, and both
    equal the composed step; images_raw is images == no raw side"""
    x, x_raw, labels, mask, sel = _frames_case(u8)
    nets = [_twin(icnet19) for _ in range(3)]
    tr_a, tr_b = (SemiSupervisedICNetHeadTrainer(n, **HYPER) for n in nets[:2])
    tr_c = ICNetHeadTrainer(nets[2], **HYPER)
    for tr in (tr_a, tr_b, tr_c):
        tr.reinitialize(seed=4)
    thr = _frame_threshold(nets[2], x_raw, "margin")
    feats, feats_raw = tr_b.features(x), tr_b.features(x_raw)
    assert not torch.equal(feats, feats_raw)
    conf = [torch.zeros((19, 19), dtype=torch.int64, device="cuda") for _ in range(3)]
    for step in range(2):
        la, ppa = tr_a.step(x, labels, mask, labelled=sel, measure="margin", threshold=thr, images_raw=x_raw,
                            confusion=conf[0], return_pseudo_pixels=True)
        lb, ppb = tr_b.step_features(feats, labels, mask, labelled=sel, measure="margin", threshold=thr,
                                     features_raw=feats_raw, confusion=conf[1], return_pseudo_pixels=True)
        lc, ppc = _composed_step(nets[2], tr_c, x, x_raw, labels, mask, sel, "margin", thr, conf[2])
        print("step %d: loss %.17g / %.17g / %.17g, pseudo pixels %s" % (step, float(la), float(lb), float(lc), ppa.tolist()))
        assert float(la).hex() == float(lb).hex() == float(lc).hex(), "loss differs at step %d" % step
        for other in nets[1:]:
            assert all(np.array_equal(a, b) for a, b in zip(_head_of(nets[0]), _head_of(other))), "head differs at step %d" % step
        assert torch.equal(ppa, ppb) and torch.equal(ppa, ppc) and ppa[0].item() == 0 and 0 < ppa[1].item() < 64 * 128
        assert torch.equal(conf[0], conf[1]) and torch.equal(conf[0], conf[2])
    net_d, net_e = _twin(icnet19), _twin(icnet19)
    tr_d, tr_e = SemiSupervisedICNetHeadTrainer(net_d, **HYPER), SemiSupervisedICNetHeadTrainer(net_e, **HYPER)
    ld = tr_d.step(x, labels, mask, labelled=sel, threshold=0.3, images_raw=x)
    le = tr_e.step(x, labels, mask, labelled=sel, threshold=0.3)
    assert float(ld).hex() == float(le).hex() and all(np.array_equal(a, b) for a, b in zip(_head_of(net_d), _head_of(net_e)))


def test_twin_nets_ten_steps(icnet19):
    """ten fused steps on one net, ten composed steps on its twin (mixed `labelled`, images_raw given): kernel, bias, m, v,
    loss, confusion and pseudo pixels equal after every step; afterwards the score planes of both nets agree"""
    x, x_raw, labels, mask, sel = _frames_case()
    net_a, net_b = _twin(icnet19), _twin(icnet19)
    tr_a, tr_b = SemiSupervisedICNetHeadTrainer(net_a, **HYPER), ICNetHeadTrainer(net_b, **HYPER)
    tr_a.reinitialize(seed=5)
    tr_b.reinitialize(seed=5)
    thr = _frame_threshold(net_b, x_raw, "entropy")
    conf_a = torch.zeros((19, 19), dtype=torch.int64, device="cuda")
    conf_b = torch.zeros_like(conf_a)
    for step in range(10):
        la, ppa = tr_a.step(x, labels, mask, labelled=sel, measure="entropy", threshold=thr, images_raw=x_raw,
                            confusion=conf_a, return_pseudo_pixels=True)
        lb, ppb = _composed_step(net_b, tr_b, x, x_raw, labels, mask, sel, "entropy", thr, conf_b)
        print("step %d: loss %.17g / %.17g, pseudo pixels %s (%.3f of the frame)"
              % (step, float(la), float(lb), ppa.tolist(), ppa[1].item() / (64 * 128)))
        assert float(la).hex() == float(lb).hex(), "loss differs at step %d" % step
        assert all(np.array_equal(a, b) for a, b in zip(_head_of(net_a), _head_of(net_b))), "head differs at step %d" % step
        assert all(np.array_equal(a, b) for a, b in zip(_flat_state(tr_a), _flat_state(tr_b))), "Adam slots differ at step %d" % step
        assert torch.equal(ppa, ppb) and ppa[0].item() == 0
        assert torch.equal(conf_a, conf_b), "confusion differs at step %d" % step
    assert tr_a.state["t"] == tr_b.state["t"] == 10 and int(conf_a.sum()) > 0
    s_a, e_a = net_a.score(x, return_label=True, return_mask=True, return_confidence=True)
    s_b, e_b = net_b.score(x, return_label=True, return_mask=True, return_confidence=True)
    assert torch.equal(s_a, s_b)
    for key in ("label", "mask", "confidence"):
        assert torch.equal(e_a[key], e_b[key]), key


def test_determinism_and_bookkeeping():
    """two calls give the same bits; the confusion matrix accumulates across two calls; labelled images get 0 pseudo pixels;
    a call with no semi keyword gives ICNetHeadTrainer's bits"""
    k, labelled = 19, [0, 1]
    x, head, labels, mask = _case(9200, 2, 3, 5, k, labelled)
    x2 = (x * 1.1).contiguous()
    tr0 = ICNetHeadTrainer(_shared_net(k), 1e-3, loginverse_scaling=1.02, label_smoothing=0.1)
    tr1 = SemiSupervisedICNetHeadTrainer(_shared_net(k), 1e-3, loginverse_scaling=1.02, label_smoothing=0.1)
    thr = _median_threshold(x2, head, k, "entropy", labelled)
    a = _fused(k, tr1, x, x2, head, labels, mask, labelled, "entropy", thr)
    b = _fused(k, tr1, x, x2, head, labels, mask, labelled, "entropy", thr)
    _assert_same("second call", b, a)
    assert a[3][1].item() == 0 and a[3][0].item() > 0
    conf = a[2].clone()
    tr1.gradient_features(x, labels, mask, params=_params(head, k), labelled=labelled, threshold=thr, features_raw=x2,
                          confusion=conf)
    assert torch.equal(conf, 2 * a[2]) and int(a[2].sum()) > 0
    xl, _, labels_l, mask_l = _case(9201, 2, 3, 5, k, [1, 1])
    l0, g0 = tr0.gradient_features(xl, labels_l, mask_l, params=_params(head, k), max_workgroups=1)
    l1, g1 = tr1.gradient_features(xl, labels_l, mask_l, params=_params(head, k), max_workgroups=1)
    assert torch.equal(l0, l1) and torch.equal(_pack(g0), _pack(g1))
    l2, g2 = tr1.gradient_features(xl, labels_l, mask_l, params=_params(head, k), max_workgroups=1,
                                   labelled=torch.ones(2, dtype=torch.bool))
    assert torch.equal(l0, l2) and torch.equal(_pack(g0), _pack(g2))
