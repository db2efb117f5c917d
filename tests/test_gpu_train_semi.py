"""The semi-supervised output-layer step on the MI355X: pseudo annotation and training metrics inside
the head-gradient kernel, against the COMPOSITION of the parent API -- score with label + mask planes, training_targets,
the plain gradient / step, the stand-alone confusion op.  The logits, pixel_score and the gradient arithmetic are the same
code in both routes, so loss and gradient are compared bit for bit and the counts exactly."""
import itertools

import numpy as np
import pytest
import torch

import semanticsegmentationactivelearning_amd as ssal
from semanticsegmentationactivelearning_amd import _lib
from semanticsegmentationactivelearning_amd import active_learning as al
from semanticsegmentationactivelearning_amd import synthetic as syn
from semanticsegmentationactivelearning_amd.tensortools import metrics
from semanticsegmentationactivelearning_amd.training import FinalLayerTrainer

from helpers import make_model

pytestmark = pytest.mark.gpu

MEASURES = ("entropy", "margin", "confidence")
_NETS = {}


def _plain_net(k):
    """an ENet(k) whose Final layer serves as the composition's logits op (the trunk is not used)"""
    if k not in _NETS:
        net = ssal.ENet(k)
        net.build((None, None, None, 3))
        _NETS[k] = net
    return _NETS[k]


def _case(seed, n, h, w, k, labelled, gain=0.3):
    """features, kernel and annotation on the device; the planes of unlabelled images hold 0xFF labels and NaN masks"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, h, w, 16)) * 0.7).astype(np.float32)
    kern = rng.uniform(-gain, gain, (3, 3, k, 16)).astype(np.float32)
    labels = rng.integers(0, k, (n, 2 * h, 2 * w)).astype(np.uint8)
    mask = (rng.uniform(size=(n, 2 * h, 2 * w)) > 0.25).astype(np.float32)
    labels[rng.uniform(size=labels.shape) < 0.05] = 255  # ignored pixels under both mask values
    for i, l in enumerate(labelled):
        if not l:
            labels[i] = 0xFF
            mask[i] = np.nan
    return tuple(torch.as_tensor(a).cuda() for a in (x, kern, labels, mask))


def _quantile(plane, q):
    v = plane.flatten()
    v = v[:: max(1, v.numel() // 1000003) | 1].float().cpu().numpy()  # an odd stride: every quad position is sampled
    return float(np.quantile(v, q))


def _pseudo_planes(net, feats_raw, kern, measure, threshold=None, q=0.5):
    """the parent route to the pseudo annotation of materialised features: the Final layer alone, then score_logits.
    threshold None: the q-quantile of the case's confidence plane"""
    net.Final.kernel.assign(kern.cpu().numpy())
    logits = net.Final(feats_raw, training=False)
    if threshold is None:
        _, p = al.score_logits(logits, measure, 0.0, return_confidence=True)
        threshold = _quantile(p["confidence"], q)
    _, p = al.score_logits(logits, measure, threshold, return_label=True, return_mask=True)
    return p["label"], p["mask"], threshold


def _composed_features(k, tr, feats, feats_raw, kern, labels, mask, labelled, measure, threshold=None, q=0.5):
    """(loss, grad, confusion, pseudo_pixels, threshold) of the composed step"""
    net = _plain_net(k)
    sel = torch.as_tensor(np.asarray(labelled, dtype=bool)).cuda()
    pl, pm, threshold = _pseudo_planes(net, feats_raw, kern, measure, threshold, q)
    lab, mk = al.training_targets(sel, labels, mask, pl, pm.float())
    loss, grad = tr.gradient_features(feats, lab, mk, kernel=kern)
    _, p = al.score_logits(net.Final(feats, training=False), "confidence", 0.0, return_label=True)  # first maximum
    conf = metrics.confusion_mat(lab, p["label"], k, weights=mk)
    pp = pm.to(torch.int64).sum(dim=(1, 2)) * (~sel).to(torch.int64)
    return loss, grad, conf, pp, threshold


def _assert_same(name, got, want):
    loss, grad, conf, pp = got
    wloss, wgrad, wconf, wpp = want
    assert loss.cpu().numpy().tobytes() == wloss.cpu().numpy().tobytes(), "%s: loss %r != %r" % (
        name, float(loss.cpu()[0]), float(wloss.cpu()[0]))
    d = (grad != wgrad) & ~(torch.isnan(grad) & torch.isnan(wgrad))
    assert not bool(d.any()), "%s: %d of %d gradient entries differ (max |d| %.3e)" % (
        name, int(d.sum()), d.numel(), float((grad - wgrad).abs().max()))
    assert np.array_equal(grad.cpu().numpy().view(np.uint32), wgrad.cpu().numpy().view(np.uint32)), name + ": gradient bits"
    assert torch.equal(conf, wconf), "%s: confusion differs in %d entries" % (name, int((conf != wconf).sum()))
    assert torch.equal(pp, wpp), "%s: pseudo pixels %s != %s" % (name, pp.tolist(), wpp.tolist())


def _fused_features(tr, feats, feats_raw, kern, labels, mask, labelled, measure, threshold, k):
    conf = torch.zeros((k, k), dtype=torch.int64, device=feats.device)
    loss, grad, pp = tr.gradient_features(feats, labels, mask, kernel=kern, labelled=labelled, measure=measure,
                                          threshold=threshold, features_raw=feats_raw, confusion=conf,
                                          return_pseudo_pixels=True)
    return loss, grad, conf, pp


PATTERNS = {(1, 33, 65): {"none": [0], "all": [1]}, (3, 20, 17): {"none": [0, 0, 0], "all": [1, 1, 1], "mixed": [1, 0, 1],
                                                                   "mixed2": [0, 1, 0]}}


@pytest.mark.parametrize("k", (2, 6, 19, 32))
@pytest.mark.parametrize("measure", MEASURES)
def test_feature_entry_matches_composition(k, measure):
    """1: bitwise loss and gradient, exact confusion matrix and pseudo-pixel counts; weight 0 / 1.02, label smoothing 0 / 0.1,
    shapes that are not whole tiles, every `labelled` pattern, thresholds at the median confidence of the case"""
    seed = 1000 * k + 10 * MEASURES.index(measure)
    for (weight, ls), (shape, pats) in itertools.product(((0.0, 0.0), (1.02, 0.0), (0.0, 0.1), (1.02, 0.1)), PATTERNS.items()):
        tr = FinalLayerTrainer(_plain_net(k), 1e-3, loginverse_scaling=weight, label_smoothing=ls)
        for pname, labelled in pats.items():
            seed += 1
            n, h, w = shape
            x, kern, labels, mask = _case(seed, n, h, w, k, labelled)
            want = _composed_features(k, tr, x, x, kern, labels, mask, labelled, measure)
            thr = want[4]
            got = _fused_features(tr, x, None, kern, labels, mask, np.asarray(labelled, np.uint8), measure, thr, k)
            share = float(want[3].sum()) / max(1, (n - sum(labelled)) * 4 * h * w)
            name = "K=%d %s w=%g ls=%g %dx%dx%d labelled=%s" % (k, measure, weight, ls, n, h, w, pname)
            print("%s: threshold %.6g, share of mask-1 pixels in unlabelled images %.3f, loss %.9g, confusion sum %d"
                  % (name, thr, share, float(got[0].cpu()[0]), int(got[2].sum())))
            if sum(labelled) < n:
                assert 0.2 < share < 0.8, name + ": the threshold does not give a mixed mask"
            _assert_same(name, got, want[:4])


def test_all_labelled_is_todays_gradient_and_confusion_alone():
    """2: `labelled` all ones, no extras: the bits of today's gradient_features; labelled=None with a confusion: the same
    bits plus the right matrix"""
    k = 19
    tr = FinalLayerTrainer(_plain_net(k), 1e-3, loginverse_scaling=1.02, label_smoothing=0.1)
    x, kern, labels, mask = _case(77, 3, 20, 17, k, [1, 1, 1])
    l0, g0 = tr.gradient_features(x, labels, mask, kernel=kern)
    l1, g1 = tr.gradient_features(x, labels, mask, kernel=kern, labelled=torch.ones(3, dtype=torch.bool))
    assert torch.equal(l0, l1) and torch.equal(g0, g1)
    conf = torch.zeros((k, k), dtype=torch.int64, device="cuda")
    l2, g2 = tr.gradient_features(x, labels, mask, kernel=kern, confusion=conf)
    assert torch.equal(l0, l2) and torch.equal(g0, g2)
    net = _plain_net(k)
    net.Final.kernel.assign(kern.cpu().numpy())
    _, p = al.score_logits(net.Final(x, training=False), "confidence", 0.0, return_label=True)
    want = metrics.confusion_mat(labels, p["label"], k, weights=mask)
    assert torch.equal(conf, want) and int(conf.sum()) > 0
    # labels / mask may be None when no image is labelled
    l3, g3, pp = tr.gradient_features(x, None, None, kernel=kern, labelled=[0, 0, 0], threshold=-1.0, return_pseudo_pixels=True)
    assert pp.tolist() == [4 * 20 * 17] * 3 and bool(torch.isfinite(g3).all())


@pytest.mark.parametrize("measure", MEASURES)
def test_raw_features_differ_from_training_features(measure):
    """3 (features): the pseudo annotation comes from features_raw, the gradient from the (distorted) training features"""
    k, labelled = 19, [0, 1, 0]
    tr = FinalLayerTrainer(_plain_net(k), 1e-3, loginverse_scaling=1.02)
    x_raw, kern, labels, mask = _case(31 + MEASURES.index(measure), 3, 20, 17, k, labelled)
    scale = torch.linspace(0.8, 1.25, 16, device="cuda")
    x = (x_raw * scale).contiguous()
    want = _composed_features(k, tr, x, x_raw, kern, labels, mask, labelled, measure)
    got = _fused_features(tr, x, x_raw, kern, labels, mask, labelled, measure, want[4], k)
    _assert_same("features_raw " + measure, got, want[:4])
    one_pass = _fused_features(tr, x, None, kern, labels, mask, labelled, measure, want[4], k)
    assert not torch.equal(one_pass[1], got[1]), "the raw features made no difference: the case shows nothing"
    same = _fused_features(tr, x, x, kern, labels, mask, labelled, measure, want[4], k)
    _assert_same("features_raw is features", same, one_pass)
    clone = _fused_features(tr, x, x.clone(), kern, labels, mask, labelled, measure, want[4], k)
    _assert_same("features_raw == features (a copy: the two-pass kernel path)", clone, one_pass)


HYPER = dict(learning_rate=5e-4, beta1=0.9, beta2=0.99, loginverse_scaling=1.02, l2=2e-4)


def _twin_nets():
    a, _ = make_model(19, 3, seed=0)
    b, _ = make_model(19, 3, seed=0)
    return a, b


def _frames_case():
    x = syn.synth_frames_device(0, 2, 64, 128, 3)
    rng = np.random.default_rng(21)
    labels = rng.integers(0, 19, (2, 64, 128)).astype(np.uint8)
    mask = (rng.uniform(size=(2, 64, 128)) > 0.2).astype(np.float32)
    labels[1], mask[1] = 0xFF, np.nan  # image 1 is unlabelled
    return x, torch.as_tensor(labels).cuda(), torch.as_tensor(mask).cuda(), torch.tensor([True, False]).cuda()


def _composed_step(net, tr, x, x_raw, labels, mask, sel, measure, thr, conf=None):
    _, p = net.score(x_raw, measure, thr, return_label=True, return_mask=True)
    lab, mk = al.training_targets(sel, labels, mask, p["label"], p["mask"].float())
    if conf is not None:
        _, pt = net.score(x, "confidence", 0.0, return_label=True)
        metrics.confusion_mat(lab, pt["label"], net.classes, weights=mk, out=conf)
    pp = p["mask"].to(torch.int64).sum(dim=(1, 2)) * (~sel).to(torch.int64)
    return tr.step(x, lab, mk), pp


def test_image_entry_end_to_end_twenty_steps():
    """4: 20 fused steps on one net, 20 composed steps on its twin: kernel, m, v and loss bitwise equal after every step,
    the confusion matrices and pseudo-pixel counts too; then net.score of both agrees (the handle refresh still works)"""
    net_a, net_b = _twin_nets()
    x, labels, mask, sel = _frames_case()
    tr_a, tr_b = FinalLayerTrainer(net_a, **HYPER), FinalLayerTrainer(net_b, **HYPER)
    tr_a.reinitialize(seed=5)
    tr_b.reinitialize(seed=5)
    _, p = net_b.score(x, "entropy", 0.0, return_confidence=True)
    thr = _quantile(p["confidence"][1], 0.5)
    conf_a = torch.zeros((19, 19), dtype=torch.int64, device="cuda")
    conf_b = torch.zeros_like(conf_a)
    for step in range(20):
        la, ppa = tr_a.step(x, labels, mask, labelled=sel, measure="entropy", threshold=thr, confusion=conf_a,
                            return_pseudo_pixels=True)
        lb, ppb = _composed_step(net_b, tr_b, x, x, labels, mask, sel, "entropy", thr, conf_b)
        sa, sb = tr_a.state, tr_b.state
        print("step %2d: loss %.12g / %.12g, pseudo pixels %s (%.3f of the frame)"
              % (step, float(la), float(lb), ppa.tolist(), ppa[1].item() / (64 * 128)))
        assert float(la).hex() == float(lb).hex(), "loss differs at step %d" % step
        assert np.array_equal(net_a.Final.kernel.numpy(), net_b.Final.kernel.numpy()), "kernel differs at step %d" % step
        assert np.array_equal(sa["m"], sb["m"]) and np.array_equal(sa["v"], sb["v"]), "Adam slots differ at step %d" % step
        assert torch.equal(ppa, ppb) and ppa[0].item() == 0
        assert torch.equal(conf_a, conf_b), "confusion differs at step %d" % step
    assert 0 < ppa[1].item() < 64 * 128
    s_a, e_a = net_a.score(x, return_label=True)
    s_b, e_b = net_b.score(x, return_label=True)
    assert torch.equal(s_a, s_b) and torch.equal(e_a["label"], e_b["label"])


def test_images_raw_against_composition():
    """3 (images): images_raw differing from the training frames (a channel-scaled copy, as InputStage's image_dist);
    images_raw is images == images_raw=None"""
    net_a, net_b = _twin_nets()
    x_raw, labels, mask, sel = _frames_case()
    x = (x_raw * torch.tensor([0.9, 1.1, 0.8], device="cuda")).contiguous()
    tr_a, tr_b = FinalLayerTrainer(net_a, **HYPER), FinalLayerTrainer(net_b, **HYPER)
    _, p = net_b.score(x_raw, "margin", 0.0, return_confidence=True)
    thr = _quantile(p["confidence"][1], 0.5)
    for step in range(3):
        la, ppa = tr_a.step(x, labels, mask, labelled=sel, measure="margin", threshold=thr, images_raw=x_raw,
                            return_pseudo_pixels=True)
        lb, ppb = _composed_step(net_b, tr_b, x, x_raw, labels, mask, sel, "margin", thr)
        assert float(la).hex() == float(lb).hex(), "loss differs at step %d" % step
        assert np.array_equal(net_a.Final.kernel.numpy(), net_b.Final.kernel.numpy()), "kernel differs at step %d" % step
        assert torch.equal(ppa, ppb)
    net_c, net_d = _twin_nets()
    tr_c, tr_d = FinalLayerTrainer(net_c, **HYPER), FinalLayerTrainer(net_d, **HYPER)
    lc = tr_c.step(x, labels, mask, labelled=sel, threshold=0.3, images_raw=x)
    ld = tr_d.step(x, labels, mask, labelled=sel, threshold=0.3)
    assert float(lc).hex() == float(ld).hex() and np.array_equal(net_c.Final.kernel.numpy(), net_d.Final.kernel.numpy())
    # the image form's workspace with the raw slot: larger by at least the raw features
    L = _lib.lib()
    h_ = tr_c._trunk_handle()
    q = L.ssal_enet_train_final_semi_workspace_bytes
    assert q(h_, 2, 64, 128, 1) - q(h_, 2, 64, 128, 0) >= 2 * 32 * 64 * 16 * 4
    assert q(h_, 2, 64, 128, 0) >= L.ssal_enet_train_final_workspace_bytes(h_, 2, 64, 128)


def test_determinism_and_accumulation():
    """5: two calls give the same bits, the confusion matrix included; two calls into one matrix give twice one call"""
    k, labelled = 19, [0, 1, 0]
    tr = FinalLayerTrainer(_plain_net(k), 1e-3, loginverse_scaling=1.02, label_smoothing=0.1)
    x, kern, labels, mask = _case(55, 3, 20, 17, k, labelled)
    x2 = (x * 1.1).contiguous()
    a = _fused_features(tr, x, x2, kern, labels, mask, labelled, "entropy", 0.2, k)
    b = _fused_features(tr, x, x2, kern, labels, mask, labelled, "entropy", 0.2, k)
    _assert_same("second call", b, a)
    conf = a[2].clone()
    tr.gradient_features(x, labels, mask, kernel=kern, labelled=labelled, threshold=0.2, features_raw=x2, confusion=conf)
    assert torch.equal(conf, 2 * a[2]) and int(a[2].sum()) > 0


def test_full_size_batch_matches_composition():
    """6: 8 x 512 x 1024 features, K = 19, entropy, four images unlabelled"""
    k, labelled = 19, [1, 0, 1, 0, 0, 1, 0, 1]
    tr = FinalLayerTrainer(_plain_net(k), 1e-3, loginverse_scaling=1.02)
    x, kern, labels, mask = _case(7, 8, 512, 1024, k, labelled)
    want = _composed_features(k, tr, x, x, kern, labels, mask, labelled, "entropy")
    got = _fused_features(tr, x, None, kern, labels, mask, labelled, "entropy", want[4], k)
    print("full size: threshold %.6g, pseudo pixels %s, loss %.12g" % (want[4], got[3].tolist(), float(got[0].cpu()[0])))
    _assert_same("full size", got, want[:4])


def test_invalid_arguments():
    """7: Python exceptions and C statuses with their messages"""
    k = 19
    net = _plain_net(k)
    tr = FinalLayerTrainer(net, 1e-3)
    x = torch.zeros((2, 8, 8, 16), device="cuda")
    lab = torch.zeros((2, 16, 16), dtype=torch.uint8, device="cuda")
    msk = torch.ones((2, 16, 16), device="cuda")
    with pytest.raises(NotImplementedError, match="Uncertainty function not implemented."):
        tr.gradient_features(x, lab, msk, labelled=[0, 1], measure="bald")
    with pytest.raises(ValueError, match="labelled"):
        tr.gradient_features(x, lab, msk, labelled=torch.ones(3, device="cuda"))
    with pytest.raises(ValueError, match="features_raw"):
        tr.gradient_features(x, lab, msk, labelled=[0, 1], features_raw=torch.zeros((2, 8, 4, 16), device="cuda"))
    with pytest.raises(ValueError, match="confusion"):
        tr.gradient_features(x, lab, msk, confusion=torch.zeros((k, k), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="None only"):
        tr.gradient_features(x, None, None, labelled=torch.tensor([0, 1], device="cuda"))
    with pytest.raises(ValueError, match="images_raw"):
        tr.step(torch.zeros((2, 16, 16, 3), device="cuda"), lab, msk, labelled=[0, 1],
                images_raw=torch.zeros((2, 16, 8, 3), device="cuda"))
    L = _lib.lib()
    p = _lib.dev_ptr(x)
    loss = torch.zeros(1, dtype=torch.float64, device="cuda")
    grad = torch.zeros((3, 3, k, 16), device="cuda")
    ws = torch.zeros(int(L.ssal_final_grad_semi_workspace_bytes(2, 8, 8, k)), dtype=torch.uint8, device="cuda")
    lbd = torch.zeros(2, dtype=torch.uint8, device="cuda")

    def call(classes=k, measure=0, labels=_lib.dev_ptr(lab), labelled=_lib.dev_ptr(lbd), ws_bytes=ws.numel()):
        return L.ssal_final_grad_semi_nhwc(p, None, 2, 8, 8, classes, _lib.dev_ptr(grad), labels,
                                           _lib.dev_ptr(msk) if labels else None, labelled, measure, 0.5, 0.0, 0.0,
                                           _lib.dev_ptr(loss), _lib.dev_ptr(grad), None, None, _lib.dev_ptr(ws), ws_bytes,
                                           _lib.stream_ptr())

    assert call() == _lib.SSAL_OK
    assert call(labels=None) == _lib.SSAL_OK  # no image labelled: the planes may be NULL
    assert call(classes=33) == _lib.SSAL_EINVAL and b"classes must be in [2,32]" in L.ssal_last_error()
    assert call(measure=3) == _lib.SSAL_ENOTIMPL and b"Uncertainty function not implemented" in L.ssal_last_error()
    assert call(labels=None, labelled=None) == _lib.SSAL_EINVAL and b"may be NULL only" in L.ssal_last_error()
    assert call(ws_bytes=ws.numel() - 1) == _lib.SSAL_ENOMEM and b"workspace too small" in L.ssal_last_error()
    h_ = net._sync_handle()
    big = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    xi = torch.zeros((2, 16, 16, 3), device="cuda")
    rc = L.ssal_enet_train_final_semi_nhwc(h_, _lib.dev_ptr(xi), None, 0, 2, 16, 16, _lib.dev_ptr(lab), _lib.dev_ptr(msk),
                                           _lib.dev_ptr(lbd), 0, 0.5, _lib.dev_ptr(grad), 0.0, 0.0, _lib.dev_ptr(loss),
                                           _lib.dev_ptr(grad), None, None, _lib.dev_ptr(big), 1024, _lib.stream_ptr())
    assert rc == _lib.SSAL_ENOMEM
    rc = L.ssal_enet_train_final_semi_nhwc(h_, _lib.dev_ptr(xi), None, 0, 2, 16, 12, _lib.dev_ptr(lab), _lib.dev_ptr(msk),
                                           _lib.dev_ptr(lbd), 0, 0.5, _lib.dev_ptr(grad), 0.0, 0.0, _lib.dev_ptr(loss),
                                           _lib.dev_ptr(grad), None, None, _lib.dev_ptr(big), big.numel(), _lib.stream_ptr())
    assert rc == _lib.SSAL_EINVAL  # W not divisible by 8
    torch.cuda.synchronize()
