"""Every class count of the K-templated kernel families on the MI355X ("Class-count coverage"): each family below is
compiled once per K = 2 .. 32, and each test here runs all 31 instantiations at the smallest shape that still crosses a tile
boundary and a batch boundary, against the reference the family's own test file uses, under that file's tolerance.  The inputs
come from class_count_cases.py, whose reference side test_class_counts_cpu.py checks on the host.

  SSAL_SL    k_score_logits              al.score_logits against the C oracle
  SSAL_US    k_upscore                   cops.upscore_logits against resize_bilinear + the C oracle's score
  SSAL_FS    k_final_score<K, .>         net(x), net.score(x, return_label / return_confidence) against the C oracle
  SSAL_FS51  k_final_score<K, false, true>  the score-only pass with Bottleneck5_1 inside (fuse_ends = 3)
  SSAL_FE    k_final_score<K, ., ., true>   net.evaluate, with Bottleneck5_1 inside (fuse_ends = 3) and without (0)
  SSAL_XE    k_masked_xent               losses.masked_softmax_cross_entropy against the float64 restatement
  SSAL_FG    k_final_grad<K, false / true>  FinalLayerTrainer.gradient_features against float64, and fused against composed
  SSAL_TB    k_tb_head<K, false / true>, the target-only launch  LastBlockTrainer / SemiSupervisedBlockTrainer likewise
  SSAL_IH    k_icnet_head_grad           ICNetHeadTrainer.gradient_features against float64

The block head's data: class_count_cases.BLOCK_SEED = 300, the first seed >= 300 by the recipe of test_gpu_train_decoder.py;
its PReLU margin is 139.8 on the search host and 252.2 on the MI355X host (float64 against float32 torch on the CPU, the GPU
plays no part; asserted > 16 here and in test_class_counts_cpu.py).
Each test prints its worst error / bound ratio for its K; the last test checks that every family met all 31 class counts."""
import numpy as np
import pytest
import torch

import semanticsegmentationactivelearning_amd as ssal
from oracle import enet_oracle as orc
from oracle import icnet_oracle as ico
from semanticsegmentationactivelearning_amd import _lib, active_learning as al
from semanticsegmentationactivelearning_amd.models.util import conv_ops as cops
from semanticsegmentationactivelearning_amd.tensortools import losses, metrics
from semanticsegmentationactivelearning_amd.training import (FinalLayerTrainer, ICNetHeadTrainer, LastBlockTrainer,
                                                             SemiSupervisedBlockTrainer)

import class_count_cases as cc
import final_train_oracle as fto
import icnet_head_train_oracle as iho
import last_block_train_oracle as lbo
import test_gpu_train_deep_semi as deep_semi
import test_gpu_train_icnet_head as icnet_head
import test_gpu_train_semi as semi
from helpers import frames, make_model, report_diff
from test_gpu_parity import TOL

pytestmark = pytest.mark.gpu

KS = pytest.mark.parametrize("k", cc.CLASS_COUNTS)
FAMILIES = ("SL", "US", "FS", "FS51", "FE", "XE", "FG", "TB", "FG<semi>", "TB<semi>", "TB<target-only>", "IH")
RAN = {f: set() for f in FAMILIES}  # family -> the class counts whose case ran to its end


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    _lib.lib()  # the HIP extension must be the thing that runs
    yield
    torch.cuda.synchronize()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ran(k, *families):
    for f in families:
        RAN[f].add(k)


def _check_scores(tag, scores, extra, want_mean, want_conf, want_label):
    """labels bit-exact, confidence within TOL, means within 1e-6 -> the worst error / bound ratio"""
    report_diff(tag + " label (bit-exact argmax)", extra["label"].cpu().numpy(), want_label)
    conf = extra["confidence"].cpu().numpy()
    report_diff(tag + " confidence", conf, want_conf, exact=False, atol=TOL)
    report_diff(tag + " mean", scores.cpu().numpy(), want_mean, exact=False, atol=1e-6)
    return max(float(np.abs(conf - want_conf).max()) / TOL, float(np.abs(scores.cpu().numpy() - want_mean).max()) / 1e-6)


# ---- scores of materialised logits ---------------------------------------------------------------------------------------
@KS
def test_score_logits_every_class_count(k):
    """SSAL_SL: logits 2 x 3 x 5 x K, the three measures, the assertions of test_score_logits_kernel"""
    lg = cc.sweep_logits(k)
    worst = 0.0
    for measure in cc.MEASURES:
        want_mean, want_conf, want_label = orc.score_logits(lg, measure)
        thr = float(np.median(want_conf))
        scores, extra = al.score_logits(dev(lg), measure, threshold=thr, return_label=True, return_mask=True,
                                        return_confidence=True)
        worst = max(worst, _check_scores("K=%d %s" % (k, measure), scores, extra, want_mean, want_conf, want_label))
        conf, mask = extra["confidence"].cpu().numpy(), extra["mask"].cpu().numpy()
        assert (mask == (conf >= np.float32(thr))).all()  # active_learning.py:265-269 on the kernel's own confidence
        assert torch.equal(scores, al.score_logits(dev(lg), measure))  # the launch without per-pixel outputs
    print("SL K=%d: worst error / bound %.3e" % (k, worst))
    _ran(k, "SL")


@KS
def test_upscore_every_class_count(k):
    """SSAL_US: logits 2 x 3 x 5 x K at a quarter of the resolution, the three measures, the assertions of test_upscore_kernel"""
    lq = cc.sweep_logits(k)
    full = ico.resize_bilinear(lq, 12, 20)
    worst = 0.0
    for measure in cc.MEASURES:
        want_mean, want_conf, want_label = orc.score_logits(full, measure)
        thr = float(np.median(want_conf))
        s, e = cops.upscore_logits(dev(lq), measure, threshold=thr, return_label=True, return_mask=True,
                                   return_confidence=True)
        worst = max(worst, _check_scores("K=%d %s" % (k, measure), s, e, want_mean, want_conf, want_label))
        assert (e["mask"].cpu().numpy() == (e["confidence"].cpu().numpy() >= np.float32(thr))).all()
        assert torch.equal(s, cops.upscore_logits(dev(lq), measure))  # the score-only launch gives the same means
    print("US K=%d: worst error / bound %.3e" % (k, worst))
    _ran(k, "US")


# ---- ENet's Final layer in its three fused forms -----------------------------------------------------------------------------
@KS
def test_enet_final_score_and_evaluate_every_class_count(k):
    """SSAL_FS, SSAL_FS51, SSAL_FE: make_model(K, 3, seed=K) on 2 frames of 16 x 24.  Logits bit-exact against the C oracle;
    labels, confidences and means against orc.score_images as in test_forward_and_score_other_class_counts, for the score-only
    call too; the confusion matrix of net.evaluate equal to metrics.confusion_mat of the oracle's labels; all of it with
    fuse_ends = 0 and 3, whose results are the same bits"""
    net, P = make_model(k, 3, seed=k)
    x = frames([60, 61], 16, 24, 3)
    xd = dev(x)
    want = {m: orc.score_images(P, x, m) for m in cc.MEASURES}
    want_logits, want_label = want["entropy"][3], want["entropy"][2]
    rng = np.random.default_rng(6100 + k)
    lab = rng.integers(0, k, size=(2, 16, 24), dtype=np.uint8)
    lab[rng.random(lab.shape) < 0.1] = 255
    lab[0, :4] = want_label[0, :4]  # a band on the diagonal
    mask = (lab != 255).astype(np.uint8)
    want_conf_mat = metrics.confusion_mat(dev(lab), dev(want_label), k, weights=dev(mask))
    got, worst = {}, 0.0
    try:
        for fuse in (0, 3):
            _lib.set_knob("fuse_ends", fuse)
            logits = net(xd, training=False)
            report_diff("K=%d fuse_ends=%d logits (bit-exact)" % (k, fuse), logits.cpu().numpy(), want_logits)
            got[fuse] = [logits]
            for m in cc.MEASURES:
                tag = "K=%d fuse_ends=%d %s" % (k, fuse, m)
                alone = net.score(xd, m)  # fuse_ends = 3: Bottleneck5_1 inside the Final + score kernel
                scores, extra = net.score(xd, m, return_label=True, return_confidence=True)
                want_mean, want_c, want_l, _ = want[m]
                worst = max(worst, _check_scores(tag, scores, extra, want_mean, want_c, want_l))
                report_diff(tag + " mean (score only)", alone.cpu().numpy(), want_mean, exact=False, atol=1e-6)
                assert torch.equal(alone, scores), tag + ": the score-only call differs from the call with planes"
                got[fuse] += [alone, scores, extra["label"], extra["confidence"]]
            ev = net.evaluate(xd, dev(lab), dev(mask))
            assert torch.equal(ev, want_conf_mat), "K=%d fuse_ends=%d: evaluate differs from the oracle's labels" % (k, fuse)
            assert int(ev.sum()) == int(mask.sum()) and int(torch.diagonal(ev).sum()) >= int(mask[0, :4].sum())
            got[fuse].append(ev)
    finally:
        _lib.set_knob("fuse_ends", 3)
    for a, b in zip(got[0], got[3]):
        assert torch.equal(a, b), "K=%d: fuse_ends = 0 and 3 give different bits" % k
    print("FS / FS51 / FE K=%d: worst error / bound %.3e" % (k, worst))
    _ran(k, "FS", "FS51", "FE")


# ---- the loss op -----------------------------------------------------------------------------------------------------------
@KS
def test_loss_op_every_class_count(k):
    """SSAL_XE: logits 2 x 6 x 10 x K, label 255 under both mask values and one label == K under mask 1, against the float64
    restatement sum(pixel_loss) x mask_scale of final_train_oracle; the bound is test_masked_softmax_cross_entropy_forward's
    against its oracle, 1e-5 max(1, |want|) (its bound against its own float64 statement, 2e-5, is the wider of its two)"""
    lg, labels, mask = cc.loss_case(k)
    lg64, mk64 = torch.as_tensor(lg.astype(np.float64)), torch.as_tensor(mask.astype(np.float64))
    worst = 0.0
    for weight, ls in cc.LOSSES:
        on, off, w32, c_w = fto.xent_constants(k, weight, ls)
        want = float(fto.pixel_loss(lg64, fto.one_hot(labels, k, on, off), mk64, w32, c_w).sum()) * fto.mask_scale(mask)
        got = float(losses.masked_softmax_cross_entropy(dev(labels), dev(lg), dev(mask), k, weight, ls))
        bound = 1e-5 * max(1.0, abs(want))
        print("XE K=%d w=%g ls=%g: %.17g, float64 %.17g, error / bound %.3e" % (k, weight, ls, got, want, abs(got - want) / bound))
        assert abs(got - want) <= bound, (got, want)
        worst = max(worst, abs(got - want) / bound)
    print("XE K=%d: worst error / bound %.3e" % (k, worst))
    _ran(k, "XE")


# ---- the output layer's gradient ---------------------------------------------------------------------------------------------
@KS
def test_final_gradient_every_class_count(k):
    """SSAL_FG: features 2 x 3 x 17 x 16 (two 16-wide tiles, the second ragged; two images).  |g - g64| <= kappa 2^-24 C_j for
    every entry (fto.grad_and_bound, fto.kappa, as test_gpu_train_final.py); the loss equal to the forward op's, bit for bit;
    two calls give the same bits"""
    x, kern, labels, mask = cc.final_case(k)
    n, h, w = cc.BLOCK_SHAPE
    net = semi._plain_net(k)
    net.Final.kernel.assign(kern)
    xd = dev(x)
    logits = net.Final(xd, training=False)
    logits32 = orc.conv2d_transpose_3x3_s2(x, kern)
    report_diff("K=%d Final logits (bit-exact)" % k, logits.cpu().numpy(), logits32)
    worst = 0.0
    for weight, ls in cc.LOSSES:
        tr = FinalLayerTrainer(net, 1e-3, loginverse_scaling=weight, label_smoothing=ls)
        loss, g = tr.gradient_features(xd, labels, mask, kernel=kern)
        loss2, g2 = tr.gradient_features(xd, labels, mask, kernel=kern)
        assert torch.equal(loss, loss2) and torch.equal(g, g2), "two calls differ"
        want = losses.masked_softmax_cross_entropy(dev(labels), logits, dev(mask), k, weight, ls)
        got_loss, want_loss = float(loss.cpu()[0]), float(want)
        print("FG K=%d w=%g ls=%g: loss %.17g, forward op %.17g" % (k, weight, ls, got_loss, want_loss))
        assert got_loss == want_loss, "loss %r != forward op %r" % (got_loss, want_loss)
        g64, c, loss64 = fto.grad_and_bound(x, kern, labels, mask, weight, ls, logits32)
        bound = fto.kappa(n, h, w, k, weight) * 2.0 ** -24 * c
        d = np.abs(g.cpu().numpy().astype(np.float64) - g64)
        ratio = float((d / np.maximum(bound, 1e-300)).max())
        print("FG K=%d w=%g ls=%g: max |g - g64| %.3e, max |g - g64| / bound %.3e, max |g64| %.3e"
              % (k, weight, ls, d.max(), ratio, np.abs(g64).max()))
        bad = d > bound
        assert not bad.any(), "K=%d w=%g ls=%g: %d of %d entries beyond kappa 2^-24 C (first at %s)" % (
            k, weight, ls, int(bad.sum()), bad.size, tuple(int(i) for i in np.argwhere(bad)[0]))
        assert abs(got_loss - loss64) <= 1e-5 * abs(loss64)
        worst = max(worst, ratio)
    print("FG K=%d: worst error / bound %.3e" % (k, worst))
    _ran(k, "FG")


@KS
def test_final_semi_supervised_every_class_count(k):
    """SSAL_FG<K, true>: the same shape with image 1 unlabelled, entropy, the threshold at the median confidence: the fused
    step against the composed one (test_gpu_train_semi's helpers) -- loss, gradient, confusion matrix and pseudo-pixel
    counts bit-identical -- once with features_raw (the pseudo pass on the undistorted features) and once without"""
    n, h, w = cc.BLOCK_SHAPE
    labelled = [1, 0]
    tr = FinalLayerTrainer(semi._plain_net(k), 1e-3, loginverse_scaling=1.02, label_smoothing=0.1)
    x_raw, kern, labels, mask = semi._case(7100 + k, n, h, w, k, labelled)
    x = (x_raw * torch.linspace(0.8, 1.25, 16, device="cuda")).contiguous()
    for name, raw in (("features_raw", x_raw), ("one pass", None)):
        want = semi._composed_features(k, tr, x, x if raw is None else raw, kern, labels, mask, labelled, "entropy")
        got = semi._fused_features(tr, x, raw, kern, labels, mask, np.asarray(labelled, np.uint8), "entropy", want[4], k)
        share = float(want[3].sum()) / (4 * h * w)
        print("FG<semi> K=%d %s: threshold %.6g, %.3f of the unlabelled pixels pass, loss %.17g"
              % (k, name, want[4], share, float(got[0].cpu()[0])))
        assert 0.2 < share < 0.8, "the threshold does not give a mixed mask"
        assert want[3][0].item() == 0 and int(want[2].sum()) > 0
        semi._assert_same("K=%d %s" % (k, name), got, want[:4])
    _ran(k, "FG<semi>")


# ---- the block head ------------------------------------------------------------------------------------------------------------
_BLOCK_MARGIN = []


def _block_margin():
    if not _BLOCK_MARGIN:
        _BLOCK_MARGIN.append(cc.block_margin(*cc.block_inputs()))
    return _BLOCK_MARGIN[0]


def _block_net(k, params, stats):
    net = ssal.ENet(k)
    net.build((None, None, None, 3))
    net.Final.kernel.assign(params["Final.kernel"])
    for a in lbo.BLOCK_VARS:
        getattr(net.Bottleneck5_1, a).assign(params["%s.%s" % (lbo.BLOCK, a)])
    for a in lbo.STATS:
        getattr(net.Bottleneck5_1, a).assign(stats[a])
    return net


@KS
def test_block_head_every_class_count(k):
    """SSAL_TB: a5_0 2 x 3 x 17 x 16 through Bottleneck5_1 (the same block, statistics and features for every K) and Final;
    the 13 gradients within lbo.tolerance of float64, the loss equal to the forward op's bit for bit, two calls the same bits,
    as test_gpu_train_block.py; the PReLU inputs meet margin > 16 (float64 against float32 torch on the CPU)"""
    margin = _block_margin()
    assert margin > 16.0, "the chosen data does not meet the condition on the PReLU inputs (margin %.1f)" % margin
    x, labels, mask, params, stats = cc.block_case(k)
    net = _block_net(k, params, stats)
    xd = dev(x)
    logits = net.Final(net.Bottleneck5_1(xd, training=False), training=False)
    logits32 = logits.cpu().numpy()
    worst = 0.0
    for weight, ls in cc.LOSSES:
        tr = LastBlockTrainer(net, 1e-3, loginverse_scaling=weight, label_smoothing=ls)
        loss, g = tr.gradient_features(xd, labels, mask)
        loss2, g2 = tr.gradient_features(xd, labels, mask)
        torch.cuda.synchronize()
        assert set(g) == set(lbo.NAMES)
        assert torch.equal(loss, loss2) and all(torch.equal(g[nm], g2[nm]) for nm in g), "two calls differ"
        want = losses.masked_softmax_cross_entropy(dev(labels), logits, dev(mask), k, weight, ls)
        got_loss, want_loss = float(loss.cpu()[0]), float(want)
        assert got_loss == want_loss, "loss %r != forward op %r" % (got_loss, want_loss)
        _, g64, _ = lbo.loss_and_grads(x, params, stats, labels, mask, weight, ls, logits32=logits32)
        _, g32, _ = lbo.loss_and_grads(x, params, stats, labels, mask, weight, ls, dtype=torch.float32)
        tol = lbo.tolerance(g32, g64)
        ratios = {nm: float(np.abs(g[nm].cpu().numpy().astype(np.float64) - g64[nm]).max()) / tol[nm] for nm in lbo.NAMES}
        top = max(ratios, key=ratios.get)
        print("TB K=%d w=%g ls=%g: loss %.17g, worst ratio %.3f (%s)" % (k, weight, ls, got_loss, ratios[top], top))
        bad = [nm for nm in lbo.NAMES if not ratios[nm] <= 1.0]
        assert not bad, "K=%d w=%g ls=%g: beyond max(8 e_ref, 2^-22 max |g64|): %s" % (
            k, weight, ls, ["%s %.3f" % (nm, ratios[nm]) for nm in bad])
        worst = max(worst, ratios[top])
    print("TB K=%d: worst error / tolerance %.3f, PReLU margin %.1f" % (k, worst, margin))
    _ran(k, "TB")


@KS
def test_block_head_semi_supervised_every_class_count(k):
    """SSAL_TB<K, true> and the target-only launch: a5_0 2 x 3 x 17 x 16 with image 1 unlabelled, entropy, the threshold at
    the median confidence of the unlabelled pixels: SemiSupervisedBlockTrainer's fused step against the composed one
    (test_gpu_train_deep_semi's helpers) -- loss, the 13 gradients, confusion matrix and pseudo-pixel counts bit-identical --
    once with features_raw (the target-only launch) and once without"""
    side, labelled = deep_semi.BLOCK, [1, 0]
    n, h, w = cc.BLOCK_SHAPE
    net = deep_semi._net(k)
    rng = np.random.default_rng(8100 + k)
    raw = side.inputs(rng, n, h, w)
    inputs = ((raw[0] * torch.linspace(0.8, 1.25, 16, device="cuda")).contiguous(),)
    labels, mask = deep_semi._annotation(rng, n, 2 * h, 2 * w, k, labelled)
    parent = LastBlockTrainer(net, 1e-3, loginverse_scaling=1.02, label_smoothing=0.1)
    fused = SemiSupervisedBlockTrainer(net, 1e-3, loginverse_scaling=1.02, label_smoothing=0.1)
    for name, r, family in (("features_raw", raw, "TB<target-only>"), ("one pass", None, "TB<semi>")):
        print("TB<semi> K=%d %s" % (k, name))
        lab, mk, wconf, wpp, thr = deep_semi._yardstick_targets(side, net, k, inputs, r, labels, mask, labelled, "entropy")
        wloss, wgrads = parent.gradient_features(*inputs, lab, mk)
        got = deep_semi._fused(side, fused, inputs, r, labels, mask, np.asarray(labelled, np.uint8), "entropy", thr, k)
        assert wpp[0].item() == 0 and 0 < wpp[1].item() < 4 * h * w and int(wconf.sum()) > 0
        deep_semi._assert_same("K=%d %s" % (k, name), got, (wloss, wgrads, wconf, wpp))
        _ran(k, family)


# ---- ICNet's head ----------------------------------------------------------------------------------------------------------------
@KS
def test_icnet_head_gradient_every_class_count(k):
    """SSAL_IH: sub12_sum 2 x 3 x 5 x 128 (two tiles across, both partial, two images), the case and the helpers of
    test_gpu_train_icnet_head.py.  |g - g64| <= kappa 2^-24 C_j for every entry of dKernel and dBias (iho.grad_and_bound,
    iho.kappa); the loss equal to the forward op's on the forward path's logits, bit for bit; two calls the same bits"""
    n, h, w = 2, 3, 5
    x, head, labels, mask = icnet_head._case(9100 + k, n, h, w, k)
    xd = torch.as_tensor(x).cuda()
    logits = icnet_head._forward_logits(x, head, k)
    worst = 0.0
    for weight, ls in cc.LOSSES:
        tr = ICNetHeadTrainer(icnet_head._shared_net(k), 1e-3, loginverse_scaling=weight, label_smoothing=ls)
        loss, gd = tr.gradient_features(xd, labels, mask, params=icnet_head._params(head, k))
        loss2, gd2 = tr.gradient_features(xd, labels, mask, params=icnet_head._params(head, k))
        want = losses.masked_softmax_cross_entropy(torch.as_tensor(labels).cuda(), logits, torch.as_tensor(mask).cuda(), k,
                                                   weight, ls)
        torch.cuda.synchronize()
        g = icnet_head._pack(gd)
        assert np.array_equal(g, icnet_head._pack(gd2)) and torch.equal(loss, loss2), "two calls differ"
        assert float(loss[0]) == float(want), "loss %r != forward op %r" % (float(loss[0]), float(want))
        g64, c, loss64 = iho.grad_and_bound(x, head, labels, mask, weight, ls, logits.cpu().numpy())
        bound = iho.kappa(n, h, w, k, weight) * 2.0 ** -24 * c
        d = np.abs(g.astype(np.float64) - g64)
        ratio = float((d / np.maximum(bound, 1e-300)).max())
        print("IH K=%d w=%g ls=%g: loss %.17g, max |g - g64| %.3e, max |g - g64| / bound %.3e, max |g64| %.3e"
              % (k, weight, ls, float(loss[0]), d.max(), ratio, np.abs(g64).max()))
        bad = d > bound
        assert not bad.any(), "K=%d w=%g ls=%g: %d of %d entries beyond kappa 2^-24 C (first at %d)" % (
            k, weight, ls, int(bad.sum()), bad.size, int(np.argwhere(bad)[0]))
        assert abs(float(loss[0]) - loss64) <= 1e-5 * abs(loss64)
        worst = max(worst, ratio)
    print("IH K=%d: worst error / bound %.3e" % (k, worst))
    _ran(k, "IH")


# ---- the sweep is whole ------------------------------------------------------------------------------------------------------------
def test_every_family_met_every_class_count(request):
    """collection: every test above is parametrised over exactly K = 2 .. 32, without a skip or an expected failure; execution:
    of the cases this session selected, every one ran to its end -- in a run of the whole file, 31 of 31 per family"""
    here = [it for it in request.session.items if it.path == request.node.path and it is not request.node]
    assert here, "the sweep's tests come before this one"
    selected = {}
    for it in here:
        assert not list(it.iter_markers("skip")) and not list(it.iter_markers("skipif")) and not list(it.iter_markers("xfail"))
        marks = [m for m in it.iter_markers("parametrize")]
        assert len(marks) == 1 and tuple(marks[0].args[1]) == tuple(range(2, 33)), it.nodeid
        selected.setdefault(it.originalname, set()).add(it.callspec.params["k"])
    tests = {"test_score_logits_every_class_count": ("SL",), "test_upscore_every_class_count": ("US",),
             "test_enet_final_score_and_evaluate_every_class_count": ("FS", "FS51", "FE"),
             "test_loss_op_every_class_count": ("XE",), "test_final_gradient_every_class_count": ("FG",),
             "test_final_semi_supervised_every_class_count": ("FG<semi>",), "test_block_head_every_class_count": ("TB",),
             "test_block_head_semi_supervised_every_class_count": ("TB<semi>", "TB<target-only>"),
             "test_icnet_head_gradient_every_class_count": ("IH",)}
    assert sorted(f for fs in tests.values() for f in fs) == sorted(FAMILIES)
    whole = set(selected) == set(tests) and all(ks == set(range(2, 33)) for ks in selected.values())
    for name, families in tests.items():
        for f in families:
            print("%-16s %2d of %2d class counts executed" % (f, len(RAN[f]), len(selected.get(name, ()))))
            assert RAN[f] == selected.get(name, set()), "%s: K = %s did not run to the end" % (
                f, sorted(selected.get(name, set()) - RAN[f]))
            if whole:
                assert len(RAN[f]) == 31
