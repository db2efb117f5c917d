"""Deep-tail training on the MI355X: the 50 gradients of Bottleneck4_1, Bottleneck4_2, Bottleneck5_0,
Bottleneck5_1 and Final.kernel against the float64 oracle with the tolerance measured from the reference arithmetic's own
error; the loss against the forward op and the tail's 38 gradients against DecoderTailTrainer, bit for bit; determinism; Adam
bit for bit against the float32 restatement; the weights of record after three steps; the semi-supervised step against the
composed one; a short end-to-end run; the C entries' statuses."""
import numpy as np
import pytest
import torch

import semanticsegmentationactivelearning_amd as ssal
from semanticsegmentationactivelearning_amd import _lib
from semanticsegmentationactivelearning_amd import active_learning as al
from semanticsegmentationactivelearning_amd import synthetic as syn
from semanticsegmentationactivelearning_amd.tensortools import losses, metrics
from semanticsegmentationactivelearning_amd.training import DecoderTailTrainer, DeepTailTrainer, SemiSupervisedDeepTailTrainer

import decoder_tail_train_oracle as dto
import deep_tail_train_oracle as ddo
import final_train_oracle as fto
import last_block_train_oracle as lbo
import last_stage_train_oracle as lso
from helpers import frames, make_model

pytestmark = pytest.mark.gpu

AL_PARAMS = {"hyperparams": {"learning_rate": 0.0005, "learning_rate_decay": 0.0,
                             "optimizer": {"type": "Adam", "kwargs": {"beta1": 0.9, "beta2": 0.99}},
                             "weight_reg": {"L2": 0.0002, "L1": 0.0},
                             "softmax": {"label_smoothing": 0.0, "loginverse_scaling": 1.02, "multiscale": False}}}
BLOCKS = ((lbo.BLOCK, lbo.BLOCK_VARS), (lso.STAGE, lso.STAGE_VARS), (dto.TAIL, dto.TAIL_VARS), (ddo.DEEP, ddo.DEEP_VARS))

CASES = [(k, weight, ls) for k in (2, 19, 32) for weight in (0.0, 1.02) for ls in (0.0, 0.1)]
# seeds for which the ORACLE ALONE (float64 against float32 torch on the CPU) meets the condition on the inputs: the smallest
# |PReLU input| of the float64 forward, over all twelve PReLUs, exceeds 16 x the largest |fp32 - float64| deviation there
# (deep_tail_train_oracle: prelu_inputs / prelu_margin on _case's x, argmax and parameters; the forward does not depend on the
# loss' weight or smoothing; the GPU's results play no part).  Recipe, 1 x 9 x 12: try 300, 301, ... and keep the first seed whose
# ratio exceeds 24 (25.7 / 31.9 / 29.7 for K = 2 / 19 / 32).  2 x 10 x 17 and 1 x 20 x 20 have more than twice the PReLU inputs
# and no seed reaches 24, neither in [300, 40 000) nor, with the search started again at base 40 000, in [40 000, 80 000) (the
# best ratios seen: 23.3 / 20.7 / 23.6 at K = 2 / 19 / 32).  For 2 x 10 x 17 the shape is kept and the recipe's threshold, not
# the asserted condition, gives way: the first seed from 300 up whose ratio exceeds 19 (22.6 / 20.7 / 23.7 for K = 2 / 19 / 32;
# 22.2 / 22.0 / 23.9 on the MI355X host).  The fp32 deviation is the host CPU's: torch's float32 kernels differ between
# instruction sets, and the ratio of one seed moves by a third between hosts.  1 x 20 x 20's first pick, 4627 (19.6), fell to
# 14.7 on the MI355X host and is replaced: the search went on at base 80 000 through 540 000 for seeds whose smallest |PReLU
# input| (float64, the same on every host) is at least 7.5e-5; of those, 143998 has the largest smallest ratio over the hosts
# and instruction sets tried (smallest |input| 9.43e-5; 18.6 with AVX-512, 24.1 with AVX2, 24.6 on the MI355X host).
SEEDS = {((1, 9, 12), 2): 438, ((1, 9, 12), 19): 445, ((1, 9, 12), 32): 445, ((2, 10, 17), 2): 2344, ((2, 10, 17), 19): 22724,
         ((2, 10, 17), 32): 3802, ((1, 20, 20), 19): 143998}


def _shape(idx):
    return (1, 9, 12) if (idx // 2 + idx) % 2 == 0 else (2, 10, 17)


def _case(seed, n, h, w, k):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, h, w, 64)) * 0.7).astype(np.float32)
    am = lso.random_argmax(rng, n, h, w)
    labels = rng.integers(0, k, (n, 4 * h, 4 * w)).astype(np.uint8)
    mask = (rng.uniform(size=(n, 4 * h, 4 * w)) > 0.25).astype(np.float32)
    labels[rng.uniform(size=labels.shape) < 0.05] = 255  # label 255 under both mask values
    params, stats = ddo.random_params(seed + 1000, k)
    return x, am, labels, mask, params, stats


def _net_with(k, params, stats):
    net = ssal.ENet(k)
    net.build((None, None, None, 3))
    net.Final.kernel.assign(params["Final.kernel"])
    for blk, names in BLOCKS:
        for a in names:
            getattr(getattr(net, blk), a).assign(params["%s.%s" % (blk, a)])
        for a in ddo.STATS:
            getattr(getattr(net, blk), a).assign(stats[blk][a])
    return net


def _check_case(name, n, h, w, k, weight, ls, max_workgroups=0):
    x, am, labels, mask, params, stats = _case(SEEDS[((n, h, w), k)], n, h, w, k)
    net = _net_with(k, params, stats)
    tr = DeepTailTrainer(net, 1e-3, loginverse_scaling=weight, label_smoothing=ls)
    xd, amd = torch.as_tensor(x).cuda(), torch.as_tensor(am).cuda()
    loss, g = tr.gradient_features(xd, amd, labels, mask, max_workgroups=max_workgroups)
    loss2, g2 = tr.gradient_features(xd, amd, labels, mask, max_workgroups=max_workgroups)
    torch.cuda.synchronize()
    assert set(g) == set(ddo.NAMES)
    assert torch.equal(loss, loss2) and all(torch.equal(g[nm], g2[nm]) for nm in g), "two calls differ"
    # the forward the scoring path computes: the five layers of the model
    a41 = net.Bottleneck4_1(xd, training=False)
    a42 = net.Bottleneck4_2(a41, training=False)
    logits = net.Final(net.Bottleneck5_1(net.Bottleneck5_0(a42, amd, training=False), training=False), training=False)
    want = losses.masked_softmax_cross_entropy(torch.as_tensor(labels).cuda(), logits, torch.as_tensor(mask).cuda(), k,
                                               weight, ls)
    got_loss, want_loss = float(loss.cpu()[0]), float(want)
    print("%s: loss %.17g, forward op %.17g" % (name, got_loss, want_loss))
    assert got_loss == want_loss, "loss %r != forward op %r" % (got_loss, want_loss)
    # the prefix is the tail: the other 38 gradients are DecoderTailTrainer's on the model's own a4_1, bit for bit
    lt, gt = DecoderTailTrainer(net, 1e-3, loginverse_scaling=weight, label_smoothing=ls).gradient_features(
        a41, amd, labels, mask, max_workgroups=max_workgroups)
    assert torch.equal(lt, loss)
    for nm in dto.NAMES:
        assert torch.equal(gt[nm], g[nm]), "%s differs from DecoderTailTrainer's" % nm
    logits32 = logits.cpu().numpy()
    _, g64, _ = ddo.loss_and_grads(x, am, params, stats, labels, mask, weight, ls, logits32=logits32)
    _, _, pre64 = ddo.loss_and_grads(x, am, params, stats, labels, mask, weight, ls)
    _, g32, pre32 = ddo.loss_and_grads(x, am, params, stats, labels, mask, weight, ls, dtype=torch.float32)
    margin = ddo.prelu_margin(pre64, pre32)
    print("%s: smallest |PReLU input| %.3e = %.1f x the largest fp32 deviation" % (name, np.abs(pre64).min(), margin))
    assert margin > 16.0, "the chosen data does not meet the condition on the PReLU inputs"
    tol = ddo.tolerance(g32, g64)
    worst = {}
    for nm in ddo.NAMES:
        d = float(np.abs(g[nm].cpu().numpy().astype(np.float64) - g64[nm]).max())
        worst[nm] = d / tol[nm]
        print("%s: %-32s max |g - g64| %.3e, tolerance %.3e, ratio %.3f, max |g64| %.3e"
              % (name, nm, d, tol[nm], worst[nm], np.abs(g64[nm]).max()))
    bad = [nm for nm in ddo.NAMES if not worst[nm] <= 1.0]
    assert not bad, "%s: beyond max(8 e_ref, 2^-22 max |g64|): %s" % (name, bad)


@pytest.mark.parametrize("k,weight,ls", CASES)
def test_gradients_match_float64_oracle(k, weight, ls):
    """max |g_gpu - g64| <= max(8 e_ref, 2^-22 max |g64|) per tensor, e_ref = max |g32 - g64| of float32 torch autograd of the
    same restatement; a4_0 1 x 9 x 12 and 2 x 10 x 17 (ragged against the 8 x 8 tile in both directions), alternated so that,
    for every K, each shape meets both weights and both smoothing values"""
    idx = CASES.index((k, weight, ls))
    n, h, w = _shape(idx)
    _check_case("K=%d w=%g ls=%g %dx%dx%d" % (k, weight, ls, n, h, w), n, h, w, k, weight, ls)


def test_gradients_more_tiles_than_workgroups():
    """a4_0 1 x 20 x 20: 9 tiles on 2 workgroups"""
    _check_case("20x20 on 2 workgroups", 1, 20, 20, 19, 1.02, 0.0, max_workgroups=2)


def test_adam_bit_identical_and_regulariser_ranges():
    """three step_features calls: every w, m, v of the 50 trained variables equals final_train_oracle.adam_step fed with the
    GPU's own gradient; l1 / l2 only on the variables the reference regularises; the 24 statistics and every other variable
    of the model are unchanged"""
    k = 19
    x, am, labels, mask, params, stats = _case(31, 2, 12, 20, k)
    params["Final.kernel"][0, 0, :3, :] = 0.0  # exact zeros: sign(0) = 0
    params["Bottleneck4_1.exp_kernel"][0, 0, :4, :] = 0.0
    net = _net_with(k, params, stats)
    before = {v.name: v.numpy().copy() for v in net.variables}
    tr = DeepTailTrainer(net, 5e-4, 0.9, 0.99, l1=1e-4, l2=2e-4, loginverse_scaling=1.02)
    xd, amd = torch.as_tensor(x).cuda(), torch.as_tensor(am).cuda()
    w = {nm: np.array(params[nm]) for nm in ddo.NAMES}
    m = {nm: np.zeros_like(w[nm]) for nm in ddo.NAMES}
    v = {nm: np.zeros_like(w[nm]) for nm in ddo.NAMES}
    b1p, b2p = np.float32(0.9), np.float32(0.99)
    var_of = lambda nm: net.Final.kernel if nm == "Final.kernel" else getattr(getattr(net, nm.split(".")[0]), nm.split(".")[1])
    for step in range(3):
        _, g = tr.gradient_features(xd, amd, labels, mask)
        tr.step_features(xd, amd, labels, mask)
        st = tr.state
        for nm in ddo.NAMES:
            reg = nm in ddo.REGULARISED
            w[nm], m[nm], v[nm] = fto.adam_step(w[nm], m[nm], v[nm], g[nm].cpu().numpy(), np.float32(5e-4), 0.9, 0.99, 1e-8,
                                                b1p, b2p, l1=1e-4 if reg else 0.0, l2=2e-4 if reg else 0.0)
            assert np.array_equal(st["m"][nm], m[nm]), "m of %s differs at step %d" % (nm, step)
            assert np.array_equal(st["v"][nm], v[nm]), "v of %s differs at step %d" % (nm, step)
            assert np.array_equal(var_of(nm).numpy(), w[nm]), "%s differs at step %d" % (nm, step)
        b1p, b2p = np.float32(b1p * np.float32(0.9)), np.float32(b2p * np.float32(0.99))
    assert tr.state["t"] == 3
    for blk, _ in BLOCKS:
        for a in ddo.STATS:
            assert np.array_equal(getattr(getattr(net, blk), a).numpy(), stats[blk][a])
    trained = {var_of(nm).name for nm in ddo.NAMES}
    changed = {vv.name for vv in net.variables if not np.array_equal(vv.numpy(), before[vv.name])}
    assert changed == trained, "changed %s, trained %s" % (sorted(changed ^ trained), len(trained))


def _frames_case():
    x = syn.synth_frames_device(0, 2, 64, 128, 3)
    rng = np.random.default_rng(9)
    labels = rng.integers(0, 19, (2, 64, 128)).astype(np.uint8)
    mask = (rng.uniform(size=(2, 64, 128)) > 0.2).astype(np.float32)
    return x, labels, mask


def test_image_entry_matches_features_and_weights_of_record():
    """step(images) == step_features(*features(images)); after three steps net(x) and net.score(x) use the new weights
    (bit-identical to the C oracle with the host variables); everything outside the trained variables is unchanged"""
    from oracle import enet_oracle as orc
    net, _ = make_model(19, 3, seed=0)
    twin, _ = make_model(19, 3, seed=0)
    x, labels, mask = _frames_case()
    before = {v.name: v.numpy().copy() for v in net.variables}
    trained = {"Final/Kernel"} | {getattr(getattr(net, blk), a).name for blk, names in BLOCKS for a in names}
    tr = DeepTailTrainer.from_params(net, AL_PARAMS)
    tw = DeepTailTrainer.from_params(twin, AL_PARAMS)
    feats, am = tw.features(x)
    assert tuple(feats.shape) == (2, 16, 32, 64) and tuple(am.shape) == (2, 16, 32, 16) and am.dtype == torch.int64
    # Bottleneck4_0's output: the model's own Bottleneck4_1 turns it into the tail trainer's features, bit for bit
    f41, am41 = DecoderTailTrainer.from_params(twin, AL_PARAMS).features(x)
    assert torch.equal(twin.Bottleneck4_1(feats, training=False), f41) and not torch.equal(feats, f41)
    assert torch.equal(am, am41)
    for step in range(3):
        la = tr.step(x, labels, mask)
        lb = tw.step_features(feats, am, labels, mask)
        assert float(la) == float(lb), "step %d: step(images) loss %r != step_features loss %r" % (step, float(la), float(lb))
    for nm, var, _, _ in tr._named():
        blk, a = nm.split(".")
        other = twin.Final.kernel if nm == "Final.kernel" else getattr(getattr(twin, blk), a)
        assert np.array_equal(var.numpy(), other.numpy()), nm
    changed = {v.name for v in net.variables if not np.array_equal(v.numpy(), before[v.name])}
    assert changed == trained, "written outside the trained variables: %s" % sorted(changed ^ trained)
    P = syn.enet_params_dict(net)
    want_mean, _, want_label, want_logits = orc.score_images(P, frames([0, 1], 64, 128, 3), "entropy")
    scores, ex = net.score(x, return_label=True)
    logits = net(x, training=False)
    torch.cuda.synchronize()
    assert np.array_equal(logits.cpu().numpy(), want_logits)
    assert np.array_equal(ex["label"].cpu().numpy(), want_label)
    assert np.abs(scores.cpu().numpy() - want_mean).max() <= 1e-6
    want = float(losses.masked_softmax_cross_entropy(torch.as_tensor(labels).cuda(), logits, torch.as_tensor(mask).cuda(), 19,
                                                     1.02, 0.0))
    assert float(tr.step(x, labels, mask)) == want
    # the images entry leaves Bottleneck4_0's output where ssal_enet_train_tail2_features_offset says
    off = _lib.lib().ssal_enet_train_tail2_features_offset(net._handle, 2, 64, 128)
    left = net._ws[off:off + 4 * feats.numel()].view(torch.float32).view(feats.shape)
    assert torch.equal(left, feats)


@pytest.mark.parametrize("with_raw", (False, True), ids=("training-logits", "images_raw"))
def test_semi_supervised_step_matches_composition(with_raw):
    """SemiSupervisedDeepTailTrainer.step on 2 x 64 x 128 with image 1 unlabelled (0xFF labels and NaN masks in its planes)
    against the composed step on a twin: net.score's label / mask planes -> training_targets -> the plain step; the loss, the
    packed gradient (every variable's), the confusion matrix and the pseudo-pixel counts, bit for bit, over two steps"""
    net_a, _ = make_model(19, 3, seed=0)
    net_b, _ = make_model(19, 3, seed=0)
    x_raw, labels, mask = _frames_case()
    labels[1], mask[1] = 0xFF, np.nan
    labels, mask = torch.as_tensor(labels).cuda(), torch.as_tensor(mask).cuda()
    sel = torch.tensor([True, False]).cuda()
    x = (x_raw * torch.tensor([0.9, 1.1, 0.8], device="cuda")).contiguous() if with_raw else x_raw
    tr_a, tr_b = SemiSupervisedDeepTailTrainer.from_params(net_a, AL_PARAMS), DeepTailTrainer.from_params(net_b, AL_PARAMS)
    _, p = net_b.score(x_raw, "entropy", 0.0, return_confidence=True)
    thr = float(np.median(p["confidence"][1].float().cpu().numpy()))
    conf_a = torch.zeros((19, 19), dtype=torch.int64, device="cuda")
    conf_b = torch.zeros_like(conf_a)
    for step in range(2):
        la, ppa = tr_a.step(x, labels, mask, labelled=sel, measure="entropy", threshold=thr, confusion=conf_a,
                            return_pseudo_pixels=True, **({"images_raw": x_raw} if with_raw else {}))
        _, p = net_b.score(x_raw, "entropy", thr, return_label=True, return_mask=True)
        pl, pm = p["label"], p["mask"].float()
        lab, mk = al.training_targets(sel, labels, mask, pl, pm)
        _, pt = al.score_logits(net_b(x, training=False), "confidence", 0.0, return_label=True)  # the first maximum
        conf_b += metrics.confusion_mat(lab, pt["label"], 19, weights=mk)
        ppb = pm.to(torch.int64).sum(dim=(1, 2)) * (~sel).to(torch.int64)
        lb = tr_b.step(x, lab, mk)
        print("step %d: loss %.17g / %.17g, pseudo pixels %s" % (step, float(la), float(lb), ppa.tolist()))
        assert float(la).hex() == float(lb).hex(), "loss differs at step %d" % step
        ga, gb = tr_a._dev["grad"].cpu().numpy(), tr_b._dev["grad"].cpu().numpy()
        assert ga.shape == gb.shape and np.array_equal(ga.view(np.uint32), gb.view(np.uint32)), "gradients differ at step %d" % step
        assert torch.equal(ppa, ppb) and ppa[0].item() == 0 and 0 < ppa[1].item() < 64 * 128
        assert torch.equal(conf_a, conf_b), "confusion differs at step %d" % step
    for (nm, va, _, _), (_, vb, _, _) in zip(tr_a._named(), tr_b._named()):
        assert np.array_equal(va.numpy(), vb.numpy()), nm


def test_end_to_end_deep_tail_learns():
    """section 15's setup: labels from the original head's argmax, reinitialize(0), 50 steps at the reference's settings: the
    loss ends no higher than DecoderTailTrainer's on the same data and start"""
    out = {}
    for cls in (DecoderTailTrainer, DeepTailTrainer):
        net, _ = make_model(19, 3, seed=0)
        x = syn.synth_frames_device(0, 2, 64, 128, 3)
        _, extra = net.score(x, return_label=True)
        labels = extra["label"].clone()
        mask = torch.ones((2, 64, 128), dtype=torch.float32, device=x.device)
        tr = cls.from_params(net, AL_PARAMS)
        tr.reinitialize(seed=0)
        ls_ = [float(tr.step(x, labels, mask)) for _ in range(50)]
        out[cls.__name__] = ls_
        print("end to end, %s: loss %.6g -> %.6g (x%.3f)" % (cls.__name__, ls_[0], ls_[-1], ls_[-1] / ls_[0]))
    assert out["DeepTailTrainer"][0] == out["DecoderTailTrainer"][0]  # the same start, the same forward
    assert out["DeepTailTrainer"][-1] <= out["DecoderTailTrainer"][-1]


def test_invalid_arguments_on_device():
    """classes 1 and 33, a too-small workspace (the one-block call's) and a mismatched argmax shape: refused without a launch
    (the outputs keep their bytes)"""
    L = _lib.lib()
    n, h, w, k = 1, 8, 8, 19
    x = torch.zeros((n, h, w, 64), device="cuda")
    am = torch.as_tensor(lso.random_argmax(np.random.default_rng(0), n, h, w)).cuda()
    lab = torch.zeros((n, 4 * h, 4 * w), dtype=torch.uint8, device="cuda")
    mk = torch.ones((n, 4 * h, 4 * w), device="cuda")
    params = torch.zeros((L.ssal_train_tail2_param_floats(32),), device="cuda")
    nbytes = L.ssal_train_tail2_grad_workspace_bytes(n, h, w, 32)
    ws = torch.zeros((nbytes,), dtype=torch.uint8, device="cuda")
    loss = torch.full((1,), 7.0, dtype=torch.float64, device="cuda")
    grad = torch.full_like(params, 7.0)

    def call(classes=k, ws_bytes=nbytes):
        return L.ssal_train_tail2_grad_nhwc(_lib.dev_ptr(x), _lib.dev_ptr(am), n, h, w, classes, _lib.dev_ptr(params),
                                            _lib.dev_ptr(lab), _lib.dev_ptr(mk), 0.0, 0.0, 0, _lib.dev_ptr(loss),
                                            _lib.dev_ptr(grad), _lib.dev_ptr(ws), ws_bytes, _lib.stream_ptr())
    assert call(classes=1) == _lib.SSAL_EINVAL and call(classes=33) == _lib.SSAL_EINVAL
    assert call(ws_bytes=L.ssal_train_tail2_grad_workspace_bytes(n, h, w, k) - 1) in (_lib.SSAL_EINVAL, _lib.SSAL_ENOMEM)
    assert call(ws_bytes=L.ssal_train_tail_grad_workspace_bytes(n, h, w, k)) == _lib.SSAL_ENOMEM
    torch.cuda.synchronize()
    assert float(loss[0]) == 7.0 and bool((grad == 7.0).all()) and not bool(ws.any())
    net = ssal.ENet(19)
    net.build((None, None, None, 3))
    tr = DeepTailTrainer(net, 1e-3)
    labn, mkn = np.zeros((1, 32, 32), np.uint8), np.ones((1, 32, 32), np.float32)
    with pytest.raises(ValueError):
        tr.gradient_features(x, am[:, :, :4], labn, mkn)  # argmax of another shape
    with pytest.raises(ValueError):
        tr.gradient_features(x, am + 32, labn, mkn)  # a device tensor of indices outside their windows
    with pytest.raises(ValueError):
        tr.gradient_features(x, am, labn[:, :8], mkn)
    assert call() == _lib.SSAL_OK  # the same arguments, valid
    torch.cuda.synchronize()
    assert bool((grad[:L.ssal_train_tail2_param_floats(k)] != 7.0).all())
