"""Last-stage training on the MI355X: the 26 gradients against the float64 oracle with the tolerance
measured from the reference arithmetic's own error; the loss against the forward op, bit for bit; determinism; Adam bit for
bit against the float32 restatement; the weights of record after three steps; the last block's 13 gradients against
LastBlockTrainer; a short end-to-end run."""
import numpy as np
import pytest
import torch

import semanticsegmentationactivelearning_amd as ssal
from semanticsegmentationactivelearning_amd import synthetic as syn
from semanticsegmentationactivelearning_amd.tensortools import losses
from semanticsegmentationactivelearning_amd.training import LastBlockTrainer, LastStageTrainer

import final_train_oracle as fto
import last_block_train_oracle as lbo
import last_stage_train_oracle as lso
from helpers import frames, make_model

pytestmark = pytest.mark.gpu

AL_PARAMS = {"hyperparams": {"learning_rate": 0.0005, "learning_rate_decay": 0.0,
                             "optimizer": {"type": "Adam", "kwargs": {"beta1": 0.9, "beta2": 0.99}},
                             "weight_reg": {"L2": 0.0002, "L1": 0.0},
                             "softmax": {"label_smoothing": 0.0, "loginverse_scaling": 1.02, "multiscale": False}}}

CASES = [(k, weight, ls) for k in (2, 6, 19, 32) for weight in (0.0, 1.02) for ls in (0.0, 0.1)]
# seeds for which the ORACLE ALONE (float64 against float32 torch on the CPU) meets the condition on the inputs: the smallest
# |PReLU input| of the float64 forward, over all six PReLUs, exceeds 16 x the largest |fp32 - float64| deviation there.
# Found by trying 300, 301, ... per case and keeping the first seed whose ratio exceeds 24
# (tests/last_stage_train_oracle.py: prelu_margin).
SEEDS = {0: 306, 1: 1092, 2: 1092, 3: 306, 4: 301, 5: 749, 6: 749, 7: 301, 8: 300, 9: 393, 10: 393, 11: 300, 12: 300, 13: 885,
         14: 885, 15: 300, "tiles": 1645}


def _shape(idx):
    return (1, 9, 12) if (idx // 2 + idx) % 2 == 0 else (2, 10, 17)


def _case(seed, n, h, w, k):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, h, w, 64)) * 0.7).astype(np.float32)
    am = lso.random_argmax(rng, n, h, w)
    labels = rng.integers(0, k, (n, 4 * h, 4 * w)).astype(np.uint8)
    mask = (rng.uniform(size=(n, 4 * h, 4 * w)) > 0.25).astype(np.float32)
    labels[rng.uniform(size=labels.shape) < 0.05] = 255  # label 255 under both mask values
    params, stats = lso.random_params(seed + 1000, k)
    return x, am, labels, mask, params, stats


def _net_with(k, params, stats):
    net = ssal.ENet(k)
    net.build((None, None, None, 3))
    net.Final.kernel.assign(params["Final.kernel"])
    for blk, names in ((lbo.BLOCK, lbo.BLOCK_VARS), (lso.STAGE, lso.STAGE_VARS)):
        for a in names:
            getattr(getattr(net, blk), a).assign(params["%s.%s" % (blk, a)])
        for a in lso.STATS:
            getattr(getattr(net, blk), a).assign(stats[blk][a])
    return net


def _check_case(name, n, h, w, k, weight, ls, seed, max_workgroups=0):
    x, am, labels, mask, params, stats = _case(seed, n, h, w, k)
    net = _net_with(k, params, stats)
    tr = LastStageTrainer(net, 1e-3, loginverse_scaling=weight, label_smoothing=ls)
    xd, amd = torch.as_tensor(x).cuda(), torch.as_tensor(am).cuda()
    loss, g = tr.gradient_features(xd, amd, labels, mask, max_workgroups=max_workgroups)
    loss2, g2 = tr.gradient_features(xd, amd, labels, mask, max_workgroups=max_workgroups)
    torch.cuda.synchronize()
    assert torch.equal(loss, loss2) and all(torch.equal(g[nm], g2[nm]) for nm in g), "two calls differ"
    # the forward the scoring path computes: the three layers of the model
    a5 = net.Bottleneck5_0(xd, amd, training=False)
    logits = net.Final(net.Bottleneck5_1(a5, training=False), training=False)
    want = losses.masked_softmax_cross_entropy(torch.as_tensor(labels).cuda(), logits, torch.as_tensor(mask).cuda(), k,
                                               weight, ls)
    got_loss, want_loss = float(loss.cpu()[0]), float(want)
    print("%s: loss %.17g, forward op %.17g" % (name, got_loss, want_loss))
    assert got_loss == want_loss, "loss %r != forward op %r" % (got_loss, want_loss)
    logits32 = logits.cpu().numpy()
    _, g64, _ = lso.loss_and_grads(x, am, params, stats, labels, mask, weight, ls, logits32=logits32)
    _, _, pre64 = lso.loss_and_grads(x, am, params, stats, labels, mask, weight, ls)
    _, g32, pre32 = lso.loss_and_grads(x, am, params, stats, labels, mask, weight, ls, dtype=torch.float32)
    margin = lso.prelu_margin(pre64, pre32)
    print("%s: smallest |PReLU input| %.3e = %.1f x the largest fp32 deviation" % (name, np.abs(pre64).min(), margin))
    assert margin > 16.0, "the chosen data does not meet the condition on the PReLU inputs"
    tol = lso.tolerance(g32, g64)
    worst = {}
    for nm in lso.NAMES:
        d = float(np.abs(g[nm].cpu().numpy().astype(np.float64) - g64[nm]).max())
        worst[nm] = d / tol[nm]
        print("%s: %-32s max |g - g64| %.3e, tolerance %.3e, ratio %.3f, max |g64| %.3e"
              % (name, nm, d, tol[nm], worst[nm], np.abs(g64[nm]).max()))
    bad = [nm for nm in lso.NAMES if not worst[nm] <= 1.0]
    assert not bad, "%s: beyond max(8 e_ref, 2^-22 max |g64|): %s" % (name, bad)


@pytest.mark.parametrize("k,weight,ls", CASES)
def test_gradients_match_float64_oracle(k, weight, ls):
    """max |g_gpu - g64| <= max(8 e_ref, 2^-22 max |g64|) per tensor, e_ref = max |g32 - g64| of float32 torch autograd of
    the same restatement; a4_2 1 x 9 x 12 and 2 x 10 x 17 (half resolution 18 x 24 and 20 x 34: ragged tiles in both
    directions), alternated so that, for every K, each shape meets both weights and both smoothing values"""
    idx = CASES.index((k, weight, ls))
    n, h, w = _shape(idx)
    _check_case("K=%d w=%g ls=%g %dx%dx%d" % (k, weight, ls, n, h, w), n, h, w, k, weight, ls, SEEDS[idx])


def test_gradients_more_tiles_than_workgroups():
    """a4_2 1 x 20 x 20: 9 tiles of the 40 x 40 half-resolution map on 2 workgroups"""
    _check_case("20x20 on 2 workgroups", 1, 20, 20, 19, 1.02, 0.0, SEEDS["tiles"], max_workgroups=2)


def test_adam_bit_identical_and_regulariser_ranges():
    """three step_features calls: every w, m, v of the 26 variables equals final_train_oracle.adam_step fed with the GPU's
    own gradient; l1 / l2 only on the variables the reference regularises; the 12 statistics are unchanged"""
    k = 19
    x, am, labels, mask, params, stats = _case(31, 2, 12, 20, k)
    params["Final.kernel"][0, 0, :3, :] = 0.0  # exact zeros: sign(0) = 0
    params["Bottleneck5_0.res_kernel"][0, 0, :4, :] = 0.0
    net = _net_with(k, params, stats)
    before = {v.name: v.numpy().copy() for v in net.variables}
    tr = LastStageTrainer(net, 5e-4, 0.9, 0.99, l1=1e-4, l2=2e-4, loginverse_scaling=1.02)
    xd, amd = torch.as_tensor(x).cuda(), torch.as_tensor(am).cuda()
    w = {nm: np.array(params[nm]) for nm in lso.NAMES}
    m = {nm: np.zeros_like(w[nm]) for nm in lso.NAMES}
    v = {nm: np.zeros_like(w[nm]) for nm in lso.NAMES}
    b1p, b2p = np.float32(0.9), np.float32(0.99)
    var_of = lambda nm: net.Final.kernel if nm == "Final.kernel" else getattr(getattr(net, nm.split(".")[0]), nm.split(".")[1])
    for step in range(3):
        _, g = tr.gradient_features(xd, amd, labels, mask)
        tr.step_features(xd, amd, labels, mask)
        st = tr.state
        for nm in lso.NAMES:
            reg = nm in lso.REGULARISED
            w[nm], m[nm], v[nm] = fto.adam_step(w[nm], m[nm], v[nm], g[nm].cpu().numpy(), np.float32(5e-4), 0.9, 0.99, 1e-8,
                                                b1p, b2p, l1=1e-4 if reg else 0.0, l2=2e-4 if reg else 0.0)
            assert np.array_equal(st["m"][nm], m[nm]), "m of %s differs at step %d" % (nm, step)
            assert np.array_equal(st["v"][nm], v[nm]), "v of %s differs at step %d" % (nm, step)
            assert np.array_equal(var_of(nm).numpy(), w[nm]), "%s differs at step %d" % (nm, step)
        b1p, b2p = np.float32(b1p * np.float32(0.9)), np.float32(b2p * np.float32(0.99))
    assert tr.state["t"] == 3
    for blk in (lbo.BLOCK, lso.STAGE):
        for a in lso.STATS:
            assert np.array_equal(getattr(getattr(net, blk), a).numpy(), stats[blk][a])
    trained = {var_of(nm).name for nm in lso.NAMES}
    changed = {vv.name for vv in net.variables if not np.array_equal(vv.numpy(), before[vv.name])}
    assert changed == trained, "changed %s, trained %s" % (sorted(changed ^ trained), len(trained))


def test_image_entry_matches_features_and_weights_of_record():
    """step(images) == step_features(*features(images)); after three steps net(x) and net.score(x) use the new weights
    (bit-identical to the C oracle with the host variables); everything outside the 26 variables is unchanged"""
    from oracle import enet_oracle as orc
    net, _ = make_model(19, 3, seed=0)
    twin, _ = make_model(19, 3, seed=0)
    x = syn.synth_frames_device(0, 2, 64, 128, 3)
    rng = np.random.default_rng(9)
    labels = rng.integers(0, 19, (2, 64, 128)).astype(np.uint8)
    mask = (rng.uniform(size=(2, 64, 128)) > 0.2).astype(np.float32)
    before = {v.name: v.numpy().copy() for v in net.variables}
    trained = {"Final/Kernel"} | {getattr(net.Bottleneck5_1, a).name for a in lbo.BLOCK_VARS} \
        | {getattr(net.Bottleneck5_0, a).name for a in lso.STAGE_VARS}
    tr = LastStageTrainer.from_params(net, AL_PARAMS)
    tw = LastStageTrainer.from_params(twin, AL_PARAMS)
    feats, am = tw.features(x)
    assert tuple(feats.shape) == (2, 16, 32, 64) and tuple(am.shape) == (2, 16, 32, 16) and am.dtype == torch.int64
    for step in range(3):
        la = tr.step(x, labels, mask)
        lb = tw.step_features(feats, am, labels, mask)
        assert float(la) == float(lb), "step %d: step(images) loss %r != step_features loss %r" % (step, float(la), float(lb))
    for nm, var, _, _ in tr._named():
        blk, a = nm.split(".")
        other = twin.Final.kernel if nm == "Final.kernel" else getattr(getattr(twin, blk), a)
        assert np.array_equal(var.numpy(), other.numpy()), nm
    changed = {v.name for v in net.variables if not np.array_equal(v.numpy(), before[v.name])}
    assert changed <= trained, "written outside the 26 trained variables: %s" % sorted(changed - trained)
    assert changed == trained
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


def test_last_block_gradients_equal_last_block_trainer():
    """with Bottleneck5_0's 13 gradients ignored, the other 13 equal LastBlockTrainer.gradient_features on the same a5_0,
    bit for bit, and so does the loss"""
    net, _ = make_model(19, 3, seed=0)
    x = syn.synth_frames_device(0, 2, 64, 128, 3)
    rng = np.random.default_rng(4)
    labels = rng.integers(0, 19, (2, 64, 128)).astype(np.uint8)
    mask = (rng.uniform(size=(2, 64, 128)) > 0.2).astype(np.float32)
    ts, tb = LastStageTrainer.from_params(net, AL_PARAMS), LastBlockTrainer.from_params(net, AL_PARAMS)
    feats, am = ts.features(x)
    a5 = tb.features(x)
    ls_, gs = ts.gradient_features(feats, am, labels, mask)
    lb_, gb = tb.gradient_features(a5, labels, mask)
    assert torch.equal(ls_, lb_)
    for nm in lbo.NAMES:
        assert torch.equal(gs[nm], gb[nm]), nm
    assert all(float(gs[nm].abs().max()) > 0.0 for nm in lso.STAGE_NAMES)


def test_end_to_end_last_stage_learns():
    """section 15's setup: labels from the original head's argmax, reinitialize(0), 50 steps at the reference's settings: the
    loss ends at <= 0.9 x its first value; LastBlockTrainer's figure on the same start is printed next to it"""
    out = {}
    for cls in (LastBlockTrainer, LastStageTrainer):
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
    assert out["LastStageTrainer"][0] == out["LastBlockTrainer"][0]  # the same start, the same forward
    assert out["LastStageTrainer"][-1] <= 0.9 * out["LastStageTrainer"][0]


def test_invalid_arguments_on_device():
    net = ssal.ENet(19)
    net.build((None, None, None, 3))
    tr = LastStageTrainer(net, 1e-3)
    x = torch.zeros((1, 4, 4, 64), device="cuda")
    am = torch.as_tensor(lso.random_argmax(np.random.default_rng(0), 1, 4, 4)).cuda()
    lab, msk = np.zeros((1, 16, 16), np.uint8), np.ones((1, 16, 16), np.float32)
    with pytest.raises(ValueError):
        tr.gradient_features(x, am + 32, lab, msk)  # a device tensor of indices outside their windows
    with pytest.raises(ValueError):
        tr.gradient_features(x, am, lab[:, :8], msk)
    with pytest.raises(ValueError):
        tr.step(torch.zeros((1, 16, 16, 3), device="cuda"), lab[:, :8], msk)
