"""Last-block training on the MI355X: the 13 gradients against the float64 oracle with the tolerance
measured from the reference arithmetic's own error; the loss against the forward op, bit for bit; determinism; Adam bit for
bit against the float32 restatement; the weights of record after three steps; a short end-to-end run."""
import numpy as np
import pytest
import torch

import semanticsegmentationactivelearning_amd as ssal
from semanticsegmentationactivelearning_amd import synthetic as syn
from semanticsegmentationactivelearning_amd.tensortools import losses
from semanticsegmentationactivelearning_amd.training import FinalLayerTrainer, LastBlockTrainer

import final_train_oracle as fto
import last_block_train_oracle as lbo
from helpers import frames, make_model

pytestmark = pytest.mark.gpu

AL_PARAMS = {"hyperparams": {"learning_rate": 0.0005, "learning_rate_decay": 0.0,
                             "optimizer": {"type": "Adam", "kwargs": {"beta1": 0.9, "beta2": 0.99}},
                             "weight_reg": {"L2": 0.0002, "L1": 0.0},
                             "softmax": {"label_smoothing": 0.0, "loginverse_scaling": 1.02, "multiscale": False}}}


def _case(seed, n, h, w, k):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, h, w, 16)) * 0.7).astype(np.float32)
    labels = rng.integers(0, k, (n, 2 * h, 2 * w)).astype(np.uint8)
    mask = (rng.uniform(size=(n, 2 * h, 2 * w)) > 0.25).astype(np.float32)
    labels[rng.uniform(size=labels.shape) < 0.05] = 255  # label 255 under both mask values
    params, stats = lbo.random_params(seed + 1000, k)
    return x, labels, mask, params, stats


def _net_with(k, params, stats):
    net = ssal.ENet(k)
    net.build((None, None, None, 3))
    net.Final.kernel.assign(params["Final.kernel"])
    for a in lbo.BLOCK_VARS:
        getattr(net.Bottleneck5_1, a).assign(params["%s.%s" % (lbo.BLOCK, a)])
    for a in lbo.STATS:
        getattr(net.Bottleneck5_1, a).assign(stats[a])
    return net


def _check_case(name, n, h, w, k, weight, ls, seed):
    x, labels, mask, params, stats = _case(seed, n, h, w, k)
    net = _net_with(k, params, stats)
    tr = LastBlockTrainer(net, 1e-3, loginverse_scaling=weight, label_smoothing=ls)
    xd = torch.as_tensor(x).cuda()
    loss, g = tr.gradient_features(xd, labels, mask)
    loss2, g2 = tr.gradient_features(xd, labels, mask)
    torch.cuda.synchronize()
    assert torch.equal(loss, loss2) and all(torch.equal(g[nm], g2[nm]) for nm in g), "two calls differ"
    # the forward the scoring path computes: Bottleneck5_1 and Final as layers of the model
    logits = net.Final(net.Bottleneck5_1(xd, training=False), training=False)
    want = losses.masked_softmax_cross_entropy(torch.as_tensor(labels).cuda(), logits, torch.as_tensor(mask).cuda(), k,
                                               weight, ls)
    got_loss, want_loss = float(loss.cpu()[0]), float(want)
    print("%s: loss %.17g, forward op %.17g" % (name, got_loss, want_loss))
    assert got_loss == want_loss, "loss %r != forward op %r" % (got_loss, want_loss)
    logits32 = logits.cpu().numpy()
    _, g64, smallest = lbo.loss_and_grads(x, params, stats, labels, mask, weight, ls, logits32=logits32)
    assert smallest > 0.0, "a PReLU input of the chosen data is exactly 0"
    _, g32, _ = lbo.loss_and_grads(x, params, stats, labels, mask, weight, ls, dtype=torch.float32)
    tol = lbo.tolerance(g32, g64)
    worst = {}
    for nm in lbo.NAMES:
        d = float(np.abs(g[nm].cpu().numpy().astype(np.float64) - g64[nm]).max())
        worst[nm] = d / tol[nm]
        print("%s: %-32s max |g - g64| %.3e, tolerance %.3e, ratio %.3f, max |g64| %.3e"
              % (name, nm, d, tol[nm], worst[nm], np.abs(g64[nm]).max()))
    bad = [nm for nm in lbo.NAMES if not worst[nm] <= 1.0]
    assert not bad, "%s: beyond max(8 e_ref, 2^-22 max |g64|): %s" % (name, bad)


CASES = [(k, weight, ls) for k in (2, 6, 19, 32) for weight in (0.0, 1.02) for ls in (0.0, 0.1)]


@pytest.mark.parametrize("k,weight,ls", CASES)
def test_gradients_match_float64_oracle(k, weight, ls):
    """max |g_gpu - g64| <= max(8 e_ref, 2^-22 max |g64|) per tensor, e_ref = max |g32 - g64| of float32 torch autograd of
    the same restatement; N = 1 (17 x 23 features) and N = 2 (20 x 33): neither is a multiple of the 16 x 16 tile.  N
    alternates so that, for every K, each N meets both weights and both smoothing values"""
    idx = CASES.index((k, weight, ls))
    n, h, w = (1, 17, 23) if (idx // 2 + idx) % 2 == 0 else (2, 20, 33)
    _check_case("K=%d w=%g ls=%g %dx%dx%d" % (k, weight, ls, n, h, w), n, h, w, k, weight, ls, 200 + idx)


def test_gradients_more_tiles_than_workgroups():
    """512 x 1024 features: 2048 tiles on 1024 workgroups; the oracle runs one image at a time"""
    _check_case("512x1024", 1, 512, 1024, 19, 1.02, 0.0, 77)


def test_adam_bit_identical_and_regulariser_ranges():
    """three step_features calls: every w, m, v equals final_train_oracle.adam_step fed with the GPU's own gradient; l1 / l2
    only on the variables the reference regularises"""
    k = 19
    x, labels, mask, params, stats = _case(31, 2, 24, 40, k)
    params["Final.kernel"][0, 0, :3, :] = 0.0  # exact zeros: sign(0) = 0
    net = _net_with(k, params, stats)
    tr = LastBlockTrainer(net, 5e-4, 0.9, 0.99, l1=1e-4, l2=2e-4, loginverse_scaling=1.02)
    xd = torch.as_tensor(x).cuda()
    w = {nm: np.array(params[nm]) for nm in lbo.NAMES}
    m = {nm: np.zeros_like(w[nm]) for nm in lbo.NAMES}
    v = {nm: np.zeros_like(w[nm]) for nm in lbo.NAMES}
    b1p, b2p = np.float32(0.9), np.float32(0.99)
    for step in range(3):
        _, g = tr.gradient_features(xd, labels, mask)
        tr.step_features(xd, labels, mask)
        st = tr.state
        for nm in lbo.NAMES:
            reg = nm in lbo.REGULARISED
            w[nm], m[nm], v[nm] = fto.adam_step(w[nm], m[nm], v[nm], g[nm].cpu().numpy(), np.float32(5e-4), 0.9, 0.99, 1e-8,
                                                b1p, b2p, l1=1e-4 if reg else 0.0, l2=2e-4 if reg else 0.0)
            var = net.Final.kernel if nm == "Final.kernel" else getattr(net.Bottleneck5_1, nm.split(".")[1])
            assert np.array_equal(st["m"][nm], m[nm]), "m of %s differs at step %d" % (nm, step)
            assert np.array_equal(st["v"][nm], v[nm]), "v of %s differs at step %d" % (nm, step)
            assert np.array_equal(var.numpy(), w[nm]), "%s differs at step %d" % (nm, step)
        b1p, b2p = np.float32(b1p * np.float32(0.9)), np.float32(b2p * np.float32(0.99))
    assert tr.state["t"] == 3
    for a in lbo.STATS:
        assert np.array_equal(getattr(net.Bottleneck5_1, a).numpy(), stats[a])


def test_image_entry_matches_features_and_weights_of_record():
    """step(images) == step_features(Bottleneck5_0 features); after three steps net(x) and net.score(x) use the new weights
    (bit-identical to the C oracle with the host variables), the statistics and everything below the block are unchanged"""
    from oracle import enet_oracle as orc
    net, _ = make_model(19, 3, seed=0)
    twin, _ = make_model(19, 3, seed=0)
    x = syn.synth_frames_device(0, 2, 64, 128, 3)
    rng = np.random.default_rng(9)
    labels = rng.integers(0, 19, (2, 64, 128)).astype(np.uint8)
    mask = (rng.uniform(size=(2, 64, 128)) > 0.2).astype(np.float32)
    before = {v.name: v.numpy().copy() for v in net.variables}
    trained = {"Final/Kernel"} | {getattr(net.Bottleneck5_1, a).name for a in lbo.BLOCK_VARS}
    tr = LastBlockTrainer.from_params(net, AL_PARAMS)
    tw = LastBlockTrainer.from_params(twin, AL_PARAMS)
    feats = tw.features(x)  # Bottleneck5_0's output
    assert tuple(feats.shape) == (2, 32, 64, 16)
    for step in range(3):
        la = tr.step(x, labels, mask)
        lb = tw.step_features(feats, labels, mask)
        assert float(la) == float(lb), "step %d: step(images) loss %r != step_features loss %r" % (step, float(la), float(lb))
    for a in lbo.BLOCK_VARS:
        assert np.array_equal(getattr(net.Bottleneck5_1, a).numpy(), getattr(twin.Bottleneck5_1, a).numpy()), a
    assert np.array_equal(net.Final.kernel.numpy(), twin.Final.kernel.numpy())
    changed = {v.name for v in net.variables if not np.array_equal(v.numpy(), before[v.name])}
    print("variables changed by three steps:", sorted(changed))
    assert changed <= trained, "written outside the 13 trained variables: %s" % sorted(changed - trained)
    assert changed == trained
    P = syn.enet_params_dict(net)
    want_mean, _, want_label, want_logits = orc.score_images(P, frames([0, 1], 64, 128, 3), "entropy")
    scores, ex = net.score(x, return_label=True)
    logits = net(x, training=False)
    torch.cuda.synchronize()
    assert np.array_equal(logits.cpu().numpy(), want_logits)
    assert np.array_equal(ex["label"].cpu().numpy(), want_label)
    assert np.abs(scores.cpu().numpy() - want_mean).max() <= 1e-6
    # and the loss of a further step is the forward op's on those logits, bit for bit
    want = float(losses.masked_softmax_cross_entropy(torch.as_tensor(labels).cuda(), logits, torch.as_tensor(mask).cuda(), 19,
                                                     1.02, 0.0))
    assert float(tr.step(x, labels, mask)) == want


def test_end_to_end_last_block_learns():
    """section 15's setup: labels from the original head's argmax, reinitialize(0), 50 steps at the reference's settings: the
    loss ends at <= 0.9 x its first value; FinalLayerTrainer's figure on the same start is printed next to it"""
    out = {}
    for cls in (FinalLayerTrainer, LastBlockTrainer):
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
    assert out["LastBlockTrainer"][0] == out["FinalLayerTrainer"][0]  # the same start, the same forward
    assert out["LastBlockTrainer"][-1] <= 0.9 * out["LastBlockTrainer"][0]


def test_invalid_arguments_on_device():
    net = ssal.ENet(19)
    net.build((None, None, None, 3))
    tr = LastBlockTrainer(net, 1e-3)
    x = torch.zeros((1, 8, 8, 16), device="cuda")
    lab, msk = np.zeros((1, 16, 16), np.uint8), np.ones((1, 16, 16), np.float32)
    with pytest.raises(ValueError):
        tr.gradient_features(torch.zeros((1, 8, 8, 8), device="cuda"), lab, msk)
    with pytest.raises(ValueError):
        tr.gradient_features(x, lab[:, :8], msk)
    with pytest.raises(ValueError):
        tr.gradient_features(x, lab, msk, params={"Bottleneck4_2.proj_kernel": np.zeros((1, 1, 64, 16), np.float32)})
    with pytest.raises(ValueError):
        tr.step(torch.zeros((1, 16, 16, 3), device="cuda"), lab[:, :8], msk)
