"""Output-layer training on the MI355X: the fused head gradient against the float64 oracle,
elementwise; the loss against the forward op; determinism; Adam bit for bit against the float32 restatement; a short
end-to-end run; argument errors."""
import numpy as np
import pytest
import torch

import semanticsegmentationactivelearning_amd as ssal
from semanticsegmentationactivelearning_amd import _lib
from semanticsegmentationactivelearning_amd import synthetic as syn
from semanticsegmentationactivelearning_amd.tensortools import losses
from semanticsegmentationactivelearning_amd.training import FinalLayerTrainer

import final_train_oracle as fto
from helpers import frames, make_model

pytestmark = pytest.mark.gpu


def _case(seed, n, h, w, k, kernel_gain=0.3):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, h, w, 16)) * 0.7).astype(np.float32)
    kern = rng.uniform(-kernel_gain, kernel_gain, (3, 3, k, 16)).astype(np.float32)
    labels = rng.integers(0, k, (n, 2 * h, 2 * w)).astype(np.uint8)
    mask = (rng.uniform(size=(n, 2 * h, 2 * w)) > 0.25).astype(np.float32)
    ign = rng.uniform(size=labels.shape) < 0.05  # label 255 under both mask values
    labels[ign] = 255
    return x, kern, labels, mask


def _gpu_grad(net_k, x, kern, labels, mask, weight, ls):
    net = ssal.ENet(net_k)
    net.build((None, None, None, 3))
    tr = FinalLayerTrainer(net, 1e-3, loginverse_scaling=weight, label_smoothing=ls)
    loss, grad = tr.gradient_features(torch.as_tensor(x).cuda(), labels, mask, kernel=kern)
    torch.cuda.synchronize()
    return float(loss.cpu()[0]), grad.cpu().numpy()


def _check_elementwise(name, g, g64, c, kap):
    bound = kap * 2.0 ** -24 * c
    d = np.abs(g.astype(np.float64) - g64)
    ratio = float((d / np.maximum(bound, 1e-300)).max())
    print("%s: kappa %.0f, max |g - g64| %.3e, max |g - g64| / bound %.3e, max |g64| %.3e"
          % (name, kap, d.max(), ratio, np.abs(g64).max()))
    bad = d > bound
    assert not bad.any(), "%s: %d of %d entries beyond kappa 2^-24 C (first at %s)" % (
        name, int(bad.sum()), bad.size, tuple(int(i) for i in np.argwhere(bad)[0]))


CASES = [(k, weight, ls) for k in (2, 6, 19, 32) for weight in (0.0, 1.02) for ls in (0.0, 0.1)]


@pytest.mark.parametrize("k,weight,ls", CASES)
def test_gradient_matches_float64_oracle_elementwise(k, weight, ls):
    """|g - g64| <= kappa 2^-24 C_j for every entry; shapes that are not whole 16 x 16 tiles, N = 1 and N = 3"""
    idx = CASES.index((k, weight, ls))
    n, h, w = (1, 33, 65) if idx % 2 == 0 else (3, 20, 17)
    x, kern, labels, mask = _case(100 + idx, n, h, w, k)
    loss, g = _gpu_grad(k, x, kern, labels, mask, weight, ls)
    from oracle import enet_oracle as orc
    logits32 = orc.conv2d_transpose_3x3_s2(x, kern)
    g64, c, loss64 = fto.grad_and_bound(x, kern, labels, mask, weight, ls, logits32)
    _check_elementwise("K=%d w=%g ls=%g %dx%dx%d" % (k, weight, ls, n, h, w), g, g64, c,
                       fto.kappa(n, h, w, k, weight))
    assert abs(loss - loss64) <= 1e-5 * abs(loss64)


def test_gradient_full_size_batch():
    """one full-size batch: 8 x 512 x 1024 features (1024 x 2048 frames), K = 19, weight 1.02"""
    n, h, w, k, weight, ls = 8, 512, 1024, 19, 1.02, 0.0
    x, kern, labels, mask = _case(7, n, h, w, k)
    loss, g = _gpu_grad(k, x, kern, labels, mask, weight, ls)
    from oracle import enet_oracle as orc
    logits32 = orc.conv2d_transpose_3x3_s2(x, kern)
    g64, c, _ = fto.grad_and_bound(x, kern, labels, mask, weight, ls, logits32)
    _check_elementwise("full size", g, g64, c, fto.kappa(n, h, w, k, weight))


@pytest.mark.parametrize("weight,ls", [(0.0, 0.0), (1.02, 0.1)])
def test_loss_matches_forward_op(enet_c3k19, weight, ls):
    """the trainer's float64 loss against losses.masked_softmax_cross_entropy(labels, net(x), mask): per-pixel terms are
    bit-identical, only the float64 order differs: <= 2^24 * 2^-53 relative, bound 1e-8"""
    net, _ = enet_c3k19
    x = syn.synth_frames_device(0, 2, 64, 128, 3)
    rng = np.random.default_rng(5)
    labels = rng.integers(0, 19, (2, 64, 128)).astype(np.uint8)
    labels[:, :4] = 255
    mask = (rng.uniform(size=(2, 64, 128)) > 0.3).astype(np.float32)
    want = float(losses.masked_softmax_cross_entropy(torch.as_tensor(labels).cuda(), net(x, training=False),
                                                     torch.as_tensor(mask).cuda(), 19, weight, ls))
    feats = net.endpoint_outputs[0][1].clone()
    tr = FinalLayerTrainer(net, 1e-3, loginverse_scaling=weight, label_smoothing=ls)
    got_f = float(tr.gradient_features(feats, labels, mask)[0].cpu()[0])
    print("loss: forward op %.17g, gradient kernel %.17g, rel %.3e" % (want, got_f, abs(got_f - want) / want))
    assert abs(got_f - want) <= 1e-8 * abs(want)


def test_determinism_and_image_entry_matches_features(enet_c3k19):
    net0, P = enet_c3k19
    net = ssal.ENet(19)
    net.build((None, None, None, 3))
    net.assign_named({v.name: v.numpy() for v in net0.variables})
    x = syn.synth_frames_device(3, 2, 64, 128, 3)
    rng = np.random.default_rng(9)
    labels = rng.integers(0, 19, (2, 64, 128)).astype(np.uint8)
    mask = (rng.uniform(size=(2, 64, 128)) > 0.2).astype(np.float32)
    tr = FinalLayerTrainer(net, 5e-4, 0.9, 0.99, loginverse_scaling=1.02, label_smoothing=0.1, l2=2e-4)
    net(x, training=False)
    feats = net.endpoint_outputs[0][1].clone()
    l1, g1 = tr.gradient_features(feats, labels, mask)
    l2, g2 = tr.gradient_features(feats, labels, mask)
    assert torch.equal(g1, g2) and torch.equal(l1, l2)
    tr.reinitialize(seed=4)
    la = tr.step(x, labels, mask)
    ka = net.Final.kernel.numpy().copy()
    tr.reinitialize(seed=4)
    lb = tr.step_features(feats, labels, mask)
    kb = net.Final.kernel.numpy().copy()
    assert float(la) == float(lb), "step(images) loss %r != step_features loss %r" % (float(la), float(lb))
    assert np.array_equal(ka, kb)
    assert tr.state["t"] == 1


def test_adam_bit_identical_to_float32_restatement():
    """the GPU gradient fed to ssal_adam_apply and to the numpy ApplyAdam restatement: m, v and w bit-identical (sqrt and
    the divisions are correctly rounded on both sides); l1, l2 and sign(0) = 0 covered"""
    k = 19
    x, kern, labels, mask = _case(11, 2, 24, 40, k)
    kern[0, 0, :3, :] = 0.0  # exact zeros: sign(0) = 0
    _, g = _gpu_grad(k, x, kern, labels, mask, 1.02, 0.0)
    rng = np.random.default_rng(2)
    w = kern.copy()
    m = (rng.standard_normal(w.shape) * 1e-3).astype(np.float32)
    v = (rng.uniform(size=w.shape) * 1e-5).astype(np.float32)
    dw, dm, dv, dg = (torch.as_tensor(a).cuda() for a in (w, m, v, g))
    b1p, b2p = np.float32(0.9), np.float32(0.99)
    for step in range(3):
        lr = np.float32(5e-4)
        _lib.check(_lib.lib().ssal_adam_apply(_lib.dev_ptr(dw), _lib.dev_ptr(dm), _lib.dev_ptr(dv), _lib.dev_ptr(dg),
                                              w.size, float(lr), 0.9, 0.99, 1e-8, float(b1p), float(b2p), 1e-4, 2e-4,
                                              _lib.stream_ptr()))
        w, m, v = fto.adam_step(w, m, v, g, lr, 0.9, 0.99, 1e-8, b1p, b2p, l1=1e-4, l2=2e-4)
        b1p, b2p = np.float32(b1p * np.float32(0.9)), np.float32(b2p * np.float32(0.99))
        torch.cuda.synchronize()
        assert np.array_equal(dm.cpu().numpy(), m), "m differs at step %d" % step
        assert np.array_equal(dv.cpu().numpy(), v), "v differs at step %d" % step
        assert np.array_equal(dw.cpu().numpy(), w), "w differs at step %d" % step


def test_end_to_end_reinitialized_head_learns_and_score_uses_it():
    """labels from the original head's argmax, reinitialize, 50 steps at the reference's settings: the loss ends at
    <= 0.9 x its first value; then net(x) / net.score(x) use the new kernel (logits bit-identical to the C oracle's)"""
    net, _ = make_model(19, 3, seed=0)
    x = syn.synth_frames_device(0, 2, 64, 128, 3)
    _, extra = net.score(x, return_label=True)
    labels = extra["label"].clone()
    mask = torch.ones((2, 64, 128), dtype=torch.float32, device=x.device)
    params = {"hyperparams": {"learning_rate": 0.0005, "learning_rate_decay": 0.0,
                              "optimizer": {"type": "Adam", "kwargs": {"beta1": 0.9, "beta2": 0.99}},
                              "weight_reg": {"L2": 0.0002, "L1": 0.0},
                              "softmax": {"label_smoothing": 0.0, "loginverse_scaling": 1.02, "multiscale": False}}}
    tr = FinalLayerTrainer.from_params(net, params)
    tr.reinitialize(seed=0)
    losses_ = [float(tr.step(x, labels, mask)) for _ in range(50)]
    print("end to end: loss %.6g -> %.6g (x%.3f)" % (losses_[0], losses_[-1], losses_[-1] / losses_[0]))
    assert losses_[-1] <= 0.9 * losses_[0]
    from oracle import enet_oracle as orc
    P = syn.enet_params_dict(net)
    assert np.array_equal(P["Final.kernel"], net.Final.kernel.numpy())
    x_host = frames([0, 1], 64, 128, 3)
    want_mean, _, want_label, want_logits = orc.score_images(P, x_host, "entropy")
    scores, ex = net.score(x, return_label=True)
    logits = net(x, training=False)
    torch.cuda.synchronize()
    assert np.array_equal(logits.cpu().numpy(), want_logits)
    assert np.array_equal(ex["label"].cpu().numpy(), want_label)
    assert np.abs(scores.cpu().numpy() - want_mean).max() <= 1e-6


def test_invalid_arguments():
    net = ssal.ENet(19)
    net.build((None, None, None, 3))
    tr = FinalLayerTrainer(net, 1e-3)
    x = torch.zeros((1, 8, 8, 16), device="cuda")
    lab = np.zeros((1, 16, 16), np.uint8)
    msk = np.ones((1, 16, 16), np.float32)
    with pytest.raises(ValueError):
        tr.gradient_features(torch.zeros((1, 8, 8, 8), device="cuda"), lab, msk)  # wrong feature channels
    with pytest.raises(ValueError):
        tr.gradient_features(x, lab[:, :8], msk)  # label shape
    with pytest.raises(ValueError):
        tr.step(torch.zeros((1, 16, 16, 3), device="cuda"), lab[:, :8], msk)
    big = ssal.ENet(33)
    big.build((None, None, None, 3))
    with pytest.raises(ValueError):
        FinalLayerTrainer(big, 1e-3)  # K > 32
    p = _lib.lib()
    rc = p.ssal_final_grad_nhwc(_lib.dev_ptr(x), 1, 8, 8, 33, _lib.dev_ptr(x), _lib.dev_ptr(x), _lib.dev_ptr(x), 0.0, 0.0,
                                _lib.dev_ptr(x), _lib.dev_ptr(x), _lib.dev_ptr(x), 1 << 20, _lib.stream_ptr())
    assert rc == _lib.SSAL_EINVAL
    with pytest.raises(NotImplementedError):
        FinalLayerTrainer.from_params(net, {"learning_rate": 1e-3, "softmax": {"multiscale": True}})
    with pytest.raises(NotImplementedError):
        FinalLayerTrainer(ssal.ICNet(19), 1e-3)
    with pytest.raises(NotImplementedError):
        net(torch.zeros((1, 16, 16, 3), device="cuda"), training=True)
