"""Output-layer training without a GPU: the float64 oracle's gradient against finite differences, the float32 Adam
restatement against the closed form, the reference's JSON keys, training_targets, and the gradient kernel's size limit."""
import ctypes

import numpy as np
import pytest

import semanticsegmentationactivelearning_amd as ssal
from semanticsegmentationactivelearning_amd import _lib
from semanticsegmentationactivelearning_amd import active_learning as al
from semanticsegmentationactivelearning_amd.training import FinalLayerTrainer

import final_train_oracle as fto


def _tiny_case(seed=0, k=3, n=2, h=4, w=6):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, h, w, 16)).astype(np.float32)
    kern = rng.uniform(-0.4, 0.4, (3, 3, k, 16)).astype(np.float32)
    labels = rng.integers(0, k, (n, 2 * h, 2 * w)).astype(np.uint8)
    mask = (rng.uniform(size=(n, 2 * h, 2 * w)) > 0.2).astype(np.float32)
    labels[0, 0, :3] = 255  # ignored pixels: label 255 under mask 0
    mask[0, 0, :3] = 0.0
    return x, kern, labels, mask


def _loss64(x, kern, labels, mask, weight, ls):
    return fto.loss_and_grad(x, kern, labels, mask, weight, ls)[0]


def test_oracle_gradient_matches_finite_differences():
    """weight = 1.02, ls = 0.1: the float64 gradient (with the p_class term) agrees with central differences of the
    loss; leaving the p_class term out does not"""
    x, kern, labels, mask = _tiny_case()
    weight, ls = 1.02, 0.1
    _, g = fto.loss_and_grad(x, kern, labels, mask, weight, ls)
    _, g_stop = fto.loss_and_grad(x, kern, labels, mask, weight, ls, p_class_gradient=False)
    kd = kern.astype(np.float64)
    eps = 1e-6
    fd = np.zeros_like(kd)
    for idx in np.ndindex(*kd.shape):
        kp, km = kd.copy(), kd.copy()
        kp[idx] += eps
        km[idx] -= eps
        fd[idx] = (_loss64(x, kp, labels, mask, weight, ls) - _loss64(x, km, labels, mask, weight, ls)) / (2 * eps)
    err = np.abs(g - fd).max()
    scale = np.abs(fd).max()
    print("max |g - fd| = %.3e, max |fd| = %.3e, max |g_stop - fd| = %.3e" % (err, scale, np.abs(g_stop - fd).max()))
    # central differences: O(eps^2) truncation + O(1e-16 / eps) cancellation, both far below 1e-7 of the scale
    assert err <= 1e-7 * scale
    assert np.abs(g_stop - fd).max() > 1e-3 * scale  # the p_class term is not negligible here


def test_oracle_gradient_is_softmax_minus_y_for_an_all_off_row():
    """a label >= K under mask 1: TensorFlow backpropagates softmax - y (not the derivative of sum(y) * lse)"""
    import torch
    k = 4
    on, off, _, _ = fto.xent_constants(k, 0.0, 0.1)
    lg = torch.tensor([[[[0.3, -1.0, 2.0, 0.5]]]], dtype=torch.float64, requires_grad=True)
    y = fto.one_hot(np.array([[[255]]], np.uint8), k, on, off)
    fto.pixel_loss(lg, y, torch.ones((1, 1, 1), dtype=torch.float64), 0.0, 0.0).sum().backward()
    want = torch.softmax(lg.detach(), -1) - y
    assert torch.allclose(lg.grad, want, rtol=0, atol=1e-15)
    assert float(y.sum()) == pytest.approx(4 * off)


def test_adam_restatement_matches_closed_form():
    """constant gradient, zero slots: m_t = g (1 - b1^t), v_t = g^2 (1 - b2^t), so every step moves w by
    lr g / (|g| + eps / sqrt(1 - b2^t)); three float32 steps against the float64 closed form"""
    rng = np.random.default_rng(1)
    w0 = rng.standard_normal(64).astype(np.float32)
    g = rng.standard_normal(64).astype(np.float32)
    lr, b1, b2, eps = 5e-4, 0.9, 0.99, 1e-8
    w, m, v = w0.copy(), np.zeros(64, np.float32), np.zeros(64, np.float32)
    b1p, b2p = np.float32(b1), np.float32(b2)
    want = w0.astype(np.float64)
    b1d, b2d = float(np.float32(b1)), float(np.float32(b2))  # the closed form of the fp32 hyper-parameters
    for t in range(1, 4):
        w, m, v = fto.adam_step(w, m, v, g, lr, b1, b2, eps, b1p, b2p)
        b1p, b2p = np.float32(b1p * np.float32(b1)), np.float32(b2p * np.float32(b2))
        gd = g.astype(np.float64)
        want -= float(np.float32(lr)) * gd / (np.abs(gd) + eps / np.sqrt(1 - b2d ** t))
        assert np.allclose(m, gd * (1 - b1d ** t), rtol=1e-6, atol=0)
        assert np.allclose(v, gd * gd * (1 - b2d ** t), rtol=1e-6, atol=0)
        # float32 w (|w| ~ 1) after t updates of 5e-4: a few ulp of w per step
        assert np.abs(w - want).max() <= 4 * t * 2.0 ** -24 * np.abs(want).max()


def test_adam_restatement_regulariser():
    """l2 adds 2 l2 w, l1 adds l1 sign(w) with sign(0) = 0"""
    w = np.array([-2.0, 0.0, 3.0], np.float32)
    g = np.zeros(3, np.float32)
    z = np.zeros(3, np.float32)
    _, m, _ = fto.adam_step(w, z, z, g, 1e-3, 0.5, 0.5, 1e-8, 0.5, 0.5, l1=0.25, l2=0.125)
    # m = g_total * (1 - b1) = 0.5 * (2 * 0.125 * w + 0.25 * sign(w))
    assert m.tolist() == [0.5 * (-0.5 - 0.25), 0.0, 0.5 * (0.75 + 0.25)]


# the reference's conf/enet_cityscapes_active_learning.json "hyperparams" section, key for key
AL_PARAMS = {"hyperparams": {
    "dropout_rates": [0.01, 0.1, 0.1, 0.1, 0.1], "learning_rate": 0.0005, "learning_rate_decay": 0.0,
    "optimizer": {"type": "Adam", "kwargs": {"beta1": 0.9, "beta2": 0.99}},
    "weight_reg": {"L2": 0.0002, "L1": 0.0, "glorot_scaling": False},
    "softmax": {"label_smoothing": 0.0, "loginverse_scaling": 1.02, "multiscale": False}}}


def _net(k=19):
    net = ssal.ENet(k)
    net.build((None, None, None, 3))
    return net


def test_from_params_reads_the_reference_keys():
    tr = FinalLayerTrainer.from_params(_net(), AL_PARAMS)
    assert (tr.learning_rate, tr.beta1, tr.beta2, tr.epsilon) == (0.0005, 0.9, 0.99, 1e-8)
    assert (tr.l1, tr.l2, tr.weight, tr.label_smoothing, tr.learning_rate_decay) == (0.0, 0.0002, 1.02, 0.0, 0.0)
    tr2 = FinalLayerTrainer.from_params(_net(), AL_PARAMS["hyperparams"])  # the section alone
    assert tr2.l2 == 0.0002
    p = {"hyperparams": dict(AL_PARAMS["hyperparams"], learning_rate_decay=0.5)}
    tr3 = FinalLayerTrainer.from_params(_net(), p, decay_steps=10)
    tr3._t = 5
    assert tr3.current_learning_rate() == np.float32(np.float32(0.0005) / np.float32(1 + np.float32(0.5) * np.float32(0.5)))
    with pytest.raises(ValueError):
        FinalLayerTrainer.from_params(_net(), p)  # decay without decay_steps
    ms = {"hyperparams": dict(AL_PARAMS["hyperparams"], softmax={"label_smoothing": 0.0, "loginverse_scaling": 0.0,
                                                                 "multiscale": True})}
    with pytest.raises(NotImplementedError):
        FinalLayerTrainer.from_params(_net(), ms)


def test_trainer_rejects_icnet_and_reinitializes():
    icn = ssal.ICNet(19)
    with pytest.raises(NotImplementedError):
        FinalLayerTrainer(icn, 1e-3)
    net = _net(6)
    tr = FinalLayerTrainer(net, 1e-3)
    before = net.Final.kernel.numpy().copy()
    tr.reinitialize(seed=3)
    a = net.Final.kernel.numpy().copy()
    tr.reinitialize(seed=3)
    assert np.array_equal(a, net.Final.kernel.numpy()) and not np.array_equal(a, before)
    limit = np.sqrt(6.0 / (9 * 6 + 9 * 16))  # glorot: fan_in = 9 K, fan_out = 9 * 16 for the [3, 3, K, 16] kernel
    assert np.abs(a).max() <= limit
    st = tr.state
    assert st["t"] == 0 and not st["m"].any() and not st["v"].any()


def test_training_targets_per_image():
    labelled = np.array([True, False, True])
    labels = np.arange(3 * 2 * 2, dtype=np.uint8).reshape(3, 2, 2)
    mask = np.ones((3, 2, 2), np.uint8)
    pl = np.full((3, 2, 2), 7, np.int64)
    pm = np.array([[[0, 1], [1, 0]]] * 3, np.int64)
    lab, mk = al.training_targets(labelled, labels, mask, pl, pm)
    assert lab.dtype == np.uint8 and mk.dtype == np.uint8
    assert np.array_equal(lab[0], labels[0]) and np.array_equal(lab[2], labels[2]) and (lab[1] == 7).all()
    assert np.array_equal(mk[1], pm[1]) and (mk[0] == 1).all()
    import torch
    tl, tm = al.training_targets(torch.as_tensor(labelled), torch.as_tensor(labels), torch.as_tensor(mask),
                                 torch.as_tensor(pl), torch.as_tensor(pm))
    assert np.array_equal(tl.numpy(), lab) and np.array_equal(tm.numpy(), mk)
    with pytest.raises(ValueError):
        al.training_targets(labelled[:2], labels, mask, pl, pm)


def test_final_grad_size_limit_boundaries():
    """ssal_final_grad_workspace_bytes = -1 exactly beyond the kernel's int limits: 2h + 1 / 2w + 1 and the count of
    16 x 16 tiles"""
    L = _lib.lib()
    ws = L.ssal_final_grad_workspace_bytes
    assert ws(1, (1 << 30) - 1, 1, 19) > 0
    assert ws(1, 1 << 30, 1, 19) == -1
    assert ws(1, 1, (1 << 30) - 1, 19) > 0
    assert ws(1, 1, 1 << 30, 19) == -1
    assert ws(1, 16 * 46340, 16 * 46340, 19) > 0     # 46340^2 = 2147395600 tiles
    assert ws(1, 16 * 46341, 16 * 46341, 19) == -1   # 46341^2 > 2^31 - 1
    assert ws(1, 64, 64, 1) == -1 and ws(1, 64, 64, 33) == -1 and ws(1, 64, 64, 2) > 0 and ws(1, 64, 64, 32) > 0
    assert ws(0, 64, 64, 19) == -1
    # partial rows: min(tiles, 1024) workgroups x 9 K 16 floats
    assert ws(8, 512, 1024, 19) >= 1024 * 9 * 19 * 16 * 4
    assert ws(1, 33, 65, 19) < 1024 * 9 * 19 * 16 * 4


def test_final_grad_entry_validates_without_a_gpu():
    L = _lib.lib()
    p = ctypes.c_void_p(16)
    rc = L.ssal_final_grad_nhwc(p, 1, 8, 8, 33, p, p, p, 0.0, 0.0, p, p, p, 1 << 20, None)
    assert rc == _lib.SSAL_EINVAL
    rc = L.ssal_final_grad_nhwc(p, 1, 1 << 30, 8, 19, p, p, p, 0.0, 0.0, p, p, p, 1 << 20, None)
    assert rc == _lib.SSAL_EINVAL
    assert L.ssal_adam_apply(p, p, p, p, 0, 1e-3, 0.9, 0.99, 1e-8, 0.9, 0.99, 0.0, 0.0, None) == _lib.SSAL_EINVAL
