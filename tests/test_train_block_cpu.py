"""Last-block training without a GPU: the float64 oracle's 13 gradients against central finite
differences, the reference's JSON keys, the errors the trainer must raise, the state round trip, the ABI symbols and the size
limits of the workspace queries."""
import ctypes

import numpy as np
import pytest

import semanticsegmentationactivelearning_amd as ssal
from semanticsegmentationactivelearning_amd import _lib
from semanticsegmentationactivelearning_amd.training import FinalLayerTrainer, LastBlockTrainer

import last_block_train_oracle as lbo

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


def test_oracle_gradients_match_finite_differences():
    """N = 1, 4 x 6 features, K = 3, weight 1.02, label smoothing 0.1: every entry of the 13 gradients against central
    differences of the float64 loss (no PReLU input within 1e-4 of its kink, so the differences do not straddle it)"""
    k, weight, ls = 3, 1.02, 0.1
    rng = np.random.default_rng(0)
    x = rng.standard_normal((1, 4, 6, 16)).astype(np.float32)
    labels = rng.integers(0, k, (1, 8, 12)).astype(np.uint8)
    mask = (rng.uniform(size=(1, 8, 12)) > 0.2).astype(np.float32)
    labels[0, 0, :3] = 255  # ignored pixels: label 255 under mask 0 (there TensorFlow's softmax - y is not the derivative)
    mask[0, 0, :3] = 0.0
    params, stats = lbo.random_params(1, k)
    _, g, smallest = lbo.loss_and_grads(x, params, stats, labels, mask, weight, ls)
    assert smallest > 1e-4
    eps = 1e-6
    for name in lbo.NAMES:
        base = params[name].astype(np.float64)
        fd = np.zeros_like(base)
        for idx in np.ndindex(*base.shape):
            vals = []
            for sgn in (1.0, -1.0):
                p = dict(params)
                q = base.copy()
                q[idx] += sgn * eps
                p[name] = q
                vals.append(lbo.loss_and_grads(x, p, stats, labels, mask, weight, ls)[0])
            fd[idx] = (vals[0] - vals[1]) / (2 * eps)
        err, scale = np.abs(g[name] - fd).max(), max(np.abs(fd).max(), 1e-3)
        print("%-32s max |g - fd| %.3e, max |fd| %.3e" % (name, err, scale))
        # central differences: O(eps^2) truncation + O(1e-16 / eps) cancellation
        assert err <= 1e-6 * scale, name


def test_from_params_reads_the_reference_keys():
    tr = LastBlockTrainer.from_params(_net(), AL_PARAMS)
    assert (tr.learning_rate, tr.beta1, tr.beta2, tr.epsilon) == (0.0005, 0.9, 0.99, 1e-8)
    assert (tr.l1, tr.l2, tr.weight, tr.label_smoothing, tr.learning_rate_decay) == (0.0, 0.0002, 1.02, 0.0, 0.0)
    assert LastBlockTrainer.from_params(_net(), AL_PARAMS["hyperparams"]).l2 == 0.0002
    assert isinstance(tr, FinalLayerTrainer) and "LastBlockTrainer" in ssal.training.__all__


def test_not_implemented_and_value_errors():
    hp = AL_PARAMS["hyperparams"]
    with pytest.raises(NotImplementedError):
        LastBlockTrainer.from_params(_net(), {"hyperparams": dict(hp, softmax=dict(hp["softmax"], multiscale=True))})
    with pytest.raises(NotImplementedError):
        LastBlockTrainer.from_params(_net(), {"hyperparams": dict(hp, weight_reg=dict(hp["weight_reg"], glorot_scaling=True))})
    with pytest.raises(NotImplementedError):
        LastBlockTrainer(ssal.ICNet(19), 1e-3)
    big = ssal.ENet(33)
    big.build((None, None, None, 3))
    with pytest.raises(ValueError):
        LastBlockTrainer(big, 1e-3)
    with pytest.raises(ValueError):
        LastBlockTrainer(_net(), 1e-3, learning_rate_decay=0.5)  # decay without decay_steps
    tr = LastBlockTrainer(_net(), 1e-3)
    x = np.zeros((1, 8, 8, 16), np.float32)
    lab, mk = np.zeros((1, 16, 16), np.uint8), np.ones((1, 16, 16), np.float32)
    # the semi-supervised keywords of section 16 are out of scope here: judged before any device work
    for kw in ({"labelled": np.array([0])}, {"confusion": np.zeros((19, 19), np.int64)}, {"return_pseudo_pixels": True}):
        with pytest.raises(NotImplementedError):
            tr.gradient_features(x, lab, mk, **kw)
        with pytest.raises(NotImplementedError):
            tr.step_features(x, lab, mk, **kw)
        with pytest.raises(NotImplementedError):
            tr.step(np.zeros((1, 16, 16, 3), np.float32), lab, mk, **kw)
    with pytest.raises(NotImplementedError):
        tr.step(np.zeros((1, 16, 16, 3), np.float32), lab, mk, images_raw=np.zeros((1, 16, 16, 3), np.float32))


def test_state_round_trip_and_reinitialize():
    net = _net(6)
    tr = LastBlockTrainer(net, 1e-3, 0.9, 0.99)
    names = tr.variable_names
    assert names == list(lbo.NAMES) and len(names) == 13
    st = tr.state
    assert st["t"] == 0 and set(st["m"]) == set(names) and not any(a.any() for a in st["m"].values())
    assert st["m"]["Bottleneck5_1.conv_kernel"].shape == (3, 3, 4, 4) and st["v"]["Final.kernel"].shape == (3, 3, 6, 16)
    rng = np.random.default_rng(0)
    m = {n: rng.standard_normal(a.shape).astype(np.float32) for n, a in st["m"].items()}
    v = {n: rng.uniform(size=a.shape).astype(np.float32) for n, a in st["v"].items()}
    tr.load_state({"m": m, "v": v, "t": 7})
    back = tr.state
    assert back["t"] == 7
    assert all(np.array_equal(back["m"][n], m[n]) and np.array_equal(back["v"][n], v[n]) for n in names)
    b1p = np.float32(1.0)
    for _ in range(8):  # the beta power AdamOptimizer holds before step t + 1 = 8
        b1p = np.float32(b1p * np.float32(0.9))
    assert tr._b1p == b1p
    with pytest.raises(ValueError):
        tr.load_state({"m": {"Final.kernel": m["Final.kernel"]}, "v": v, "t": 0})
    with pytest.raises(ValueError):
        tr.load_state({"m": dict(m, **{"Final.kernel": np.zeros((3, 3, 5, 16), np.float32)}), "v": v, "t": 0})
    # reinitialize: the head only, and all optimiser state
    block_before = {n: getattr(net.Bottleneck5_1, n.split(".")[1]).numpy().copy() for n in names[1:]}
    head_before = net.Final.kernel.numpy().copy()
    tr.reinitialize(seed=3)
    assert not np.array_equal(head_before, net.Final.kernel.numpy())
    assert all(np.array_equal(block_before[n], getattr(net.Bottleneck5_1, n.split(".")[1]).numpy()) for n in names[1:])
    st = tr.state
    assert st["t"] == 0 and not any(a.any() for a in st["m"].values()) and not any(a.any() for a in st["v"].values())


def test_abi_symbols_and_packed_size():
    L = _lib.lib()
    for sym in ("ssal_train_block_param_floats", "ssal_train_block_grad_workspace_bytes", "ssal_train_block_grad_nhwc",
                "ssal_enet_train_block_workspace_bytes", "ssal_enet_train_block_nhwc"):
        assert hasattr(L, sym), sym
    assert L.ssal_train_block_param_floats(19) == 400 + 144 * 19
    assert L.ssal_train_block_param_floats(1) == -1 and L.ssal_train_block_param_floats(33) == -1
    assert LastBlockTrainer(_net(19), 1e-3)._floats() == L.ssal_train_block_param_floats(19)
    p = ctypes.c_void_p(16)
    assert L.ssal_train_block_grad_nhwc(p, 1, 8, 8, 33, p, p, p, 0.0, 0.0, p, p, p, 1 << 20, None) == _lib.SSAL_EINVAL
    assert L.ssal_train_block_grad_nhwc(p, 1, 1 << 30, 8, 19, p, p, p, 0.0, 0.0, p, p, p, 1 << 20, None) == _lib.SSAL_EINVAL
    assert L.ssal_train_block_grad_nhwc(p, 1, 8, 8, 19, None, p, p, 0.0, 0.0, p, p, p, 1 << 20, None) == _lib.SSAL_EINVAL
    assert L.ssal_enet_train_block_workspace_bytes(None, 1, 64, 64) == -1
    assert L.ssal_enet_train_block_features_offset(None, 1, 64, 64) == -1


def test_workspace_size_limit_boundaries():
    """-1 exactly where ssal_final_grad_workspace_bytes gives it, a positive size just inside"""
    L = _lib.lib()
    ws, ref = L.ssal_train_block_grad_workspace_bytes, L.ssal_final_grad_workspace_bytes
    cases = [(1, (1 << 30) - 1, 1, 19), (1, 1 << 30, 1, 19), (1, 1, (1 << 30) - 1, 19), (1, 1, 1 << 30, 19),
             (1, 16 * 46340, 16 * 46340, 19), (1, 16 * 46341, 16 * 46341, 19), (1, 64, 64, 1), (1, 64, 64, 33),
             (1, 64, 64, 2), (1, 64, 64, 32), (0, 64, 64, 19)]
    for c in cases:
        assert (ws(*c) == -1) == (ref(*c) == -1), c
        assert ws(*c) == -1 or ws(*c) > 0
    assert ws(1, (1 << 30) - 1, 1, 19) > 0 and ws(1, 1 << 30, 1, 19) == -1
    assert ws(1, 16 * 46340, 16 * 46340, 19) > 0 and ws(1, 16 * 46341, 16 * 46341, 19) == -1
    # dL/d(Bottleneck5_1 output) [n, h, w, 16] fp32 is part of the workspace
    assert ws(8, 512, 1024, 19) >= 8 * 512 * 1024 * 16 * 4
