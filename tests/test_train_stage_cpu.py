"""Last-stage training without a GPU: the float64 oracle's 26 gradients against central finite
differences, the packed stage block, the state keys, the regularised set, the errors the trainer must raise (the pooling
indices among them), the ABI symbols and the size limits of the workspace queries."""
import ctypes

import numpy as np
import pytest

import semanticsegmentationactivelearning_amd as ssal
from semanticsegmentationactivelearning_amd import _lib, training
from semanticsegmentationactivelearning_amd import synthetic as syn
from semanticsegmentationactivelearning_amd.training import LastBlockTrainer, LastStageTrainer

import last_block_train_oracle as lbo
import last_stage_train_oracle as lso

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
    """N = 1, a4_2 3 x 4, K = 3, weight 1.02, label smoothing 0.1: every entry of the 26 gradients against central
    differences of the float64 loss, to 1e-6 relative (no PReLU input within 1e-4 of its kink); of proj_kernel, res_kernel and
    conv_kernel of Bottleneck5_0 (over 1000 entries each) 96 entries drawn once"""
    k, weight, ls = 3, 1.02, 0.1
    rng = np.random.default_rng(0)
    x = (rng.standard_normal((1, 3, 4, 64)) * 0.7).astype(np.float32)
    am = lso.random_argmax(rng, 1, 3, 4)
    labels = rng.integers(0, k, (1, 12, 16)).astype(np.uint8)
    mask = (rng.uniform(size=(1, 12, 16)) > 0.2).astype(np.float32)
    labels[0, 0, :3] = 255  # ignored pixels: label 255 under mask 0
    mask[0, 0, :3] = 0.0
    params, stats = lso.random_params(3, k)
    _, g, pre = lso.loss_and_grads(x, am, params, stats, labels, mask, weight, ls)
    assert np.abs(pre).min() > 1e-4
    eps = 1e-6
    for name in lso.NAMES:
        base = params[name].astype(np.float64)
        fd = np.zeros_like(base)
        entries = list(np.ndindex(*base.shape))
        if len(entries) > 500:  # the three large kernels: 96 entries drawn once
            entries = [entries[i] for i in np.random.default_rng(5).choice(len(entries), 96, replace=False)]
        for idx in entries:
            vals = []
            for sgn in (1.0, -1.0):
                p = dict(params)
                q = base.copy()
                q[idx] += sgn * eps
                p[name] = q
                vals.append(lso.loss_and_grads(x, am, p, stats, labels, mask, weight, ls)[0])
            fd[idx] = (vals[0] - vals[1]) / (2 * eps)
        sel = tuple(np.array(entries).T)
        err, scale = np.abs(g[name][sel] - fd[sel]).max(), max(np.abs(fd).max(), 1e-3)
        print("%-32s max |g - fd| %.3e, max |fd| %.3e" % (name, err, scale))
        assert err <= 1e-6 * scale, name


def test_unpool_backward_is_the_gather():
    """the three positions of a window the index does not name carry no gradient into res_kernel: moving the gradient of
    those positions changes nothing"""
    import torch
    rng = np.random.default_rng(1)
    am = torch.as_tensor(lso.random_argmax(rng, 1, 2, 3))
    r = torch.as_tensor(rng.standard_normal((1, 2, 3, 16))).requires_grad_(True)
    up = lso.unpool_2d(r, am)
    g = torch.as_tensor(rng.standard_normal(up.shape))
    (up * g).sum().backward()
    assert np.array_equal(r.grad.numpy().reshape(-1), g.numpy().reshape(-1)[am.numpy().reshape(-1)])
    assert int((up != 0).sum()) == r.numel()


def test_names_layout_and_pack_round_trip():
    net = _net(6)
    tr = LastStageTrainer(net, 1e-3, 0.9, 0.99)
    names = tr.variable_names
    assert names == list(lso.NAMES) and len(names) == 26 and names[:13] == list(lbo.NAMES)
    assert isinstance(tr, LastBlockTrainer) and "LastStageTrainer" in training.__all__
    L = _lib.lib()
    assert tr._floats() == L.ssal_train_stage_param_floats(6) == 400 + 144 * 6 + 3536
    # every variable has its own range; the ranges are disjoint and leave the statistics out
    used = np.zeros(tr._floats(), np.int32)
    for name, var, off, _ in tr._named():
        used[off:off + int(np.prod(var.shape))] += 1
    assert used.max() == 1 and int(used.sum()) == 344 + 144 * 6 + 3448
    syn.randomize_enet(net, seed=3)
    packed = tr._pack()
    back = tr._unpack(packed)
    for name, var, off, _ in tr._named():
        assert np.array_equal(back[name], var.numpy()), name
    s0 = 400 + 144 * 6
    blk = net.Bottleneck5_0
    assert np.array_equal(packed[s0:s0 + 1024], blk.proj_kernel.numpy().reshape(-1))
    assert np.array_equal(packed[s0 + 1072:s0 + 2224], blk.conv_kernel.numpy().reshape(-1))
    assert np.array_equal(packed[s0 + 2408:s0 + 3432], blk.res_kernel.numpy().reshape(-1))
    for a, off, cnt in (("proj_mean", 3448, 16), ("proj_variance", 3464, 16), ("conv_mean", 3480, 8),
                        ("conv_variance", 3488, 8), ("exp_mean", 3496, 16), ("exp_variance", 3512, 16)):
        assert np.array_equal(packed[s0 + off:s0 + off + cnt], getattr(blk, a).numpy()), a
    assert not packed[s0 + 3528:].any()
    # the last-block part is LastBlockTrainer's block, float for float
    assert np.array_equal(packed[:s0], LastBlockTrainer(net, 1e-3)._pack())
    # a name -> array mapping packs without the statistics
    only = tr._pack(back)
    assert not only[s0 + 3448:].any() and np.array_equal(only[s0:s0 + 3448], packed[s0:s0 + 3448])


def test_regularised_set_and_adam_ranges():
    tr = LastStageTrainer(_net(19), 1e-3)
    reg = {n for n, _, _, r in tr._named() if r}
    assert reg == set(lso.REGULARISED) and len(reg) == 14
    covered = np.zeros(tr._floats(), np.int32)
    flag = np.zeros(tr._floats(), np.int32)
    for lo, hi, r in tr._adam_ranges():
        covered[lo:hi] += 1
        flag[lo:hi] = int(r)
    want = np.zeros(tr._floats(), np.int32)
    want_reg = np.zeros(tr._floats(), np.int32)
    for name, var, off, r in tr._named():
        want[off:off + int(np.prod(var.shape))] = 1
        want_reg[off:off + int(np.prod(var.shape))] = int(r)
    assert np.array_equal(covered, want) and np.array_equal(flag, want_reg)
    # LastBlockTrainer keeps its eight ranges
    assert len(LastBlockTrainer(_net(19), 1e-3)._adam_ranges()) == 8 and len(tr._adam_ranges()) == 15


def test_state_keys_and_reinitialize():
    net = _net(6)
    tr = LastStageTrainer(net, 1e-3, 0.9, 0.99)
    st = tr.state
    assert st["t"] == 0 and set(st["m"]) == set(lso.NAMES) == set(st["v"])
    assert st["m"]["Bottleneck5_0.conv_kernel"].shape == (3, 3, 8, 16) and st["v"]["Bottleneck5_0.res_kernel"].shape == (1, 1, 64, 16)
    rng = np.random.default_rng(0)
    m = {n: rng.standard_normal(a.shape).astype(np.float32) for n, a in st["m"].items()}
    v = {n: rng.uniform(size=a.shape).astype(np.float32) for n, a in st["v"].items()}
    tr.load_state({"m": m, "v": v, "t": 4})
    back = tr.state
    assert back["t"] == 4 and all(np.array_equal(back["m"][n], m[n]) and np.array_equal(back["v"][n], v[n]) for n in m)
    with pytest.raises(ValueError):
        tr.load_state({"m": {n: m[n] for n in lbo.NAMES}, "v": v, "t": 0})  # the 13 names of the last block are not enough
    before = {n: var.numpy().copy() for n, var, _, _ in tr._named()}
    tr.reinitialize(seed=3)
    assert not np.array_equal(before["Final.kernel"], net.Final.kernel.numpy())
    assert all(np.array_equal(before[n], var.numpy()) for n, var, _, _ in tr._named() if n != "Final.kernel")
    assert tr.state["t"] == 0 and not any(a.any() for a in tr.state["m"].values())


def test_not_implemented_and_value_errors():
    hp = AL_PARAMS["hyperparams"]
    tr = LastStageTrainer.from_params(_net(), AL_PARAMS)
    assert (tr.learning_rate, tr.beta2, tr.l2, tr.weight) == (0.0005, 0.99, 0.0002, 1.02)
    with pytest.raises(NotImplementedError):
        LastStageTrainer.from_params(_net(), {"hyperparams": dict(hp, softmax=dict(hp["softmax"], multiscale=True))})
    with pytest.raises(NotImplementedError):
        LastStageTrainer.from_params(_net(), {"hyperparams": dict(hp, weight_reg=dict(hp["weight_reg"], glorot_scaling=True))})
    with pytest.raises(NotImplementedError):
        LastStageTrainer(ssal.ICNet(19), 1e-3)
    big = ssal.ENet(33)
    big.build((None, None, None, 3))
    with pytest.raises(ValueError):
        LastStageTrainer(big, 1e-3)
    x = np.zeros((1, 4, 4, 64), np.float32)
    am = lso.random_argmax(np.random.default_rng(0), 1, 4, 4)
    lab, mk = np.zeros((1, 16, 16), np.uint8), np.ones((1, 16, 16), np.float32)
    for kw in ({"labelled": np.array([0])}, {"confusion": np.zeros((19, 19), np.int64)}, {"return_pseudo_pixels": True}):
        with pytest.raises(NotImplementedError):
            tr.gradient_features(x, am, lab, mk, **kw)
        with pytest.raises(NotImplementedError):
            tr.step_features(x, am, lab, mk, **kw)
        with pytest.raises(NotImplementedError):
            tr.step(np.zeros((1, 16, 16, 3), np.float32), lab, mk, **kw)
    # a block below Bottleneck5_0 is out of scope; a name that is no variable at all is a mistake
    with pytest.raises(NotImplementedError):
        tr.gradient_features(x, am, lab, mk, params={"Bottleneck4_2.proj_kernel": np.zeros((1, 1, 64, 16), np.float32)})
    with pytest.raises(ValueError):
        tr.gradient_features(x, am, lab, mk, params={"Bottleneck5_0.proj_mean": np.zeros((16,), np.float32)})
    with pytest.raises(ValueError):
        tr.gradient_features(x, am, lab, mk, max_workgroups=-1)


def test_bad_argmax_raises_before_any_device_work():
    tr = LastStageTrainer(_net(), 1e-3)
    x = np.zeros((1, 4, 6, 64), np.float32)
    lab, mk = np.zeros((1, 16, 24), np.uint8), np.ones((1, 16, 24), np.float32)
    good = lso.random_argmax(np.random.default_rng(0), 1, 4, 6)
    assert tr._check_argmax("argmax1", 64, 16, x.shape, good).shape == (1, 4, 6, 16)
    bad = {}
    bad["shape"] = good[:, :, :, :8]
    bad["other window"] = good.copy()
    bad["other window"][0, 1, 2, 3] += 2 * 16  # one pixel pair to the right: the neighbouring window
    bad["other row"] = good.copy()
    bad["other row"][0, 0, 0, 0] += 2 * (2 * 6) * 16  # two rows down
    bad["other channel"] = good.copy()
    bad["other channel"][0, 3, 5, 7] += 1
    bad["negative"] = good.copy()
    bad["negative"][0, 0, 0, 0] = -1
    bad["float"] = good.astype(np.float32)
    for what, am in bad.items():
        for call in (lambda a: tr.gradient_features(x, a, lab, mk), lambda a: tr.step_features(x, a, lab, mk)):
            with pytest.raises(ValueError):
                call(am)
    with pytest.raises(ValueError):
        tr.gradient_features(np.zeros((1, 4, 6, 16), np.float32), good, lab, mk)  # features of the wrong block


def test_abi_symbols_and_documented_sizes():
    """fails on a library without the last-stage entries"""
    L = _lib.lib()
    for sym in ("ssal_train_stage_param_floats", "ssal_train_stage_grad_workspace_bytes", "ssal_train_stage_grad_nhwc",
                "ssal_enet_train_stage_workspace_bytes", "ssal_enet_train_stage_nhwc", "ssal_enet_train_stage_features_offset",
                "ssal_enet_train_stage_code_offset"):
        assert hasattr(L, sym), sym
    assert L.ssal_train_stage_param_floats(19) == 400 + 144 * 19 + 3536 == L.ssal_train_block_param_floats(19) + 3536
    assert L.ssal_train_stage_param_floats(1) == -1 and L.ssal_train_stage_param_floats(33) == -1
    assert LastStageTrainer(_net(19), 1e-3)._floats() == L.ssal_train_stage_param_floats(19)
    # the workspace: the last-block workspace on the [2h, 2w] map, a5_0 and dL/d a5_0 [n, 2h, 2w, 16], the window codes, the
    # folded weights, one partial row of 3448 floats per workgroup (each piece rounded up to 256 bytes)
    n, h, w, k = 2, 20, 34, 19
    tiles = -(-2 * h // 16) * -(-2 * w // 16)
    r = lambda b: -(-b // 256) * 256
    want = (L.ssal_train_block_grad_workspace_bytes(n, 2 * h, 2 * w, k) - 256) + 2 * r(n * 4 * h * w * 16 * 4) \
        + r(n * h * w * 16) + r(4 * (128 + 6 * 16 * 16)) + r(4 * tiles * 3448) + 256
    got = L.ssal_train_stage_grad_workspace_bytes(n, h, w, k)
    assert abs(got - want) <= 7 * 256 and got >= want - 256, (got, want)
    p = ctypes.c_void_p(16)
    args = lambda n, h, w, k, params=p, mw=0, nbytes=1 << 20: (p, p, n, h, w, k, params, p, p, 0.0, 0.0, mw, p, p, p, nbytes, None)
    assert L.ssal_train_stage_grad_nhwc(*args(1, 8, 8, 33)) == _lib.SSAL_EINVAL
    assert L.ssal_train_stage_grad_nhwc(*args(1, 1 << 29, 8, 19)) == _lib.SSAL_EINVAL
    assert L.ssal_train_stage_grad_nhwc(*args(1, 8, 8, 19, params=None)) == _lib.SSAL_EINVAL
    assert L.ssal_train_stage_grad_nhwc(*args(1, 8, 8, 19, mw=-1)) == _lib.SSAL_EINVAL
    assert L.ssal_train_stage_grad_nhwc(*args(1, 8, 8, 19, nbytes=16)) == _lib.SSAL_ENOMEM  # judged before any launch
    assert L.ssal_enet_train_stage_workspace_bytes(None, 1, 64, 64) == -1
    assert L.ssal_enet_train_stage_features_offset(None, 1, 64, 64) == -1
    assert L.ssal_enet_train_stage_code_offset(None, 1, 64, 64) == -1


def test_workspace_size_limit_boundaries():
    """-1 exactly where the output-layer gradient on the [2h, 2w] map or the fused Bottleneck5_0 kernel (64 h w < 2^31)
    gives out, a positive size just inside"""
    L = _lib.lib()
    ws, ref = L.ssal_train_stage_grad_workspace_bytes, L.ssal_final_grad_workspace_bytes
    up_fits = lambda h, w: 64 * h * w < 2 ** 31
    cases = [(1, 4096, 8191, 19), (1, 4096, 8192, 19), (1, 1, (1 << 25) - 1, 19), (1, 1, 1 << 25, 19), ((1), (1 << 25) - 1, 1, 19),
             (1, 1 << 25, 1, 19), (1, 64, 64, 1), (1, 64, 64, 33), (1, 64, 64, 2), (1, 64, 64, 32), (0, 64, 64, 19),
             (1, 1 << 29, 1, 19)]
    for n, h, w, k in cases:
        inside = ref(n, min(2 * h, (1 << 31) - 1), min(2 * w, (1 << 31) - 1), k) != -1 and up_fits(h, w)
        assert (ws(n, h, w, k) != -1) == inside, (n, h, w, k)
        assert ws(n, h, w, k) == -1 or ws(n, h, w, k) > 0
    assert ws(1, 4096, 8191, 19) > 0 and ws(1, 4096, 8192, 19) == -1
    assert ws(8, 256, 512, 19) >= 2 * 8 * 512 * 1024 * 16 * 4
