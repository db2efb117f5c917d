"""Deep-tail training (Bottleneck4_1 + the decoder tail) without a GPU: the float64 oracle's gradients
against central finite differences, the packed block and its offsets, the 50 names, the regularised set, the errors the trainer
must raise before any device work, the ABI symbols and the size limits of the workspace queries."""
import ctypes

import numpy as np
import pytest

import semanticsegmentationactivelearning_amd as ssal
from semanticsegmentationactivelearning_amd import _lib, training
from semanticsegmentationactivelearning_amd import synthetic as syn
from semanticsegmentationactivelearning_amd.training import (DecoderTailTrainer, DeepTailTrainer, SemiSupervisedDeepTailTrainer,
                                                             SemiSupervisedTailTrainer)

import decoder_tail_train_oracle as dto
import deep_tail_train_oracle as ddo
import last_stage_train_oracle as lso

AL_PARAMS = {"hyperparams": {
    "dropout_rates": [0.01, 0.1, 0.1, 0.1, 0.1], "learning_rate": 0.0005, "learning_rate_decay": 0.0,
    "optimizer": {"type": "Adam", "kwargs": {"beta1": 0.9, "beta2": 0.99}},
    "weight_reg": {"L2": 0.0002, "L1": 0.0, "glorot_scaling": False},
    "softmax": {"label_smoothing": 0.0, "loginverse_scaling": 1.02, "multiscale": False}}}

# a regular bottleneck's part of the packed block (include/ssal_enet.h, "Decoder-tail training": the TT_* layout)
TT_OFFSETS = {"proj_kernel": 0, "proj_gamma": 1024, "proj_beta": 1040, "proj_alpha": 1056, "conv_kernel": 1072,
              "conv_gamma": 3376, "conv_beta": 3392, "conv_alpha": 3408, "exp_kernel": 3424, "exp_gamma": 4448,
              "exp_beta": 4512, "residual_alpha": 4576, "proj_mean": 4640, "proj_variance": 4656, "conv_mean": 4672,
              "conv_variance": 4688, "exp_mean": 4704, "exp_variance": 4768}
SYMBOLS = ("ssal_train_tail2_param_floats", "ssal_train_tail2_grad_workspace_bytes", "ssal_train_tail2_grad_nhwc",
           "ssal_enet_train_tail2_workspace_bytes", "ssal_enet_train_tail2_nhwc", "ssal_enet_train_tail2_features_offset",
           "ssal_train_tail2_grad_semi_workspace_bytes", "ssal_train_tail2_grad_semi_nhwc",
           "ssal_enet_train_tail2_semi_workspace_bytes", "ssal_enet_train_tail2_semi_nhwc")


def _net(k=19):
    net = ssal.ENet(k)
    net.build((None, None, None, 3))
    return net


def test_oracle_gradients_match_finite_differences():
    """N = 1, a4_0 3 x 4, K = 3, weight 1.02, label smoothing 0.1: every entry of the gradients against central differences
    of the float64 loss, to 1e-6 relative (no PReLU input within 1e-4 of its kink); of the kernels with over 500 entries 96
    entries drawn once"""
    k, weight, ls = 3, 1.02, 0.1
    rng = np.random.default_rng(0)
    x = (rng.standard_normal((1, 3, 4, 64)) * 0.7).astype(np.float32)
    am = lso.random_argmax(rng, 1, 3, 4)
    labels = rng.integers(0, k, (1, 12, 16)).astype(np.uint8)
    mask = (rng.uniform(size=(1, 12, 16)) > 0.2).astype(np.float32)
    labels[0, 0, :3] = 255  # ignored pixels: label 255 under mask 0
    mask[0, 0, :3] = 0.0
    params, stats = ddo.random_params(5, k)  # the first parameter seed from 3 up that keeps every PReLU input 1e-4 off its kink
    _, g, pre = ddo.loss_and_grads(x, am, params, stats, labels, mask, weight, ls)
    assert np.abs(pre).min() > 1e-4
    assert pre.size == 2 * 12 * (16 + 16 + 64) + 12 * 16 + 48 * (8 + 16) + 48 * (4 + 4 + 16)  # twelve PReLUs
    assert np.array_equal(pre, ddo.prelu_inputs(x, am, params, stats))
    eps = 1e-6
    for name in ddo.NAMES:
        base = params[name].astype(np.float64)
        fd = np.zeros_like(base)
        entries = list(np.ndindex(*base.shape))
        if len(entries) > 500:
            entries = [entries[i] for i in np.random.default_rng(5).choice(len(entries), 96, replace=False)]
        for idx in entries:
            vals = []
            for sgn in (1.0, -1.0):
                p = dict(params)
                q = base.copy()
                q[idx] += sgn * eps
                p[name] = q
                vals.append(ddo.loss_and_grads(x, am, p, stats, labels, mask, weight, ls)[0])
            fd[idx] = (vals[0] - vals[1]) / (2 * eps)
        sel = tuple(np.array(entries).T)
        err, scale = np.abs(g[name][sel] - fd[sel]).max(), max(np.abs(fd).max(), 1e-3)
        print("%-32s max |g - fd| %.3e, max |fd| %.3e" % (name, err, scale))
        assert err <= 1e-6 * scale, name


def test_oracle_parameters_extend_the_tails():
    """the 38 shared parameters are decoder_tail_train_oracle's for the same seed; Bottleneck4_1's come from their own generator"""
    p, st = ddo.random_params(7, 19)
    q, sq = dto.random_params(7, 19)
    assert all(np.array_equal(p[n], q[n]) for n in dto.NAMES) and set(p) == set(ddo.NAMES)
    assert all(np.array_equal(st[b][a], sq[b][a]) for b in sq for a in sq[b]) and set(st) == set(sq) | {"Bottleneck4_1"}
    assert not np.array_equal(p["Bottleneck4_1.proj_kernel"], p["Bottleneck4_2.proj_kernel"])


def test_names_layout_and_pack_round_trip():
    """50 names, the tail's 38 first, then Bottleneck4_1's twelve at T2 + TT_*, T2 = 3936 + 144 K + 4840"""
    k = 6
    net = _net(k)
    tr = DeepTailTrainer(net, 1e-3, 0.9, 0.99)
    names = tr.variable_names
    assert names == list(ddo.NAMES) and names[:38] == list(dto.NAMES) and len(names) == 50
    assert names[38:] == ["Bottleneck4_1." + a for a in ddo.DEEP_VARS]
    assert isinstance(tr, DecoderTailTrainer) and "DeepTailTrainer" in training.__all__
    assert issubclass(SemiSupervisedDeepTailTrainer, DeepTailTrainer) and "SemiSupervisedDeepTailTrainer" in training.__all__
    assert not issubclass(SemiSupervisedDeepTailTrainer, SemiSupervisedTailTrainer)
    L = _lib.lib()
    t2 = 3936 + 144 * k + 4840
    assert L.ssal_train_tail_param_floats(k) == t2
    assert tr._floats() == L.ssal_train_tail2_param_floats(k) == t2 + 4840
    for name, var, off, _ in tr._named()[38:]:
        assert off == t2 + TT_OFFSETS[name.split(".")[1]], name
    used = np.zeros(tr._floats(), np.int32)
    for name, var, off, _ in tr._named():
        used[off:off + int(np.prod(var.shape))] += 1
    assert used.max() == 1 and int(used[t2:].sum()) == 4640
    syn.randomize_enet(net, seed=3)
    packed = tr._pack()
    back = tr._unpack(packed)
    for name, var, off, _ in tr._named():
        assert np.array_equal(back[name], var.numpy()), name
    for a, off in TT_OFFSETS.items():
        v = getattr(net.Bottleneck4_1, a).numpy().reshape(-1)
        assert np.array_equal(packed[t2 + off:t2 + off + v.size], v), a
    assert not packed[t2 + 4832:].any()
    # the prefix is DecoderTailTrainer's block, float for float
    assert np.array_equal(packed[:t2], DecoderTailTrainer(net, 1e-3)._pack())
    only = tr._pack(back)
    assert not only[t2 + 4640:].any() and np.array_equal(only[t2:t2 + 4640], packed[t2:t2 + 4640])
    st = tr.state
    assert set(st["m"]) == set(ddo.NAMES) and st["m"]["Bottleneck4_1.conv_kernel"].shape == (3, 3, 16, 16)
    tr.load_state(st)
    with pytest.raises(ValueError):
        tr.load_state({"m": {n: st["m"][n] for n in dto.NAMES}, "v": st["v"], "t": 0})  # the tail's 38 names are not enough


def test_regularised_set_and_adam_ranges():
    tr = DeepTailTrainer(_net(19), 1e-3)
    reg = {n for n, _, _, r in tr._named() if r}
    assert reg == set(ddo.REGULARISED) and len(reg) == 14 + 6 + 6
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
    tail = DecoderTailTrainer(_net(19), 1e-3)._adam_ranges()
    assert len(tail) == 22 and len(tr._adam_ranges()) == 22 + 7 and tr._adam_ranges()[:22] == tail
    # the trained variables are the last ones of the model, so the trunk handle's version check covers everything below
    net = tr.net
    n_tail = tr._trained_tail()
    assert {v.name for v in net.variables[-n_tail:]} >= {var.name for _, var, _, _ in tr._named()}
    assert all(v.name.split("/")[0] in ("Bottleneck4_1", "Bottleneck4_2", "Bottleneck5_0", "Bottleneck5_1", "Final")
               for v in net.variables[-n_tail:])
    assert any(v.name.split("/")[0] == "Bottleneck4_1" for v in net.variables[-n_tail:])


def test_not_implemented_and_value_errors_before_any_device_work(monkeypatch):
    def no_gpu():
        raise AssertionError("device work before the host-side verdict")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    hp = AL_PARAMS["hyperparams"]
    x = np.zeros((1, 4, 4, 64), np.float32)
    am = lso.random_argmax(np.random.default_rng(0), 1, 4, 4)
    lab, mk = np.zeros((1, 16, 16), np.uint8), np.ones((1, 16, 16), np.float32)
    for cls in (DeepTailTrainer, SemiSupervisedDeepTailTrainer):
        tr = cls.from_params(_net(), AL_PARAMS)
        assert (tr.learning_rate, tr.beta2, tr.l2, tr.weight) == (0.0005, 0.99, 0.0002, 1.02)
        with pytest.raises(NotImplementedError):
            cls.from_params(_net(), {"hyperparams": dict(hp, softmax=dict(hp["softmax"], multiscale=True))})
        with pytest.raises(NotImplementedError):
            cls.from_params(_net(), {"hyperparams": dict(hp, weight_reg=dict(hp["weight_reg"], glorot_scaling=True))})
        with pytest.raises(NotImplementedError):
            cls(ssal.ICNet(19), 1e-3)
        # a block below Bottleneck4_1 is out of scope; Bottleneck4_1 itself is not; a name that is no variable is a mistake
        with pytest.raises(NotImplementedError):
            tr.gradient_features(x, am, lab, mk, params={"Bottleneck4_0.proj_kernel": np.zeros((1, 1, 128, 32), np.float32)})
        with pytest.raises(ValueError):
            tr.gradient_features(x, am, lab, mk, params={"Bottleneck4_1.proj_mean": np.zeros((16,), np.float32)})
        with pytest.raises(ValueError):
            tr.gradient_features(x, am, lab, mk, params={"Bottleneck4_1.proj_kernel": np.zeros((1, 1, 64, 8), np.float32)})
        with pytest.raises(ValueError):
            tr.gradient_features(x, am, lab, mk, max_workgroups=-1)
        with pytest.raises(ValueError):
            tr.gradient_features(x, am[:, :, :, :8], lab, mk)
        with pytest.raises(ValueError):
            tr.step_features(x, am + 32, lab, mk)
    plain = DeepTailTrainer(_net(), 1e-3)
    for kw in ({"labelled": np.array([0])}, {"confusion": np.zeros((19, 19), np.int64)}, {"return_pseudo_pixels": True}):
        with pytest.raises(NotImplementedError):
            plain.gradient_features(x, am, lab, mk, **kw)
        with pytest.raises(NotImplementedError):
            plain.step_features(x, am, lab, mk, **kw)
        with pytest.raises(NotImplementedError):
            plain.step(np.zeros((1, 16, 16, 3), np.float32), lab, mk, **kw)
    semi = SemiSupervisedDeepTailTrainer(_net(), 1e-3)
    with pytest.raises(ValueError):
        semi.gradient_features(x, am, lab, mk, labelled=np.array([0, 1]))
    with pytest.raises(NotImplementedError):
        semi.gradient_features(x, am, lab, mk, labelled=np.array([0]), measure="nope")
    big = ssal.ENet(33)
    big.build((None, None, None, 3))
    with pytest.raises(ValueError):
        DeepTailTrainer(big, 1e-3)
    # the tail trainer still refuses Bottleneck4_1
    with pytest.raises(NotImplementedError):
        DecoderTailTrainer(_net(), 1e-3).gradient_features(
            x, am, lab, mk, params={"Bottleneck4_1.proj_kernel": np.zeros((1, 1, 64, 16), np.float32)})


def test_abi_symbols_statuses_and_sizes():
    """fails on a library without the ten two-block entries"""
    L = _lib.lib()
    for sym in SYMBOLS:
        assert hasattr(L, sym), sym
    for k in (2, 19, 32):
        assert L.ssal_train_tail2_param_floats(k) == L.ssal_train_tail_param_floats(k) + 4840 == 3936 + 144 * k + 2 * 4840
    assert L.ssal_train_tail2_param_floats(1) == -1 and L.ssal_train_tail2_param_floats(33) == -1
    # the workspace: the tail's, a4_1 and dL/d a4_1 [n, h, w, 64], a second set of folded scalars and of partial rows
    n, h, w, k = 2, 20, 34, 19
    tiles = -(-h // 8) * -(-w // 8)
    r = lambda b: -(-b // 256) * 256
    want = L.ssal_train_tail_grad_workspace_bytes(n, h, w, k) + 2 * r(n * h * w * 64 * 4) + r(4 * 288) + r(4 * tiles * 4640)
    got = L.ssal_train_tail2_grad_workspace_bytes(n, h, w, k)
    assert abs(got - want) <= 4 * 256 and got >= want - 256, (got, want)  # (each piece starts at a multiple of 256 bytes)
    more = L.ssal_train_tail_grad_semi_workspace_bytes(n, h, w, k, 1) - L.ssal_train_tail_grad_workspace_bytes(n, h, w, k)
    assert abs(L.ssal_train_tail2_grad_semi_workspace_bytes(n, h, w, k, 1) - got - more) <= 2 * 256
    p = ctypes.c_void_p(16)
    args = lambda n, h, w, k, params=p, mw=0, nbytes=1 << 20: (p, p, n, h, w, k, params, p, p, 0.0, 0.0, mw, p, p, p, nbytes, None)
    assert L.ssal_train_tail2_grad_nhwc(*args(1, 8, 8, 1)) == _lib.SSAL_EINVAL
    assert L.ssal_train_tail2_grad_nhwc(*args(1, 8, 8, 33)) == _lib.SSAL_EINVAL
    assert L.ssal_train_tail2_grad_nhwc(*args(1, 1 << 29, 8, 19)) == _lib.SSAL_EINVAL
    assert L.ssal_train_tail2_grad_nhwc(*args(1, 8, 8, 19, params=None)) == _lib.SSAL_EINVAL
    assert L.ssal_train_tail2_grad_nhwc(*args(1, 8, 8, 19, mw=-1)) == _lib.SSAL_EINVAL
    assert L.ssal_train_tail2_grad_nhwc(*args(1, 8, 8, 19, nbytes=16)) == _lib.SSAL_ENOMEM  # judged before any launch
    # a workspace that holds the one-block call but not the two-block one: refused before any launch as well
    one = L.ssal_train_tail_grad_workspace_bytes(1, 8, 8, 19)
    assert one < L.ssal_train_tail2_grad_workspace_bytes(1, 8, 8, 19)
    assert L.ssal_train_tail2_grad_nhwc(*args(1, 8, 8, 19, nbytes=one)) == _lib.SSAL_ENOMEM
    sargs = lambda measure, raw=(p, p): (p, p) + raw + (1, 8, 8, 19, p, p, p, p, measure, 0.0, 0.0, 0.0, 0, p, p, p, p, p, 16, None)
    assert L.ssal_train_tail2_grad_semi_nhwc(*sargs(7)) == _lib.SSAL_ENOTIMPL
    assert L.ssal_train_tail2_grad_semi_nhwc(*sargs(0, raw=(p, None))) == _lib.SSAL_EINVAL
    assert L.ssal_train_tail2_grad_semi_nhwc(*sargs(0)) == _lib.SSAL_ENOMEM
    assert L.ssal_enet_train_tail2_workspace_bytes(None, 1, 64, 64) == -1
    assert L.ssal_enet_train_tail2_semi_workspace_bytes(None, 1, 64, 64, 1) == -1
    assert L.ssal_enet_train_tail2_features_offset(None, 1, 64, 64) == -1


def test_workspace_size_limit_boundaries():
    """the limits are the tail's: -1 exactly where the one-block queries give -1, a larger positive size elsewhere"""
    L = _lib.lib()
    ws, tail = L.ssal_train_tail2_grad_workspace_bytes, L.ssal_train_tail_grad_workspace_bytes
    semi, tail_semi = L.ssal_train_tail2_grad_semi_workspace_bytes, L.ssal_train_tail_grad_semi_workspace_bytes
    cases = [(1, 4096, 8191, 19), (1, 4096, 8192, 19), (1, 1, (1 << 25) - 1, 19), (1, 1, 1 << 25, 19), (1, (1 << 25) - 1, 1, 19),
             (1, 1 << 25, 1, 19), (1, 64, 64, 1), (1, 64, 64, 33), (1, 64, 64, 2), (1, 64, 64, 32), (0, 64, 64, 19),
             (1, 1 << 29, 1, 19), (1, 2048, 4096, 19), (1, 2048, 4097, 19), (1, 1, 1 << 23, 19), (1, (1 << 23) + 1, 1, 19)]
    for n, h, w, k in cases:
        assert (ws(n, h, w, k) == -1) == (tail(n, h, w, k) == -1), (n, h, w, k)
        for raw in (0, 1):
            assert (semi(n, h, w, k, raw) == -1) == (tail_semi(n, h, w, k, raw) == -1), (n, h, w, k, raw)
        assert ws(n, h, w, k) == -1 or ws(n, h, w, k) > tail(n, h, w, k) > 0
    assert ws(1, 2048, 4096, 19) > 0 and ws(1, 2048, 4097, 19) == -1
    assert ws(8, 256, 512, 19) >= tail(8, 256, 512, 19) + 2 * 8 * 256 * 512 * 64 * 4
