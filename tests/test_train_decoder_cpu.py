"""Decoder training (Bottleneck4_0 + the deep tail) without a GPU: the float64 oracle's gradients against
central finite differences, the packed block and its offsets, the 63 names, the regularised set, the errors the trainer must
raise before any device work, the ABI symbols and the size limits of the workspace queries."""
import ctypes

import numpy as np
import pytest

import semanticsegmentationactivelearning_amd as ssal
from semanticsegmentationactivelearning_amd import _lib, training
from semanticsegmentationactivelearning_amd import synthetic as syn
from semanticsegmentationactivelearning_amd.training import (DecoderTrainer, DeepTailTrainer, SemiSupervisedDecoderTrainer,
                                                             SemiSupervisedDeepTailTrainer)

import decoder_train_oracle as dco
import deep_tail_train_oracle as ddo
import last_stage_train_oracle as lso

AL_PARAMS = {"hyperparams": {
    "dropout_rates": [0.01, 0.1, 0.1, 0.1, 0.1], "learning_rate": 0.0005, "learning_rate_decay": 0.0,
    "optimizer": {"type": "Adam", "kwargs": {"beta1": 0.9, "beta2": 0.99}},
    "weight_reg": {"L2": 0.0002, "L1": 0.0, "glorot_scaling": False},
    "softmax": {"label_smoothing": 0.0, "loginverse_scaling": 1.02, "multiscale": False}}}

# Bottleneck4_0's part of the packed block (include/ssal_enet.h, "Decoder training": the TD_* layout of ssal_train_decoder.h)
TD_OFFSETS = {"proj_kernel": 0, "proj_gamma": 4096, "proj_beta": 4128, "proj_alpha": 4160, "conv_kernel": 4192,
              "conv_gamma": 8800, "conv_beta": 8816, "conv_alpha": 8832, "exp_kernel": 8848, "exp_gamma": 9872,
              "exp_beta": 9936, "res_kernel": 10000, "residual_alpha": 18192, "proj_mean": 18256, "proj_variance": 18288,
              "conv_mean": 18320, "conv_variance": 18336, "exp_mean": 18352, "exp_variance": 18416}
TD_TRAINED, TD_FLOATS = 18256, 18488
SYMBOLS = ("ssal_train_decoder_param_floats", "ssal_train_decoder_grad_workspace_bytes", "ssal_train_decoder_grad_nhwc",
           "ssal_enet_train_decoder_workspace_bytes", "ssal_enet_train_decoder_nhwc", "ssal_enet_train_decoder_features_offset",
           "ssal_train_decoder_grad_semi_workspace_bytes", "ssal_train_decoder_grad_semi_nhwc",
           "ssal_enet_train_decoder_semi_workspace_bytes", "ssal_enet_train_decoder_semi_nhwc")
PARAM_SEED = 5  # the first parameter seed from 3 up that keeps every PReLU input 1e-4 off its kink (asserted below)


def _net(k=19):
    net = ssal.ENet(k)
    net.build((None, None, None, 3))
    return net


def _fd_case():
    k = 3
    rng = np.random.default_rng(0)
    x = (rng.standard_normal((1, 2, 3, 128)) * 0.7).astype(np.float32)
    am2 = dco.random_argmax(rng, 1, 2, 3, 64)
    am1 = dco.random_argmax(rng, 1, 4, 6, 16)
    labels = rng.integers(0, k, (1, 16, 24)).astype(np.uint8)
    mask = (rng.uniform(size=(1, 16, 24)) > 0.2).astype(np.float32)
    labels[0, 0, :3] = 255  # ignored pixels: label 255 under mask 0
    mask[0, 0, :3] = 0.0
    return k, x, am2, am1, labels, mask


def test_oracle_gradients_match_finite_differences():
    """N = 1, a3_8 2 x 3, K = 3, weight 1.02, label smoothing 0.1: every entry of the 63 gradients against central differences
    of the float64 loss, to 1e-6 relative (no PReLU input within 1e-4 of its kink); of the kernels with over 500 entries 96
    entries drawn once"""
    weight, ls = 1.02, 0.1
    k, x, am2, am1, labels, mask = _fd_case()
    for seed in range(3, PARAM_SEED):  # the recipe: no earlier seed qualifies
        p, st = dco.random_params(seed, k)
        assert not np.abs(dco.prelu_inputs(x, am2, am1, p, st)).min() > 1e-4, seed
    params, stats = dco.random_params(PARAM_SEED, k)
    loss, g, pre = dco.loss_and_grads(x, am2, am1, params, stats, labels, mask, weight, ls)
    assert loss == dco.loss_only(x, am2, am1, params, stats, labels, mask, weight, ls)
    assert np.abs(pre).min() > 1e-4
    # 15 PReLUs: Bottleneck4_0 (6 + 24 + 24 pixels), two regular blocks on 24 pixels, Bottleneck5_0, Bottleneck5_1
    assert pre.size == 6 * 32 + 24 * (16 + 64) + 2 * 24 * (16 + 16 + 64) + 24 * 16 + 96 * (8 + 16) + 96 * (4 + 4 + 16)
    assert np.array_equal(pre, dco.prelu_inputs(x, am2, am1, params, stats))
    assert len(dco.NAMES) == 63 and dco.PRELUS == 15
    eps = 1e-6
    for name in dco.NAMES:
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
                vals.append(dco.loss_only(x, am2, am1, p, stats, labels, mask, weight, ls))
            fd[idx] = (vals[0] - vals[1]) / (2 * eps)
        sel = tuple(np.array(entries).T)
        err, scale = np.abs(g[name][sel] - fd[sel]).max(), max(np.abs(fd).max(), 1e-3)
        print("%-32s max |g - fd| %.3e, max |fd| %.3e" % (name, err, scale))
        assert err <= 1e-6 * scale, name


def test_oracle_parameters_extend_the_deep_tails():
    """the 50 shared parameters are deep_tail_train_oracle's for the same seed; Bottleneck4_0's come from their own generator"""
    p, st = dco.random_params(7, 19)
    q, sq = ddo.random_params(7, 19)
    assert all(np.array_equal(p[n], q[n]) for n in ddo.NAMES) and set(p) == set(dco.NAMES)
    assert all(np.array_equal(st[b][a], sq[b][a]) for b in sq for a in sq[b]) and set(st) == set(sq) | {"Bottleneck4_0"}
    assert all(p["Bottleneck4_0." + a].shape == dco.LOW_SHAPES[a] for a in dco.LOW_VARS)
    am = dco.random_argmax(np.random.default_rng(1), 2, 3, 5, 16)
    assert np.array_equal(am, lso.random_argmax(np.random.default_rng(1), 2, 3, 5))


def test_names_layout_and_pack_round_trip():
    """63 names, the deep tail's 50 first, then Bottleneck4_0's thirteen at T4 + TD_*, T4 = 3936 + 144 K + 2 x 4840"""
    k = 6
    net = _net(k)
    tr = DecoderTrainer(net, 1e-3, 0.9, 0.99)
    names = tr.variable_names
    assert names == list(dco.NAMES) and names[:50] == list(ddo.NAMES) and len(names) == 63
    assert names[50:] == ["Bottleneck4_0." + a for a in dco.LOW_VARS]
    assert isinstance(tr, DeepTailTrainer) and "DecoderTrainer" in training.__all__
    assert issubclass(SemiSupervisedDecoderTrainer, DecoderTrainer) and "SemiSupervisedDecoderTrainer" in training.__all__
    assert issubclass(SemiSupervisedDecoderTrainer, training._SemiKeywords)
    assert not issubclass(SemiSupervisedDecoderTrainer, SemiSupervisedDeepTailTrainer)
    L = _lib.lib()
    t4 = 3936 + 144 * k + 2 * 4840
    assert L.ssal_train_tail2_param_floats(k) == t4
    assert tr._floats() == L.ssal_train_decoder_param_floats(k) == t4 + TD_FLOATS
    for name, var, off, _ in tr._named()[50:]:
        assert off == t4 + TD_OFFSETS[name.split(".")[1]], name
        assert tuple(var.shape) == dco.LOW_SHAPES[name.split(".")[1]], name
    used = np.zeros(tr._floats(), np.int32)
    for name, var, off, _ in tr._named():
        used[off:off + int(np.prod(var.shape))] += 1
    assert used.max() == 1 and int(used[t4:].sum()) == TD_TRAINED and bool(used[t4:t4 + TD_TRAINED].all())
    syn.randomize_enet(net, seed=3)
    packed = tr._pack()
    back = tr._unpack(packed)
    for name, var, off, _ in tr._named():
        assert np.array_equal(back[name], var.numpy()), name
    for a, off in TD_OFFSETS.items():
        v = getattr(net.Bottleneck4_0, a).numpy().reshape(-1)
        assert np.array_equal(packed[t4 + off:t4 + off + v.size], v), a
    assert not packed[t4 + TD_FLOATS - 8:].any()
    # the prefix is DeepTailTrainer's block, float for float
    assert np.array_equal(packed[:t4], DeepTailTrainer(net, 1e-3)._pack())
    only = tr._pack(back)
    assert not only[t4 + TD_TRAINED:].any() and np.array_equal(only[t4:t4 + TD_TRAINED], packed[t4:t4 + TD_TRAINED])
    st = tr.state
    assert set(st["m"]) == set(dco.NAMES) and st["m"]["Bottleneck4_0.conv_kernel"].shape == (3, 3, 16, 32)
    tr.load_state(st)
    SemiSupervisedDecoderTrainer(net, 1e-3, 0.9, 0.99).load_state(st)  # interchangeable between the two classes
    with pytest.raises(ValueError):
        tr.load_state({"m": {n: st["m"][n] for n in ddo.NAMES}, "v": st["v"], "t": 0})  # the deep tail's 50 are not enough


def test_regularised_set_and_adam_ranges():
    tr = DecoderTrainer(_net(19), 1e-3)
    reg = {n for n, _, _, r in tr._named() if r}
    assert reg == set(dco.REGULARISED) and len(reg) == 14 + 6 + 6 + 7
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
    deep = DeepTailTrainer(_net(19), 1e-3)._adam_ranges()
    mine = tr._adam_ranges()
    assert len(deep) == 29 and len(mine) == 29 + 7 and mine[:29] == deep
    assert [r for _, _, r in mine[29:]] == [True, False, True, False, True, False, True]  # regularised and plain alternate
    t4 = 3936 + 144 * 19 + 2 * 4840
    assert mine[29][0] == t4 and mine[-1][1] == t4 + TD_TRAINED  # the six statistics are in no range
    # the trained variables are the last ones of the model, so the trunk handle's version check covers everything below
    net = tr.net
    n_tail = tr._trained_tail()
    assert {v.name for v in net.variables[-n_tail:]} >= {var.name for _, var, _, _ in tr._named()}
    blocks = ("Bottleneck4_0", "Bottleneck4_1", "Bottleneck4_2", "Bottleneck5_0", "Bottleneck5_1", "Final")
    assert all(v.name.split("/")[0] in blocks for v in net.variables[-n_tail:])
    assert any(v.name.split("/")[0] == "Bottleneck4_0" for v in net.variables[-n_tail:])


def test_not_implemented_and_value_errors_before_any_device_work(monkeypatch):
    def no_gpu():
        raise AssertionError("device work before the host-side verdict")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    hp = AL_PARAMS["hyperparams"]
    x = np.zeros((1, 2, 2, 128), np.float32)
    am2 = dco.random_argmax(np.random.default_rng(0), 1, 2, 2, 64)
    am1 = dco.random_argmax(np.random.default_rng(0), 1, 4, 4, 16)
    lab, mk = np.zeros((1, 16, 16), np.uint8), np.ones((1, 16, 16), np.float32)
    for cls in (DecoderTrainer, SemiSupervisedDecoderTrainer):
        tr = cls.from_params(_net(), AL_PARAMS)
        assert (tr.learning_rate, tr.beta2, tr.l2, tr.weight) == (0.0005, 0.99, 0.0002, 1.02)
        with pytest.raises(NotImplementedError):
            cls.from_params(_net(), {"hyperparams": dict(hp, softmax=dict(hp["softmax"], multiscale=True))})
        with pytest.raises(NotImplementedError):
            cls.from_params(_net(), {"hyperparams": dict(hp, weight_reg=dict(hp["weight_reg"], glorot_scaling=True))})
        with pytest.raises(NotImplementedError):
            cls(ssal.ICNet(19), 1e-3)
        # a block below Bottleneck4_0 is out of scope; Bottleneck4_0 itself is not; a name that is no variable is a mistake
        with pytest.raises(NotImplementedError):
            tr.gradient_features(x, am2, am1, lab, mk, params={"Bottleneck3_8.proj_kernel": np.zeros((1, 1, 128, 32), np.float32)})
        with pytest.raises(ValueError):
            tr.gradient_features(x, am2, am1, lab, mk, params={"Bottleneck4_0.proj_mean": np.zeros((32,), np.float32)})
        with pytest.raises(ValueError):
            tr.gradient_features(x, am2, am1, lab, mk, params={"Bottleneck4_0.proj_kernel": np.zeros((1, 1, 128, 8), np.float32)})
        with pytest.raises(ValueError):
            tr.gradient_features(x, am2, am1, lab, mk, max_workgroups=-1)
        # argmax2 is judged as argmax1 is: shape, window, channel, dtype
        with pytest.raises(ValueError, match="argmax2 must have shape"):
            tr.gradient_features(x, am2[:, :, :, :32], am1, lab, mk)
        with pytest.raises(ValueError, match="argmax2 must have shape"):
            tr.gradient_features(x, am1, am1, lab, mk)
        with pytest.raises(ValueError, match="argmax2 holds 256 indices"):
            tr.step_features(x, am2 + 2 * 4 * 64, am1, lab, mk)  # one row down: outside every window
        with pytest.raises(ValueError, match="argmax2 holds 256 indices"):
            tr.step_features(x, am2 + 1, am1, lab, mk)  # the next channel
        bad = am2.copy()
        bad[0, 1, 1, 5] = -1
        with pytest.raises(ValueError, match="argmax2 holds 1 indices"):
            tr.gradient_features(x, bad, am1, lab, mk)
        with pytest.raises(ValueError, match="integer"):
            tr.gradient_features(x, am2.astype(np.float32), am1, lab, mk)
        with pytest.raises(ValueError, match="argmax1"):
            tr.gradient_features(x, am2, am1[:, :, :, :8], lab, mk)
        with pytest.raises(ValueError, match="argmax1"):
            tr.step_features(x, am2, am1 + 32, lab, mk)
        with pytest.raises(ValueError):
            tr.gradient_features(x[..., :64], am2, am1, lab, mk)
    plain = DecoderTrainer(_net(), 1e-3)
    for kw in ({"labelled": np.array([0])}, {"confusion": np.zeros((19, 19), np.int64)}, {"return_pseudo_pixels": True},
               {"argmax2_raw": am2}):
        with pytest.raises(NotImplementedError):
            plain.gradient_features(x, am2, am1, lab, mk, **kw)
        with pytest.raises(NotImplementedError):
            plain.step_features(x, am2, am1, lab, mk, **kw)
    with pytest.raises(NotImplementedError):
        plain.step(np.zeros((1, 16, 16, 3), np.float32), lab, mk, labelled=np.array([0]))
    semi = SemiSupervisedDecoderTrainer(_net(), 1e-3)
    with pytest.raises(ValueError):
        semi.gradient_features(x, am2, am1, lab, mk, labelled=np.array([0, 1]))
    with pytest.raises(NotImplementedError):
        semi.gradient_features(x, am2, am1, lab, mk, labelled=np.array([0]), measure="nope")
    with pytest.raises(ValueError, match="together"):
        semi.gradient_features(x, am2, am1, lab, mk, labelled=np.array([0]), features_raw=x.copy(), argmax1_raw=am1)
    big = ssal.ENet(33)
    big.build((None, None, None, 3))
    with pytest.raises(ValueError):
        DecoderTrainer(big, 1e-3)
    # the deep-tail trainer still refuses Bottleneck4_0
    with pytest.raises(NotImplementedError):
        DeepTailTrainer(_net(), 1e-3).gradient_features(
            np.zeros((1, 4, 4, 64), np.float32), am1, lab, mk,
            params={"Bottleneck4_0.proj_kernel": np.zeros((1, 1, 128, 32), np.float32)})


def test_abi_symbols_statuses_and_sizes():
    """fails on a library without the ten decoder entries"""
    L = _lib.lib()
    for sym in SYMBOLS:
        assert hasattr(L, sym), sym
    for k in (2, 19, 32):
        assert L.ssal_train_decoder_param_floats(k) == L.ssal_train_tail2_param_floats(k) + TD_FLOATS
    assert L.ssal_train_decoder_param_floats(1) == -1 and L.ssal_train_decoder_param_floats(33) == -1
    # the workspace: the two-block tail's on the quarter-resolution map, a4_0 and dL/d a4_0 [n, 2h, 2w, 64], the gathered dL/du
    # and the window codes [n, h, w, 64], the folded scalars and the partial rows
    n, h, w, k = 2, 10, 17, 19
    tiles = -(-h // 8) * -(-w // 8)
    r = lambda b: -(-b // 256) * 256
    want = (L.ssal_train_tail2_grad_workspace_bytes(n, 2 * h, 2 * w, k) + 2 * r(n * 4 * h * w * 64 * 4) + r(n * h * w * 64 * 4)
            + r(n * h * w * 64) + r(4 * (336 + 6144)) + r(4 * tiles * TD_TRAINED))
    got = L.ssal_train_decoder_grad_workspace_bytes(n, h, w, k)
    assert abs(got - want) <= 4 * 256 and got >= want - 256, (got, want)  # (each piece starts at a multiple of 256 bytes)
    more = (L.ssal_train_tail2_grad_semi_workspace_bytes(n, 2 * h, 2 * w, k, 1)
            - L.ssal_train_tail2_grad_workspace_bytes(n, 2 * h, 2 * w, k))
    assert abs(L.ssal_train_decoder_grad_semi_workspace_bytes(n, h, w, k, 1) - got - more) <= 2 * 256
    p = ctypes.c_void_p(16)
    args = lambda n, h, w, k, params=p, mw=0, nbytes=1 << 20: (p, p, p, n, h, w, k, params, p, p, 0.0, 0.0, mw, p, p, p, nbytes,
                                                              None)
    assert L.ssal_train_decoder_grad_nhwc(*args(1, 4, 4, 1)) == _lib.SSAL_EINVAL
    assert L.ssal_train_decoder_grad_nhwc(*args(1, 4, 4, 33)) == _lib.SSAL_EINVAL
    assert L.ssal_train_decoder_grad_nhwc(*args(1, 1 << 29, 4, 19)) == _lib.SSAL_EINVAL
    assert L.ssal_train_decoder_grad_nhwc(*args(1, 4, 4, 19, params=None)) == _lib.SSAL_EINVAL
    assert L.ssal_train_decoder_grad_nhwc(*args(1, 4, 4, 19, mw=-1)) == _lib.SSAL_EINVAL
    assert L.ssal_train_decoder_grad_nhwc(*args(1, 4, 4, 19, nbytes=16)) == _lib.SSAL_ENOMEM  # judged before any launch
    # a workspace that holds the deep tail's call on a4_0 but not the decoder's: refused before any launch as well
    two = L.ssal_train_tail2_grad_workspace_bytes(1, 8, 8, 19)
    assert two < L.ssal_train_decoder_grad_workspace_bytes(1, 4, 4, 19)
    assert L.ssal_train_decoder_grad_nhwc(*args(1, 4, 4, 19, nbytes=two)) == _lib.SSAL_ENOMEM
    sargs = lambda measure, raw=(p, p, p): (p, p, p) + raw + (1, 4, 4, 19, p, p, p, p, measure, 0.0, 0.0, 0.0, 0, p, p, p, p, p,
                                                              16, None)
    assert L.ssal_train_decoder_grad_semi_nhwc(*sargs(7)) == _lib.SSAL_ENOTIMPL
    assert L.ssal_train_decoder_grad_semi_nhwc(*sargs(0, raw=(p, None, p))) == _lib.SSAL_EINVAL
    assert L.ssal_train_decoder_grad_semi_nhwc(*sargs(0, raw=(p, p, None))) == _lib.SSAL_EINVAL
    assert L.ssal_train_decoder_grad_semi_nhwc(*sargs(0)) == _lib.SSAL_ENOMEM
    assert L.ssal_enet_train_decoder_workspace_bytes(None, 1, 64, 64) == -1
    assert L.ssal_enet_train_decoder_semi_workspace_bytes(None, 1, 64, 64, 1) == -1
    assert L.ssal_enet_train_decoder_features_offset(None, 1, 64, 64) == -1


def test_workspace_size_limit_boundaries():
    """the limits are the two-block tail's on the quarter-resolution map [2h, 2w] and the fused 128-channel upsample kernel's
    (4 h w 64 <= 2^29, which the tail's limit implies): -1 exactly where the tail2 queries give -1 on [2h, 2w], a larger positive
    size elsewhere"""
    L = _lib.lib()
    ws, tail = L.ssal_train_decoder_grad_workspace_bytes, L.ssal_train_tail2_grad_workspace_bytes
    semi, tail_semi = L.ssal_train_decoder_grad_semi_workspace_bytes, L.ssal_train_tail2_grad_semi_workspace_bytes
    cases = [(1, 2048, 4095, 19), (1, 2048, 4096, 19), (1, 1, (1 << 24) - 1, 19), (1, 1, 1 << 24, 19), (1, (1 << 24) - 1, 1, 19),
             (1, 1 << 24, 1, 19), (1, 32, 32, 1), (1, 32, 32, 33), (1, 32, 32, 2), (1, 32, 32, 32), (0, 32, 32, 19),
             (1, 1 << 28, 1, 19), (1, 1024, 2048, 19), (1, 1024, 2049, 19), (1, 1, 1 << 22, 19), (1, (1 << 22) + 1, 1, 19)]
    for n, h, w, k in cases:
        assert (ws(n, h, w, k) == -1) == (tail(n, 2 * h, 2 * w, k) == -1), (n, h, w, k)
        for raw in (0, 1):
            assert (semi(n, h, w, k, raw) == -1) == (tail_semi(n, 2 * h, 2 * w, k, raw) == -1), (n, h, w, k, raw)
        assert ws(n, h, w, k) == -1 or ws(n, h, w, k) > tail(n, 2 * h, 2 * w, k) > 0
    assert ws(1, 1024, 2048, 19) > 0 and ws(1, 1024, 2049, 19) == -1
    assert ws(8, 128, 256, 19) >= tail(8, 256, 512, 19) + 2 * 8 * 256 * 512 * 64 * 4
    p = ctypes.c_void_p(16)
    for n, h, w, k in cases:  # the calls refuse at the same boundaries
        rc = L.ssal_train_decoder_grad_nhwc(p, p, p, n, h, w, k, p, p, p, 0.0, 0.0, 0, p, p, p, 16, None)
        assert rc == (_lib.SSAL_EINVAL if ws(n, h, w, k) == -1 else _lib.SSAL_ENOMEM), (n, h, w, k)
