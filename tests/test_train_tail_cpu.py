"""Decoder-tail training without a GPU: the float64 oracle's gradients against central finite
differences, the packed tail block and its offsets against the header, the names, the regularised set, the errors the trainer
must raise before any device work, the ABI symbols and the size limits of the workspace queries."""
import ctypes
import os
import re

import numpy as np
import pytest

import semanticsegmentationactivelearning_amd as ssal
from semanticsegmentationactivelearning_amd import _lib, training
from semanticsegmentationactivelearning_amd import synthetic as syn
from semanticsegmentationactivelearning_amd.training import DecoderTailTrainer, LastStageTrainer, SemiSupervisedTailTrainer

import decoder_tail_train_oracle as dto
import last_stage_train_oracle as lso

AL_PARAMS = {"hyperparams": {
    "dropout_rates": [0.01, 0.1, 0.1, 0.1, 0.1], "learning_rate": 0.0005, "learning_rate_decay": 0.0,
    "optimizer": {"type": "Adam", "kwargs": {"beta1": 0.9, "beta2": 0.99}},
    "weight_reg": {"L2": 0.0002, "L1": 0.0, "glorot_scaling": False},
    "softmax": {"label_smoothing": 0.0, "loginverse_scaling": 1.02, "multiscale": False}}}

# Bottleneck4_2's part of the packed block as include/ssal_enet.h ("Decoder-tail training") states it
HEADER_OFFSETS = {"proj_kernel": 0, "proj_gamma": 1024, "proj_beta": 1040, "proj_alpha": 1056, "conv_kernel": 1072,
                  "conv_gamma": 3376, "conv_beta": 3392, "conv_alpha": 3408, "exp_kernel": 3424, "exp_gamma": 4448,
                  "exp_beta": 4512, "residual_alpha": 4576, "proj_mean": 4640, "proj_variance": 4656, "conv_mean": 4672,
                  "conv_variance": 4688, "exp_mean": 4704, "exp_variance": 4768}


def _net(k=19):
    net = ssal.ENet(k)
    net.build((None, None, None, 3))
    return net


def test_oracle_gradients_match_finite_differences():
    """N = 1, a4_1 3 x 4, K = 3, weight 1.02, label smoothing 0.1: every entry of the gradients against central differences
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
    params, stats = dto.random_params(3, k)
    _, g, pre = dto.loss_and_grads(x, am, params, stats, labels, mask, weight, ls)
    assert np.abs(pre).min() > 1e-4
    assert pre.size == 12 * (16 + 16 + 64) + 12 * 16 + 48 * (8 + 16) + 48 * (4 + 4 + 16)  # nine PReLUs
    eps = 1e-6
    for name in dto.NAMES:
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
                vals.append(dto.loss_and_grads(x, am, p, stats, labels, mask, weight, ls)[0])
            fd[idx] = (vals[0] - vals[1]) / (2 * eps)
        sel = tuple(np.array(entries).T)
        err, scale = np.abs(g[name][sel] - fd[sel]).max(), max(np.abs(fd).max(), 1e-3)
        print("%-32s max |g - fd| %.3e, max |fd| %.3e" % (name, err, scale))
        assert err <= 1e-6 * scale, name


def test_names_layout_and_pack_round_trip():
    """a regular bottleneck has twelve trained variables (the list of DESIGN.md section 20: 4 640 floats), so the tail has
    26 + 12 names, the stage's 26 first; the offsets _pack / _unpack use are the header's"""
    net = _net(6)
    tr = DecoderTailTrainer(net, 1e-3, 0.9, 0.99)
    names = tr.variable_names
    assert names == list(dto.NAMES) and names[:26] == list(lso.NAMES) and len(names) == 26 + 12
    assert names[26:] == ["Bottleneck4_2." + a for a in dto.TAIL_VARS]
    assert isinstance(tr, LastStageTrainer) and "DecoderTailTrainer" in training.__all__
    assert issubclass(SemiSupervisedTailTrainer, DecoderTailTrainer) and "SemiSupervisedTailTrainer" in training.__all__
    L = _lib.lib()
    t0 = L.ssal_train_stage_param_floats(6)
    assert tr._floats() == L.ssal_train_tail_param_floats(6) == t0 + 4840
    # the header's table, read from the file itself
    text = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "ssal_enet.h")).read()
    sec = text[text.index("Decoder-tail training"):]
    for a, off in HEADER_OFFSETS.items():
        assert re.search(r"\b%d  %s \[" % (off, a), sec), (a, off)
    for name, var, off, _ in tr._named()[26:]:
        assert off == t0 + HEADER_OFFSETS[name.split(".")[1]], name
    assert dict(training._REGULAR64.stats) == {a: o for a, o in HEADER_OFFSETS.items() if a.endswith(("mean", "variance"))}
    used = np.zeros(tr._floats(), np.int32)
    for name, var, off, _ in tr._named():
        used[off:off + int(np.prod(var.shape))] += 1
    assert used.max() == 1 and int(used[t0:].sum()) == 4640
    syn.randomize_enet(net, seed=3)
    packed = tr._pack()
    back = tr._unpack(packed)
    for name, var, off, _ in tr._named():
        assert np.array_equal(back[name], var.numpy()), name
    blk = net.Bottleneck4_2
    for a, off in HEADER_OFFSETS.items():
        v = getattr(blk, a).numpy().reshape(-1)
        assert np.array_equal(packed[t0 + off:t0 + off + v.size], v), a
    assert not packed[t0 + 4832:].any()
    # the stage part is LastStageTrainer's block, float for float
    assert np.array_equal(packed[:t0], LastStageTrainer(net, 1e-3)._pack())
    only = tr._pack(back)
    assert not only[t0 + 4640:].any() and np.array_equal(only[t0:t0 + 4640], packed[t0:t0 + 4640])
    st = tr.state
    assert set(st["m"]) == set(dto.NAMES) and st["m"]["Bottleneck4_2.conv_kernel"].shape == (3, 3, 16, 16)
    with pytest.raises(ValueError):
        tr.load_state({"m": {n: st["m"][n] for n in lso.NAMES}, "v": st["v"], "t": 0})  # the stage's 26 names are not enough


def test_regularised_set_and_adam_ranges():
    tr = DecoderTailTrainer(_net(19), 1e-3)
    reg = {n for n, _, _, r in tr._named() if r}
    assert reg == set(dto.REGULARISED) and len(reg) == 14 + 6
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
    assert len(LastStageTrainer(_net(19), 1e-3)._adam_ranges()) == 15 and len(tr._adam_ranges()) == 22
    # the trained variables are the last ones of the model, so the trunk handle's version check covers everything below
    net = tr.net
    tail = tr._trained_tail()
    assert {v.name for v in net.variables[-tail:]} >= {var.name for _, var, _, _ in tr._named()}
    assert all(v.name.split("/")[0] in ("Bottleneck4_2", "Bottleneck5_0", "Bottleneck5_1", "Final") for v in net.variables[-tail:])


def test_not_implemented_and_value_errors_before_any_device_work(monkeypatch):
    def no_gpu():
        raise AssertionError("device work before the host-side verdict")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    hp = AL_PARAMS["hyperparams"]
    for cls in (DecoderTailTrainer, SemiSupervisedTailTrainer):
        tr = cls.from_params(_net(), AL_PARAMS)
        assert (tr.learning_rate, tr.beta2, tr.l2, tr.weight) == (0.0005, 0.99, 0.0002, 1.02)
        with pytest.raises(NotImplementedError):
            cls.from_params(_net(), {"hyperparams": dict(hp, softmax=dict(hp["softmax"], multiscale=True))})
        with pytest.raises(NotImplementedError):
            cls.from_params(_net(), {"hyperparams": dict(hp, weight_reg=dict(hp["weight_reg"], glorot_scaling=True))})
        with pytest.raises(NotImplementedError):
            cls(ssal.ICNet(19), 1e-3)
        x = np.zeros((1, 4, 4, 64), np.float32)
        am = lso.random_argmax(np.random.default_rng(0), 1, 4, 4)
        lab, mk = np.zeros((1, 16, 16), np.uint8), np.ones((1, 16, 16), np.float32)
        # a block below Bottleneck4_2 is out of scope; Bottleneck4_2 itself is not; a name that is no variable is a mistake
        with pytest.raises(NotImplementedError):
            tr.gradient_features(x, am, lab, mk, params={"Bottleneck4_1.proj_kernel": np.zeros((1, 1, 64, 16), np.float32)})
        with pytest.raises(ValueError):
            tr.gradient_features(x, am, lab, mk, params={"Bottleneck4_2.proj_mean": np.zeros((16,), np.float32)})
        with pytest.raises(ValueError):
            tr.gradient_features(x, am, lab, mk, params={"Bottleneck4_2.proj_kernel": np.zeros((1, 1, 64, 8), np.float32)})
        with pytest.raises(ValueError):
            tr.gradient_features(x, am, lab, mk, max_workgroups=-1)
        with pytest.raises(ValueError):
            tr.gradient_features(x, am[:, :, :, :8], lab, mk)
        with pytest.raises(ValueError):
            tr.step_features(x, am + 32, lab, mk)
    plain = DecoderTailTrainer(_net(), 1e-3)
    for kw in ({"labelled": np.array([0])}, {"confusion": np.zeros((19, 19), np.int64)}, {"return_pseudo_pixels": True}):
        with pytest.raises(NotImplementedError):
            plain.gradient_features(x, am, lab, mk, **kw)
        with pytest.raises(NotImplementedError):
            plain.step_features(x, am, lab, mk, **kw)
        with pytest.raises(NotImplementedError):
            plain.step(np.zeros((1, 16, 16, 3), np.float32), lab, mk, **kw)
    semi = SemiSupervisedTailTrainer(_net(), 1e-3)
    with pytest.raises(ValueError):
        semi.gradient_features(x, am, lab, mk, labelled=np.array([0, 1]))
    with pytest.raises(NotImplementedError):
        semi.gradient_features(x, am, lab, mk, labelled=np.array([0]), measure="nope")
    big = ssal.ENet(33)
    big.build((None, None, None, 3))
    with pytest.raises(ValueError):
        DecoderTailTrainer(big, 1e-3)


def test_abi_symbols_statuses_and_sizes():
    """fails on a library without the decoder-tail entries"""
    L = _lib.lib()
    for sym in ("ssal_train_tail_param_floats", "ssal_train_tail_grad_workspace_bytes", "ssal_train_tail_grad_nhwc",
                "ssal_enet_train_tail_workspace_bytes", "ssal_enet_train_tail_nhwc", "ssal_enet_train_tail_features_offset",
                "ssal_train_tail_grad_semi_workspace_bytes", "ssal_train_tail_grad_semi_nhwc",
                "ssal_enet_train_tail_semi_workspace_bytes", "ssal_enet_train_tail_semi_nhwc"):
        assert hasattr(L, sym), sym
    for k in (2, 19, 32):
        assert L.ssal_train_tail_param_floats(k) == L.ssal_train_stage_param_floats(k) + 4840 == 3936 + 144 * k + 4840
    assert L.ssal_train_tail_param_floats(1) == -1 and L.ssal_train_tail_param_floats(33) == -1
    # the workspace: the stage's, a4_2 and dL/d a4_2 [n, h, w, 64], the folded scalars, one row of 4640 floats per workgroup
    n, h, w, k = 2, 20, 34, 19
    tiles = -(-h // 8) * -(-w // 8)
    r = lambda b: -(-b // 256) * 256
    want = (L.ssal_train_stage_grad_workspace_bytes(n, h, w, k) - 256) + 2 * r(n * h * w * 64 * 4) + r(4 * 288) \
        + r(4 * tiles * 4640) + 256
    got = L.ssal_train_tail_grad_workspace_bytes(n, h, w, k)
    assert abs(got - want) <= 5 * 256 and got >= want - 256, (got, want)  # (each piece starts at a multiple of 256 bytes)
    more = L.ssal_train_stage_grad_semi_workspace_bytes(n, h, w, k, 1) - L.ssal_train_stage_grad_workspace_bytes(n, h, w, k)
    assert abs(L.ssal_train_tail_grad_semi_workspace_bytes(n, h, w, k, 1) - got - more) <= 2 * 256
    p = ctypes.c_void_p(16)
    args = lambda n, h, w, k, params=p, mw=0, nbytes=1 << 20: (p, p, n, h, w, k, params, p, p, 0.0, 0.0, mw, p, p, p, nbytes, None)
    assert L.ssal_train_tail_grad_nhwc(*args(1, 8, 8, 1)) == _lib.SSAL_EINVAL
    assert L.ssal_train_tail_grad_nhwc(*args(1, 8, 8, 33)) == _lib.SSAL_EINVAL
    assert L.ssal_train_tail_grad_nhwc(*args(1, 1 << 29, 8, 19)) == _lib.SSAL_EINVAL
    assert L.ssal_train_tail_grad_nhwc(*args(1, 8, 8, 19, params=None)) == _lib.SSAL_EINVAL
    assert L.ssal_train_tail_grad_nhwc(*args(1, 8, 8, 19, mw=-1)) == _lib.SSAL_EINVAL
    assert L.ssal_train_tail_grad_nhwc(*args(1, 8, 8, 19, nbytes=16)) == _lib.SSAL_ENOMEM  # judged before any launch
    sargs = lambda measure, raw=(p, p): (p, p) + raw + (1, 8, 8, 19, p, p, p, p, measure, 0.0, 0.0, 0.0, 0, p, p, p, p, p, 16, None)
    assert L.ssal_train_tail_grad_semi_nhwc(*sargs(7)) == _lib.SSAL_ENOTIMPL
    assert L.ssal_train_tail_grad_semi_nhwc(*sargs(0, raw=(p, None))) == _lib.SSAL_EINVAL
    assert L.ssal_train_tail_grad_semi_nhwc(*sargs(0)) == _lib.SSAL_ENOMEM
    assert L.ssal_enet_train_tail_workspace_bytes(None, 1, 64, 64) == -1
    assert L.ssal_enet_train_tail_semi_workspace_bytes(None, 1, 64, 64, 1) == -1
    assert L.ssal_enet_train_tail_features_offset(None, 1, 64, 64) == -1


def test_workspace_size_limit_boundaries():
    """-1 wherever the stage's query gives -1 (the output-layer gradient on the [2h, 2w] map, 64 h w < 2^31, K in [2, 32]),
    and beyond the fused 64-channel bottleneck kernel the forward runs on (64 h w <= 2^29: the byte offsets of one image in
    32 bits); a positive size inside both"""
    L = _lib.lib()
    ws, stage = L.ssal_train_tail_grad_workspace_bytes, L.ssal_train_stage_grad_workspace_bytes
    semi, stage_semi = L.ssal_train_tail_grad_semi_workspace_bytes, L.ssal_train_stage_grad_semi_workspace_bytes
    fwd_fits = lambda h, w: 64 * h * w <= 2 ** 29
    cases = [(1, 4096, 8191, 19), (1, 4096, 8192, 19), (1, 1, (1 << 25) - 1, 19), (1, 1, 1 << 25, 19), (1, (1 << 25) - 1, 1, 19),
             (1, 1 << 25, 1, 19), (1, 64, 64, 1), (1, 64, 64, 33), (1, 64, 64, 2), (1, 64, 64, 32), (0, 64, 64, 19),
             (1, 1 << 29, 1, 19), (1, 2048, 4096, 19), (1, 2048, 4097, 19), (1, 1, 1 << 23, 19), (1, (1 << 23) + 1, 1, 19)]
    for n, h, w, k in cases:
        if stage(n, h, w, k) == -1:
            assert ws(n, h, w, k) == -1 and semi(n, h, w, k, 0) == -1 and semi(n, h, w, k, 1) == -1, (n, h, w, k)
        assert (ws(n, h, w, k) != -1) == (stage(n, h, w, k) != -1 and fwd_fits(h, w)), (n, h, w, k)
        assert (semi(n, h, w, k, 1) != -1) == (stage_semi(n, h, w, k, 1) != -1 and fwd_fits(h, w)), (n, h, w, k)
        assert ws(n, h, w, k) == -1 or ws(n, h, w, k) > 0
    assert ws(1, 2048, 4096, 19) > 0 and ws(1, 2048, 4097, 19) == -1
    assert ws(8, 256, 512, 19) >= stage(8, 256, 512, 19) + 2 * 8 * 256 * 512 * 64 * 4
