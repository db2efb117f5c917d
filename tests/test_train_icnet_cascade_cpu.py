"""Training of ICNet's whole cascade head without a GPU: the trainer and the C ABI's symbols, the packed
layout for K = 2, 19, 32, the refusals (judged before any device work), the size guard's boundaries, the float64 oracle's
gradients against central differences, and the 2x resize adjoint as an adjoint."""
import ctypes

import numpy as np
import pytest
import torch

import semanticsegmentationactivelearning_amd as ssal
from semanticsegmentationactivelearning_amd import _lib, training

import icnet_cascade_train_oracle as ico
import icnet_head_train_oracle as iho

AL_HYPER = {"learning_rate": 0.0005, "learning_rate_decay": 0.0,
            "optimizer": {"type": "Adam", "kwargs": {"beta1": 0.9, "beta2": 0.99}},
            "weight_reg": {"L2": 0.0002, "L1": 0.0, "glorot_scaling": False},
            "softmax": {"label_smoothing": 0.0, "loginverse_scaling": 1.02, "multiscale": False}}
ABI = ("ssal_icnet_cascade_grad_workspace_bytes", "ssal_icnet_cascade_grad_nhwc", "ssal_icnet_train_cascade_workspace_bytes",
       "ssal_icnet_train_cascade_nhwc", "ssal_icnet_update_cascade")


def _icnet(k=19):
    net = ssal.ICNet(k)
    net.build((None, None, None, 3))
    return net


def test_trainer_and_abi_symbols_exist():
    """fails on a library / package without the feature"""
    assert issubclass(training.ICNetCascadeTrainer, training.ICNetFusionTrainer)
    assert "ICNetCascadeTrainer" in training.__all__
    L = _lib.lib()
    i, i64, f, vp = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
    want = {ABI[0]: (i64, [i, i, i, i]),
            ABI[1]: (i, [vp, vp, vp, i, i, i, i, vp, vp, vp, f, f, vp, i, vp, vp, vp, i64, vp]),
            ABI[2]: (i64, [vp, i, i, i]),
            ABI[3]: (i, [vp, vp, i, i, i, i, vp, vp, vp, f, f, vp, i, vp, vp, vp, i64, vp]),
            ABI[4]: (i, [vp, vp, vp])}
    for name in ABI:
        assert _lib.PROTOTYPES[name] == want[name], name
        assert hasattr(L, name)


@pytest.mark.parametrize("k", [2, 19, 32])
def test_packed_offsets_names_and_float_count(k):
    net = _icnet(k)
    tr = training.ICNetCascadeTrainer(net, 1e-3)
    assert tr.variable_names == list(ico.NAMES) and tr.variable_names[6:] == training.ICNetFusionTrainer.variable_names
    want = [getattr(getattr(net, n.split(".")[0]), n.split(".")[1]) for n in ico.NAMES]
    assert all(a is b for a, b in zip(tr._vars(), want))
    assert [tuple(v.shape) for v in want] == list(ico.shapes(k))
    assert tr._floats() == ico.floats(k) == 328192 + 156160 + 129 * k
    off = ico.offsets(k)
    assert off["conv_sub4.kernel"] == (0, 294912) and off["conv3_1_sub2_proj.kernel"] == (295168, 327936)
    assert off["conv_sub2.kernel"][0] == 328192 and off["conv6_cls.bias"] == (ico.floats(k) - k, ico.floats(k))
    assert tr._offsets() == [off[n] for n in ico.NAMES]
    packed = tr._pack()
    assert packed.dtype == np.float32 and np.array_equal(packed, ico.pack({n: v.numpy() for n, v in zip(ico.NAMES, want)}))
    assert all(np.array_equal(tr._unpack(packed)[n], v.numpy()) for n, v in zip(ico.NAMES, want))
    # one Adam range per variable, the regulariser on the five kernels only
    assert tr._adam_ranges() == tuple(off[n] + (n in ico.KERNELS,) for n in ico.NAMES)
    assert len(ico.KERNELS) == 5
    # the frozen statistics: the new block's four rows first
    assert [l for l, _ in tr._STATS] == ["conv_sub4"] * 2 + ["conv3_1_sub2_proj"] * 2 + ["conv_sub2"] * 2 + ["conv3_sub1_proj"] * 2


def test_state_reinitialize_and_handle_reuse():
    k = 5
    net = _icnet(k)
    tr = training.ICNetCascadeTrainer(net, 1e-3)
    block = {n: getattr(getattr(net, n.split(".")[0]), n.split(".")[1]).numpy().copy() for n in ico.NAMES[:12]}
    before = net.conv6_cls.kernel.numpy().copy()
    tr.reinitialize(seed=3)
    assert not np.array_equal(before, net.conv6_cls.kernel.numpy())
    for n, v in block.items():  # only conv6_cls is re-drawn
        assert np.array_equal(v, getattr(getattr(net, n.split(".")[0]), n.split(".")[1]).numpy()), n
    st = tr.state
    assert st["t"] == 0 and list(st["m"]) == list(ico.NAMES) and list(st["v"]) == list(ico.NAMES)
    st["m"]["conv_sub4.gamma"][...] = 2.0
    st["t"] = 4
    tr.load_state(st)
    assert tr.state["t"] == 4 and (tr.state["m"]["conv_sub4.gamma"] == 2.0).all()
    tr.reinitialize(seed=1)  # all fourteen Adam slots are reset
    assert tr.state["t"] == 0 and not any(tr.state["m"][n].any() or tr.state["v"][n].any() for n in ico.NAMES)
    with pytest.raises(ValueError):
        tr.load_state({"m": {n: st["m"][n] for n in ico.NAMES[6:]}, "v": st["v"], "t": 0})
    # the handle-reuse predicate compares every untrained variable
    allv = net.variables
    trained = [i for i, v in enumerate(allv) if any(v is t for t in tr._vars())]
    assert len(trained) == 14
    base = tuple(v.version for v in allv)
    ent = [object(), base]
    for i in trained:
        assert tr._handle_reusable(ent, base[:i] + (base[i] + 1,) + base[i + 1:])
    stat = [i for i, v in enumerate(allv) if v is net.conv_sub4.variance][0]
    for i in [j for j in range(len(allv)) if j not in trained][::7] + [stat]:
        assert not tr._handle_reusable(ent, base[:i] + (base[i] + 1,) + base[i + 1:]), allv[i].name


def test_refusals_come_before_any_device_work(monkeypatch):
    def no_gpu():
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    enet = ssal.ENet(19)
    enet.build((None, None, None, 3))
    with pytest.raises(NotImplementedError):
        training.ICNetCascadeTrainer(enet, 1e-3)
    net = _icnet()
    with pytest.raises(NotImplementedError):
        training.ICNetCascadeTrainer.from_params(net, {"hyperparams": dict(AL_HYPER, softmax={"multiscale": True})})
    with pytest.raises(NotImplementedError):
        training.ICNetCascadeTrainer.from_params(net, {"hyperparams": dict(AL_HYPER, weight_reg={"L2": 1e-4, "glorot_scaling": True})})
    tr = training.ICNetCascadeTrainer.from_params(net, {"hyperparams": AL_HYPER})
    assert tr._semi_keywords is False
    assert (tr.learning_rate, tr.beta1, tr.beta2, tr.l2, tr.weight) == (0.0005, 0.9, 0.99, 0.0002, 1.02)
    c54, c31 = np.zeros((1, 1, 2, 256), np.float32), np.zeros((1, 2, 4, 256), np.float32)
    c3 = np.zeros((1, 4, 8, 64), np.float32)
    lab, msk = np.zeros((1, 32, 64), np.uint8), np.ones((1, 32, 64), np.float32)
    img = np.zeros((1, 32, 32, 3), np.float32)
    ilab, imsk = np.zeros((1, 32, 32), np.uint8), np.ones((1, 32, 32), np.float32)
    for kw in ({"labelled": np.array([1])}, {"confusion": np.zeros((19, 19), np.int64)}, {"return_pseudo_pixels": True}):
        with pytest.raises(NotImplementedError):
            tr.gradient_features(c54, c31, c3, lab, msk, **kw)
        with pytest.raises(NotImplementedError):
            tr.step_features(c54, c31, c3, lab, msk, **kw)
        with pytest.raises(NotImplementedError):
            tr.step(img, ilab, imsk, **kw)
    for call in (lambda: tr.gradient_features(c54[..., :128], c31, c3, lab, msk),            # channels
                 lambda: tr.gradient_features(c54, c31[..., :128], c3, lab, msk),
                 lambda: tr.gradient_features(c54, c31, c3[..., :32], lab, msk),
                 lambda: tr.gradient_features(c54, c31[:, :1], c3, lab, msk),                # conv3_1 is not 2x conv5_4_k1
                 lambda: tr.gradient_features(c54, c31[:, :, :2], c3, lab, msk),
                 lambda: tr.gradient_features(c54, c31, c3[:, :2], lab, msk),                # conv3_sub1 is not 4x
                 lambda: tr.gradient_features(c54, c31, np.zeros((1, 2, 4, 64), np.float32), lab, msk),
                 lambda: tr.gradient_features(c54, c31, c3, lab[:, :16], msk),               # labels / mask are not 32x (16x)
                 lambda: tr.gradient_features(c54, c31, c3, lab, msk[:, :, :32]),
                 lambda: tr.gradient_features(c54, c31, c3, lab.astype(np.float32), msk),    # dtypes
                 lambda: tr.gradient_features(c54.astype(np.uint8), c31, c3, lab, msk),
                 lambda: tr.gradient_features(c54, c31.astype(np.int32), c3, lab, msk),
                 lambda: tr.gradient_features(c54, c31, c3.astype(np.int32), lab, msk),
                 lambda: tr.gradient_features(c54, c31, c3, lab, msk, max_workgroups=-1),
                 lambda: tr.step_features(c54, c31, c3, lab, msk, max_workgroups=-2),
                 lambda: tr.step_features(c54, c31[:, :1], c3, lab, msk),
                 lambda: tr.step(img, ilab[:, :16], imsk),
                 lambda: tr.step(img, ilab, imsk, max_workgroups=-1),
                 lambda: tr.gradient_features(c54, c31, c3, lab, msk, params={"conv_sub4.mean": np.zeros(128)}),
                 lambda: tr.gradient_features(c54, c31, c3, lab, msk, params={"conv_sub4.gamma": np.zeros(127)})):
        with pytest.raises(ValueError):
            call()
    # the existing trainers keep their refusals
    with pytest.raises(NotImplementedError):
        training.ICNetFusionTrainer(enet, 1e-3)
    with pytest.raises(ValueError):
        training.ICNetFusionTrainer(net, 1e-3).gradient_features(c54, c3, lab, msk)


def test_abi_statuses_sizes_and_both_size_guard_boundaries():
    L = _lib.lib()
    ws = L.ssal_icnet_cascade_grad_workspace_bytes
    k = 19
    # at 1/16 resolution: projection, sub24_sum, g24 and the four-fold du; 64 split-K partials of 11 x 256 x 128 and their fold;
    # the two re-laid-out kernels; then everything the fusion entry takes at (2h, 2w)
    n, h, w = 8, 32, 64
    own = (7 * n * 2 * h * 2 * w * 128 + 65 * 360448 + 294912 + 32768) * 4
    fusion = L.ssal_icnet_fusion_grad_workspace_bytes(n, 2 * h, 2 * w, k)
    assert own + fusion - 256 <= ws(n, h, w, k) <= own + fusion + (1 << 16)
    assert ws(1, 1, 1, 2) > 0 and ws(1, 1, 1, 32) > 0
    assert ws(1, 8, 8, 1) == -1 and ws(1, 8, 8, 33) == -1 and ws(0, 8, 8, k) == -1 and ws(1, 0, 8, k) == -1
    # icnet_cascade_fits(h32, w32): -1 exactly beyond 2 h32 = 2^26 (icnet_fusion_fits' coordinate limit) ...
    top = 1 << 25
    assert ws(1, top, 1, 2) > 0 and ws(1, top + 1, 1, 2) == -1
    assert ws(1, 1, top, 2) > 0 and ws(1, 1, top + 1, 2) == -1
    # ... and beyond 2^31 - 1 tiles of the head kernel (one per pixel of conv5_4_k1)
    assert ws(1, top, 63, 2) > 0 and ws(1, top, 64, 2) == -1
    assert ws(1, 46340, 46340, 2) > 0 and ws(1, 46341, 46341, 2) == -1
    p = ctypes.c_void_p(256)
    call = L.ssal_icnet_cascade_grad_nhwc
    big = 1 << 40
    assert call(p, p, p, 1, 1, 1, 33, p, p, p, 0.0, 0.0, p, 0, p, p, p, big, None) == _lib.SSAL_EINVAL
    assert call(p, p, p, 0, 1, 1, k, p, p, p, 0.0, 0.0, p, 0, p, p, p, big, None) == _lib.SSAL_EINVAL
    assert call(p, p, p, 1, 1, 1, k, p, p, p, 0.0, 0.0, p, -1, p, p, p, big, None) == _lib.SSAL_EINVAL
    assert call(p, None, p, 1, 1, 1, k, p, p, p, 0.0, 0.0, p, 0, p, p, p, big, None) == _lib.SSAL_EINVAL
    assert call(p, p, p, 1, 1, 1, k, p, p, p, 0.0, 0.0, None, 0, p, p, p, big, None) == _lib.SSAL_EINVAL
    assert call(p, p, p, 1, top + 1, 1, k, p, p, p, 0.0, 0.0, p, 0, p, p, p, big, None) == _lib.SSAL_EINVAL
    assert call(p, p, p, 1, 1, 1, k, p, p, p, 0.0, 0.0, p, 0, p, p, p, ws(1, 1, 1, k) - 512, None) == _lib.SSAL_ENOMEM
    # the images entry and the update need a committed handle
    hd = ctypes.c_void_p()
    _lib.check(L.ssal_icnet_create(3, k, ctypes.byref(hd)))
    assert L.ssal_icnet_train_cascade_workspace_bytes(hd, 1, 64, 64) == -1
    assert L.ssal_icnet_train_cascade_nhwc(hd, p, 0, 1, 64, 64, p, p, p, 0.0, 0.0, p, 0, p, p, p, big, None) == _lib.SSAL_ESTATE
    assert L.ssal_icnet_update_cascade(hd, p, None) == _lib.SSAL_ESTATE
    assert L.ssal_icnet_update_cascade(None, p, None) == _lib.SSAL_EINVAL
    assert L.ssal_icnet_update_fusion(hd, p, None) == _lib.SSAL_ESTATE
    _lib.check(L.ssal_icnet_destroy(hd))


def _tiny_case(seed=0, k=3, n=1, h=1, w=1):
    rng = np.random.default_rng(seed)
    c54 = rng.standard_normal((n, h, w, 256))
    c31 = rng.standard_normal((n, 2 * h, 2 * w, 256))
    c3 = rng.standard_normal((n, 4 * h, 4 * w, 64))
    d = {n_: rng.uniform(-0.05, 0.05, s) for n_, s in zip(ico.NAMES, ico.shapes(k))}
    for name in ("conv_sub4.gamma", "conv_sub2.gamma"):
        d[name] = rng.uniform(0.5, 1.5, 128)
    for name in ("conv3_1_sub2_proj.gamma", "conv3_sub1_proj.gamma"):
        d[name] = rng.uniform(-1.5, 1.5, 128)
    d["conv6_cls.kernel"] = rng.uniform(-0.3, 0.3, (1, 1, 128, k))
    stats = np.concatenate([rng.uniform(-0.3, 0.3, 128) if i % 2 == 0 else rng.uniform(0.5, 2.0, 128) for i in range(8)])
    labels = rng.integers(0, k, (n, 32 * h, 32 * w)).astype(np.uint8)
    mask = (rng.uniform(size=labels.shape) > 0.2).astype(np.float32)
    return c54, c31, c3, ico.pack(d), stats, labels, mask


def test_oracle_gradients_match_finite_differences():
    """1 x 1 x 1, weight = 1.02, ls = 0.1: entries of all fourteen gradients against float64 central differences of the loss"""
    c54, c31, c3, p, stats, labels, mask = _tiny_case()
    weight, ls = 1.02, 0.1
    _, g = ico.loss_and_grad(c54, c31, c3, p, stats, labels, mask, weight, ls)
    rng = np.random.default_rng(1)
    eps = 1e-6
    for name, (lo, hi) in ico.offsets(3).items():
        idx = lo + rng.choice(hi - lo, min(4, hi - lo), replace=False)
        if name == "conv_sub4.kernel":  # at h16 = 2 every off-centre tap is padding: probe the centre tap
            idx = lo + 4 * 256 * 128 + rng.choice(256 * 128, 4, replace=False)
        fd = np.zeros(idx.size)
        for j, i in enumerate(idx):
            pp, pm = p.copy(), p.copy()
            pp[i] += eps
            pm[i] -= eps
            fd[j] = (ico.loss_and_grad(c54, c31, c3, pp, stats, labels, mask, weight, ls)[0]
                     - ico.loss_and_grad(c54, c31, c3, pm, stats, labels, mask, weight, ls)[0]) / (2 * eps)
        err, scale = np.abs(g[idx] - fd).max(), np.abs(g[lo:hi]).max()
        print("%s: max |g - fd| = %.3e, max |g| = %.3e" % (name, err, scale))
        # central differences: O(eps^2) truncation + O(1e-16 / eps) cancellation (a ReLU kink within eps of a unit is not
        # drawn by this seed), both far below 1e-6 of the tensor's scale
        assert err <= 1e-6 * scale, name
    gd = ico.unpack(g)
    assert not gd["conv_sub4.kernel"][[0, 0, 0, 1, 1, 2, 2, 2], [0, 1, 2, 0, 2, 0, 1, 2]].any()  # padding taps get nothing


def test_bound_contraction_dominates_the_gradient():
    c54, c31, c3, p, stats, labels, mask = _tiny_case(seed=3, k=4)
    s24, s12, lg = ico.cascade_forward(c54, c31, c3, p, stats)
    f32 = lambda a: a.astype(np.float32)
    g, c, _ = ico.grad_and_bound(c54, c31, c3, p, stats, labels, mask, 1.02, 0.1, f32(s24), f32(s12), f32(lg))
    assert (np.abs(g) <= c * (1 + 1e-9) + 1e-300).all()
    for name in ico.NAMES:
        assert ico.kappa(name, 1, 1, 1, 4, 1.02) > 0


@pytest.mark.parametrize("h,w", [(1, 1), (2, 3), (3, 5)])
def test_resize_adjoint_is_the_adjoint(h, w):
    """<resize_2x(x), y> = <x, adjoint(y)> in float64"""
    rng = np.random.default_rng(10 * h + w)
    x, y = rng.standard_normal((2, h, w, 3)), rng.standard_normal((2, 2 * h, 2 * w, 3))
    lhs = float((iho.resize_legacy(torch.as_tensor(x), 2).numpy() * y).sum())
    rhs = float((x * ico.adjoint_2x(y)).sum())
    assert abs(lhs - rhs) <= 1e-12 * (np.abs(x).sum() + np.abs(y).sum())
    # the last row and column collect their clamped tap twice
    e = np.zeros((1, 2 * h, 2 * w, 1))
    e[0, -1, -1, 0] = 1.0
    assert ico.adjoint_2x(e)[0, -1, -1, 0] == 1.0
