"""Training of ICNet's last fusion stage without a GPU: the float64 oracle's gradients against central
differences, the refusals (judged before any device work), state and packing, the C ABI's symbols, statuses and sizes, the
size guard's boundaries, the handle-reuse predicate over variables that are not a tail of ``net.variables``."""
import ctypes

import numpy as np
import pytest

import semanticsegmentationactivelearning_amd as ssal
from semanticsegmentationactivelearning_amd import _lib, training

import icnet_fusion_train_oracle as ifo

AL_HYPER = {"learning_rate": 0.0005, "learning_rate_decay": 0.0,
            "optimizer": {"type": "Adam", "kwargs": {"beta1": 0.9, "beta2": 0.99}},
            "weight_reg": {"L2": 0.0002, "L1": 0.0, "glorot_scaling": False},
            "softmax": {"label_smoothing": 0.0, "loginverse_scaling": 1.02, "multiscale": False}}


def _icnet(k=19):
    net = ssal.ICNet(k)
    net.build((None, None, None, 3))
    return net


def _tiny_case(seed=0, k=3, n=1, h=2, w=3):
    rng = np.random.default_rng(seed)
    s24 = rng.standard_normal((n, h, w, 128))
    c3 = rng.standard_normal((n, 2 * h, 2 * w, 64))
    d = {n_: rng.uniform(-0.05, 0.05, s) for n_, s in zip(ifo.NAMES, ifo.shapes(k))}
    d["conv_sub2.gamma"] = rng.uniform(0.5, 1.5, 128)
    d["conv3_sub1_proj.gamma"] = rng.uniform(-1.5, 1.5, 128)
    d["conv6_cls.kernel"] = rng.uniform(-0.3, 0.3, (1, 1, 128, k))
    stats = np.concatenate([rng.uniform(-0.3, 0.3, 128), rng.uniform(0.5, 2.0, 128), rng.uniform(-0.3, 0.3, 128),
                            rng.uniform(0.5, 2.0, 128)])
    labels = rng.integers(0, k, (n, 16 * h, 16 * w)).astype(np.uint8)
    mask = (rng.uniform(size=labels.shape) > 0.2).astype(np.float32)
    return s24, c3, ifo.pack(d), stats, labels, mask


def test_oracle_gradients_match_finite_differences():
    """1 x 2 x 3, weight = 1.02, ls = 0.1: entries of all eight gradients against float64 central differences of the loss"""
    s24, c3, p, stats, labels, mask = _tiny_case()
    weight, ls = 1.02, 0.1
    _, g = ifo.loss_and_grad(s24, c3, p, stats, labels, mask, weight, ls)
    rng = np.random.default_rng(1)
    eps = 1e-6
    for name, (lo, hi) in ifo.offsets(3).items():
        idx = lo + rng.choice(hi - lo, min(6, hi - lo), replace=False)
        fd = np.zeros(idx.size)
        for j, i in enumerate(idx):
            pp, pm = p.copy(), p.copy()
            pp[i] += eps
            pm[i] -= eps
            fd[j] = (ifo.loss_and_grad(s24, c3, pp, stats, labels, mask, weight, ls)[0]
                     - ifo.loss_and_grad(s24, c3, pm, stats, labels, mask, weight, ls)[0]) / (2 * eps)
        err, scale = np.abs(g[idx] - fd).max(), np.abs(g[lo:hi]).max()
        print("%s: max |g - fd| = %.3e, max |g| = %.3e" % (name, err, scale))
        # central differences: O(eps^2) truncation + O(1e-16 / eps) cancellation (a ReLU kink within eps of a unit is not
        # drawn by this seed), both far below 1e-6 of the tensor's scale
        assert err <= 1e-6 * scale, name


def test_bound_contraction_dominates_the_gradient_and_dead_units_get_nothing():
    import torch
    s24, c3, p, stats, labels, mask = _tiny_case(seed=3, k=4)
    d = {n: v.copy() for n, v in ifo.unpack(p).items()}
    d["conv_sub2.beta"][:5] = -1e4          # with conv3_sub1_proj.beta: channels 0..4 of sub12_sum are 0 everywhere
    d["conv3_sub1_proj.beta"][:5] = -1e4
    d["conv_sub2.gamma"][7] = 0.0           # a zero scale: no kernel gradient through it, a gamma gradient all the same
    p = ifo.pack(d)
    x24, x3, W = ifo._tensors(s24, c3, p, grad=False)
    sub12, _, _ = ifo.fusion_forward(x24, x3, W, stats)
    assert not sub12[..., :5].any() and sub12[..., 5:].any()
    _, lg = ifo.iho.head_logits(sub12, W["conv6_cls.kernel"].reshape(128, 4), W["conv6_cls.bias"])
    g, c, _ = ifo.grad_and_bound(s24, c3, p, stats, labels, mask, 1.02, 0.1, sub12.numpy().astype(np.float32),
                                 lg.numpy().astype(np.float32))
    assert (np.abs(g) <= c * (1 + 1e-9) + 1e-300).all()
    gd = ifo.unpack(g)
    for name in ifo.NAMES[:6]:
        assert not gd[name][..., :5].any(), name           # relu'(0) = 0
    assert not gd["conv_sub2.kernel"][..., 7].any() and gd["conv_sub2.gamma"][7] != 0.0
    assert not gd["conv6_cls.kernel"][0, 0, :5].any()


def test_refusals_come_before_any_device_work(monkeypatch):
    def no_gpu():
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    enet = ssal.ENet(19)
    enet.build((None, None, None, 3))
    with pytest.raises(NotImplementedError):
        training.ICNetFusionTrainer(enet, 1e-3)
    net = _icnet()
    with pytest.raises(NotImplementedError):
        training.ICNetFusionTrainer.from_params(net, {"hyperparams": dict(AL_HYPER, softmax={"multiscale": True})})
    with pytest.raises(NotImplementedError):
        training.ICNetFusionTrainer.from_params(net, {"hyperparams": dict(AL_HYPER, weight_reg={"L2": 1e-4, "glorot_scaling": True})})
    tr = training.ICNetFusionTrainer.from_params(net, {"hyperparams": AL_HYPER})
    assert isinstance(tr, training.ICNetHeadTrainer) and tr._semi_keywords is False
    assert (tr.learning_rate, tr.beta1, tr.beta2, tr.l2, tr.weight) == (0.0005, 0.9, 0.99, 0.0002, 1.02)
    s24, c3 = np.zeros((1, 1, 2, 128), np.float32), np.zeros((1, 2, 4, 64), np.float32)
    lab, msk = np.zeros((1, 16, 32), np.uint8), np.ones((1, 16, 32), np.float32)
    img = np.zeros((1, 32, 32, 3), np.float32)
    ilab, imsk = np.zeros((1, 32, 32), np.uint8), np.ones((1, 32, 32), np.float32)
    for kw in ({"labelled": np.array([1])}, {"confusion": np.zeros((19, 19), np.int64)}, {"return_pseudo_pixels": True}):
        with pytest.raises(NotImplementedError):
            tr.gradient_features(s24, c3, lab, msk, **kw)
        with pytest.raises(NotImplementedError):
            tr.step_features(s24, c3, lab, msk, **kw)
        with pytest.raises(NotImplementedError):
            tr.step(img, ilab, imsk, **kw)
    for call in (lambda: tr.gradient_features(s24[..., :64], c3, lab, msk),             # channels
                 lambda: tr.gradient_features(s24, c3[..., :32], lab, msk),
                 lambda: tr.gradient_features(s24, c3[:, :1], lab, msk),                # conv3_sub1 is not twice sub24_sum
                 lambda: tr.gradient_features(s24, c3[:, :, :2], lab, msk),
                 lambda: tr.gradient_features(s24, np.zeros((1, 4, 4, 64), np.float32), lab, msk),
                 lambda: tr.gradient_features(s24, c3, lab[:, :8], msk),                # labels / mask are not 16x
                 lambda: tr.gradient_features(s24, c3, lab, msk[:, :, :16]),
                 lambda: tr.gradient_features(s24, c3, lab.astype(np.float32), msk),    # dtypes
                 lambda: tr.gradient_features(s24.astype(np.uint8), c3, lab, msk),
                 lambda: tr.gradient_features(s24, c3.astype(np.int32), lab, msk),
                 lambda: tr.gradient_features(s24, c3, lab, msk, max_workgroups=-1),
                 lambda: tr.step_features(s24, c3, lab, msk, max_workgroups=-2),
                 lambda: tr.step_features(s24, c3[:, :1], lab, msk),
                 lambda: tr.step(img, ilab[:, :16], imsk),
                 lambda: tr.step(img, ilab, imsk, max_workgroups=-1),
                 lambda: tr.gradient_features(s24, c3, lab, msk, params={"conv_sub2.mean": np.zeros(128)}),
                 lambda: tr.gradient_features(s24, c3, lab, msk, params={"conv_sub2.gamma": np.zeros(127)})):
        with pytest.raises(ValueError):
            call()
    # the existing trainers keep their refusals
    with pytest.raises(NotImplementedError):
        training.FinalLayerTrainer(net, 1e-3)
    with pytest.raises(ValueError):
        training.ICNetHeadTrainer(net, 1e-3).gradient_features(s24, lab, msk)


def test_variable_names_pack_unpack_and_adam_ranges():
    k = 6
    net = _icnet(k)
    tr = training.ICNetFusionTrainer(net, 1e-3)
    assert tr.variable_names == list(ifo.NAMES)
    want = [getattr(getattr(net, n.split(".")[0]), n.split(".")[1]) for n in ifo.NAMES]
    assert all(a is b for a, b in zip(tr._vars(), want))
    assert [tuple(v.shape) for v in want] == list(ifo.shapes(k))
    packed = tr._pack()
    assert packed.dtype == np.float32 and packed.size == ifo.floats(k) == 156160 + 129 * k
    assert np.array_equal(packed, ifo.pack({n: v.numpy() for n, v in zip(ifo.NAMES, want)}))
    un = tr._unpack(packed)
    assert list(un) == list(ifo.NAMES)
    for n, v in zip(ifo.NAMES, want):
        assert np.array_equal(un[n], v.numpy())
    over = tr._packed_with({"conv3_sub1_proj.beta": np.full(128, 3.0, np.float32)})
    lo, hi = ifo.offsets(k)["conv3_sub1_proj.beta"]
    assert (over[lo:hi] == 3.0).all() and np.array_equal(over[:lo], packed[:lo]) and np.array_equal(over[hi:], packed[hi:])
    # one Adam range per variable, the regulariser on the three kernels only
    off = ifo.offsets(k)
    assert tr._adam_ranges() == tuple(off[n] + (n in ifo.KERNELS,) for n in ifo.NAMES)


def test_state_round_trip_and_reinitialize():
    k = 6
    net = _icnet(k)
    tr = training.ICNetFusionTrainer(net, 1e-3, learning_rate_decay=0.5, decay_steps=10)
    block = {n: getattr(getattr(net, n.split(".")[0]), n.split(".")[1]).numpy().copy() for n in ifo.NAMES[:6]}
    before = net.conv6_cls.kernel.numpy().copy()
    net.conv6_cls.bias.assign(np.ones(k, np.float32))
    tr.reinitialize(seed=3)
    a = net.conv6_cls.kernel.numpy().copy()
    tr.reinitialize(seed=3)
    assert np.array_equal(a, net.conv6_cls.kernel.numpy()) and not np.array_equal(a, before)
    assert not net.conv6_cls.bias.numpy().any()
    for n, v in block.items():  # only conv6_cls is re-drawn
        assert np.array_equal(v, getattr(getattr(net, n.split(".")[0]), n.split(".")[1]).numpy()), n
    st = tr.state
    assert st["t"] == 0 and list(st["m"]) == list(ifo.NAMES) and list(st["v"]) == list(ifo.NAMES)
    for n, s in zip(ifo.NAMES, ifo.shapes(k)):
        assert st["m"][n].shape == s and not st["m"][n].any() and not st["v"][n].any()
    rng = np.random.default_rng(0)
    for key in ("m", "v"):
        for n in ifo.NAMES:
            st[key][n][...] = rng.standard_normal(st[key][n].shape)
    st["t"] = 5
    tr.load_state(st)
    got = tr.state
    assert got["t"] == 5
    for key in ("m", "v"):
        for n in ifo.NAMES:
            assert np.array_equal(got[key][n], st[key][n])
    assert tr.current_learning_rate() == np.float32(np.float32(1e-3) / np.float32(1 + np.float32(0.5) * np.float32(0.5)))
    tr.reinitialize(seed=1)  # all eight Adam slots are reset
    assert tr.state["t"] == 0 and not any(tr.state["m"][n].any() or tr.state["v"][n].any() for n in ifo.NAMES)
    with pytest.raises(ValueError):
        tr.load_state({"m": {n: st["m"][n] for n in ifo.NAMES[6:]}, "v": st["v"], "t": 0})
    with pytest.raises(ValueError):
        tr.load_state({"m": dict(st["m"], **{"conv_sub2.gamma": np.zeros(3)}), "v": st["v"], "t": 0})


def test_handle_reuse_predicate_compares_every_frozen_variable():
    """the trained variables are not a tail of ``net.variables``: conv1_sub1 .. conv3_sub1 sit between conv_sub2 and
    conv3_sub1_proj, and each layer's moving statistics follow its gamma / beta"""
    net = _icnet(4)
    tr = training.ICNetFusionTrainer(net, 1e-3)
    allv = net.variables
    trained = [i for i, v in enumerate(allv) if any(v is t for t in tr._vars())]
    assert len(trained) == 8 and trained != list(range(len(allv) - 8, len(allv)))
    between = [i for i, v in enumerate(allv) if v is net.conv3_sub1.kernel][0]
    assert trained[0] < between < trained[3]
    base = tuple(v.version for v in allv)
    ent = [object(), base]
    assert tr._handle_reusable(ent, base)
    assert not tr._handle_reusable(None, base) and not tr._handle_reusable([object(), None], base)
    for i in trained:  # a trained variable may have moved on
        moved = base[:i] + (base[i] + 1,) + base[i + 1:]
        assert tr._handle_reusable(ent, moved)
    frozen = [i for i in range(len(allv)) if i not in trained]
    stat = [i for i, v in enumerate(allv) if v is net.conv_sub2.variance][0]
    for i in (frozen[0], between, stat, frozen[-1]):  # a frozen one must not: below, between, a moving statistic, the last
        moved = base[:i] + (base[i] + 1,) + base[i + 1:]
        assert not tr._handle_reusable(ent, moved), allv[i].name
    assert len(tr._frozen_versions(base)) == len(allv) - 8


def test_abi_symbols_statuses_and_sizes():
    """fails on a library without the entries"""
    L = _lib.lib()
    i, i64, f, vp = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
    want = {
        "ssal_icnet_fusion_grad_workspace_bytes": (i64, [i, i, i, i]),
        "ssal_icnet_fusion_grad_nhwc": (i, [vp, vp, i, i, i, i, vp, vp, vp, f, f, vp, i, vp, vp, vp, i64, vp]),
        "ssal_icnet_train_fusion_workspace_bytes": (i64, [vp, i, i, i]),
        "ssal_icnet_train_fusion_nhwc": (i, [vp, vp, i, i, i, i, vp, vp, vp, f, f, vp, i, vp, vp, vp, i64, vp]),
        "ssal_icnet_update_fusion": (i, [vp, vp, vp]),
    }
    for name, proto in want.items():
        assert _lib.PROTOTYPES[name] == proto, name
        assert hasattr(L, name)
    ws = L.ssal_icnet_fusion_grad_workspace_bytes
    k = 19
    # three [n, 2h, 2w, 128] planes (projection, sub12_sum, g), lq, the tile windows, 96 split-K partials of 10 x 128 x 128
    # and their fold, the two re-laid-out kernels, the head kernel's 1024 partial rows
    n, h, w = 8, 64, 128
    floor = (3 * n * 2 * h * 2 * w * 128 + n * 4 * h * 4 * w * k + n * (h // 2) * (w // 2) * 36 * k + 97 * 163840
             + 147456 + 8192 + 1024 * 129 * k) * 4
    assert floor <= ws(n, h, w, k) <= floor + (1 << 16)
    assert ws(1, 1, 1, 2) > 0 and ws(1, 1, 1, 32) > 0
    assert ws(1, 8, 8, 1) == -1 and ws(1, 8, 8, 33) == -1 and ws(0, 8, 8, k) == -1 and ws(1, 0, 8, k) == -1
    p = ctypes.c_void_p(256)
    call = L.ssal_icnet_fusion_grad_nhwc
    big = 1 << 40
    assert call(p, p, 1, 1, 1, 33, p, p, p, 0.0, 0.0, p, 0, p, p, p, big, None) == _lib.SSAL_EINVAL
    assert call(p, p, 0, 1, 1, k, p, p, p, 0.0, 0.0, p, 0, p, p, p, big, None) == _lib.SSAL_EINVAL
    assert call(p, p, 1, 1, 1, k, p, p, p, 0.0, 0.0, p, -1, p, p, p, big, None) == _lib.SSAL_EINVAL
    assert call(p, None, 1, 1, 1, k, p, p, p, 0.0, 0.0, p, 0, p, p, p, big, None) == _lib.SSAL_EINVAL
    assert call(p, p, 1, 1, 1, k, p, p, p, 0.0, 0.0, None, 0, p, p, p, big, None) == _lib.SSAL_EINVAL
    assert call(p, p, 1, (1 << 26) + 1, 1, k, p, p, p, 0.0, 0.0, p, 0, p, p, p, big, None) == _lib.SSAL_EINVAL
    assert call(p, p, 1, 1, 1, k, p, p, p, 0.0, 0.0, p, 0, p, p, p, ws(1, 1, 1, k) - 512, None) == _lib.SSAL_ENOMEM
    # the images entry and the update need a committed handle
    hd = ctypes.c_void_p()
    _lib.check(L.ssal_icnet_create(3, k, ctypes.byref(hd)))
    assert L.ssal_icnet_train_fusion_workspace_bytes(hd, 1, 64, 64) == -1
    assert L.ssal_icnet_train_fusion_nhwc(hd, p, 0, 1, 64, 64, p, p, p, 0.0, 0.0, p, 0, p, p, p, big, None) == _lib.SSAL_ESTATE
    assert L.ssal_icnet_update_fusion(hd, p, None) == _lib.SSAL_ESTATE
    assert L.ssal_icnet_update_fusion(None, p, None) == _lib.SSAL_EINVAL
    _lib.check(L.ssal_icnet_destroy(hd))


def test_fusion_fits_boundaries():
    """``icnet_fusion_fits(h16, w16)`` through the workspace query: -1 exactly beyond 2 h16 = 2^27 (the head kernel's int
    coordinates) and beyond 2^31 - 1 of its 4 x 4 tiles of sub12_sum (= 2 x 2 pixels of sub24_sum), which outnumber the
    4 x 8 tiles of the weight-gradient kernel"""
    ws = _lib.lib().ssal_icnet_fusion_grad_workspace_bytes
    top = 1 << 26
    assert ws(1, top, 1, 2) > 0 and ws(1, top + 1, 1, 2) == -1
    assert ws(1, 1, top, 2) > 0 and ws(1, 1, top + 1, 2) == -1
    assert ws(1, top, 126, 2) > 0      # 2^25 x 63 tiles < 2^31
    assert ws(1, top, 127, 2) == -1    # 2^25 x 64 tiles = 2^31
    assert ws(1, 2 * 46340, 2 * 46340, 2) > 0 and ws(1, 2 * 46340 + 1, 2 * 46340 + 1, 2) == -1  # 46341^2 > 2^31 - 1


def test_adam_restatement_regularises_the_three_kernels_only():
    k = 3
    rng = np.random.default_rng(0)
    w = rng.standard_normal(ifo.floats(k)).astype(np.float32)
    z = np.zeros_like(w)
    _, m, _ = ifo.adam_fusion(w, z, z, z, k, 1e-3, 0.5, 0.5, 1e-8, 0.5, 0.5, l2=0.125)
    for name, (lo, hi) in ifo.offsets(k).items():
        if name in ifo.KERNELS:
            assert np.array_equal(m[lo:hi], np.float32(0.5) * (np.float32(0.125) * (np.float32(2.0) * w[lo:hi]))), name
        else:
            assert not m[lo:hi].any(), name
