"""Training of ICNet's output layer without a GPU: the float64 oracle's gradients against central
differences, the refusals (judged before any device work), the C ABI's symbols, statuses and sizes, the size guard's
boundaries, and Adam's float32 restatement on the packed [128 K | K] head."""
import ctypes

import numpy as np
import pytest

import semanticsegmentationactivelearning_amd as ssal
from semanticsegmentationactivelearning_amd import _lib, training
from semanticsegmentationactivelearning_amd.training import FinalLayerTrainer

import icnet_head_train_oracle as iho

AL_HYPER = {"dropout_rates": [0.01, 0.1, 0.1, 0.1, 0.1], "learning_rate": 0.0005, "learning_rate_decay": 0.0,
            "optimizer": {"type": "Adam", "kwargs": {"beta1": 0.9, "beta2": 0.99}},
            "weight_reg": {"L2": 0.0002, "L1": 0.0, "glorot_scaling": False},
            "softmax": {"label_smoothing": 0.0, "loginverse_scaling": 1.02, "multiscale": False}}


def _icnet(k=19):
    net = ssal.ICNet(k)
    net.build((None, None, None, 3))
    return net


def _tiny_case(seed=0, k=3, n=2, h=1, w=2):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, h, w, 128)).astype(np.float32)
    head = np.concatenate([rng.uniform(-0.2, 0.2, 128 * k), rng.uniform(-0.5, 0.5, k)]).astype(np.float32)
    labels = rng.integers(0, k, (n, 8 * h, 8 * w)).astype(np.uint8)
    mask = (rng.uniform(size=labels.shape) > 0.2).astype(np.float32)
    labels[0, 0, :3] = 255
    mask[0, 0, :3] = 0.0
    return x, head, labels, mask


def test_resize_restatement_is_the_legacy_mapping():
    """4x of a 2 x 2 map: src = dst / 4, the +1 tap clamped (rows / columns 4..7 repeat the last entry)"""
    import torch
    x = torch.tensor([[[[0.0], [4.0]], [[8.0], [12.0]]]], dtype=torch.float64)
    y = iho.resize_legacy(x, 4)[0, :, :, 0].numpy()
    assert y.shape == (8, 8)
    assert y[0, :5].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0] and (y[0, 4:] == 4.0).all()
    assert y[:5, 0].tolist() == [0.0, 2.0, 4.0, 6.0, 8.0] and (y[4:, 0] == 8.0).all()
    assert y[1, 1] == 3.0 and y[7, 7] == 12.0


def test_oracle_gradient_matches_finite_differences():
    """weight = 1.02, ls = 0.1: kernel and bias gradients against float64 central differences of the loss"""
    x, head, labels, mask = _tiny_case()
    weight, ls = 1.02, 0.1
    _, g = iho.loss_and_grad(x, head, labels, mask, weight, ls)
    hd = head.astype(np.float64)
    eps = 1e-6
    rng = np.random.default_rng(1)
    idx = np.concatenate([rng.choice(128 * 3, 40, replace=False), np.arange(128 * 3, 129 * 3)])  # 40 kernel entries, the bias
    fd = np.zeros(idx.size)
    for j, i in enumerate(idx):
        hp, hm = hd.copy(), hd.copy()
        hp[i] += eps
        hm[i] -= eps
        fd[j] = (iho.loss_and_grad(x, hp, labels, mask, weight, ls)[0]
                 - iho.loss_and_grad(x, hm, labels, mask, weight, ls)[0]) / (2 * eps)
    err, scale = np.abs(g[idx] - fd).max(), np.abs(fd).max()
    print("max |g - fd| = %.3e, max |fd| = %.3e" % (err, scale))
    # central differences: O(eps^2) truncation + O(1e-16 / eps) cancellation, both far below 1e-7 of the scale
    assert err <= 1e-7 * scale


def test_bound_contraction_dominates_the_gradient():
    """C is the same contraction over absolute values: |g64| <= C entry by entry"""
    import torch
    x, head, labels, mask = _tiny_case(seed=3, k=4)
    k = 4
    kern, bias = iho.split(head.astype(np.float64), k)
    _, lg = iho.head_logits(torch.as_tensor(x.astype(np.float64)), torch.as_tensor(kern), torch.as_tensor(bias))
    logits32 = lg.numpy().astype(np.float32)
    g, c, _ = iho.grad_and_bound(x, head, labels, mask, 1.02, 0.1, logits32)
    assert (np.abs(g) <= c * (1 + 1e-12)).all() and (c > 0).all()


def test_refusals_come_before_any_device_work(monkeypatch):
    def no_gpu():
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    enet = ssal.ENet(19)
    enet.build((None, None, None, 3))
    with pytest.raises(NotImplementedError):
        training.ICNetHeadTrainer(enet, 1e-3)
    net = _icnet()
    with pytest.raises(NotImplementedError):
        training.ICNetHeadTrainer.from_params(net, {"hyperparams": dict(AL_HYPER, softmax={"multiscale": True})})
    with pytest.raises(NotImplementedError):
        training.ICNetHeadTrainer.from_params(net, {"hyperparams": dict(AL_HYPER, weight_reg={"L2": 1e-4, "glorot_scaling": True})})
    tr = training.ICNetHeadTrainer.from_params(net, {"hyperparams": AL_HYPER})
    assert (tr.learning_rate, tr.beta1, tr.beta2, tr.l2, tr.weight) == (0.0005, 0.9, 0.99, 0.0002, 1.02)
    x = np.zeros((1, 1, 2, 128), np.float32)
    lab, msk = np.zeros((1, 8, 16), np.uint8), np.ones((1, 8, 16), np.float32)
    img = np.zeros((1, 32, 32, 3), np.float32)
    ilab, imsk = np.zeros((1, 32, 32), np.uint8), np.ones((1, 32, 32), np.float32)
    for kw in ({"labelled": np.array([1])}, {"confusion": np.zeros((19, 19), np.int64)}, {"return_pseudo_pixels": True}):
        with pytest.raises(NotImplementedError):
            tr.gradient_features(x, lab, msk, **kw)
        with pytest.raises(NotImplementedError):
            tr.step_features(x, lab, msk, **kw)
        with pytest.raises(NotImplementedError):
            tr.step(img, ilab, imsk, **kw)
    # ValueError: shapes, dtypes, max_workgroups
    for call in (lambda: tr.gradient_features(x[..., :64], lab, msk),            # channels
                 lambda: tr.gradient_features(x, lab[:, :4], msk),               # label shape
                 lambda: tr.gradient_features(x, lab, msk[:, :, :8]),            # mask shape
                 lambda: tr.gradient_features(x, lab.astype(np.float32), msk),   # label dtype
                 lambda: tr.gradient_features(x.astype(np.uint8), lab, msk),     # feature dtype
                 lambda: tr.gradient_features(x, lab, msk, max_workgroups=-1),
                 lambda: tr.step_features(x, lab, msk, max_workgroups=-2),
                 lambda: tr.step(img, ilab[:, :16], imsk),
                 lambda: tr.step(img, ilab, imsk, max_workgroups=-1),
                 lambda: tr.gradient_features(x, lab, msk, params={"conv6_cls.gamma": np.zeros(19)}),
                 lambda: tr.gradient_features(x, lab, msk, params={"conv6_cls.bias": np.zeros(18)})):
        with pytest.raises(ValueError):
            call()
    # the existing trainers still refuse an ICNet
    with pytest.raises(NotImplementedError):
        FinalLayerTrainer(net, 1e-3)


def test_state_reinitialize_and_learning_rate():
    net = _icnet(6)
    tr = training.ICNetHeadTrainer(net, 1e-3, learning_rate_decay=0.5, decay_steps=10)
    before = net.conv6_cls.kernel.numpy().copy()
    net.conv6_cls.bias.assign(np.ones(6, np.float32))
    tr.reinitialize(seed=3)
    a = net.conv6_cls.kernel.numpy().copy()
    tr.reinitialize(seed=3)
    assert np.array_equal(a, net.conv6_cls.kernel.numpy()) and not np.array_equal(a, before)
    assert np.abs(a).max() <= np.sqrt(6.0 / (128 + 6))  # glorot: fan_in 128, fan_out K
    assert not net.conv6_cls.bias.numpy().any()
    st = tr.state
    assert st["t"] == 0 and set(st["m"]) == {"conv6_cls.kernel", "conv6_cls.bias"}
    assert st["m"]["conv6_cls.kernel"].shape == (1, 1, 128, 6) and st["v"]["conv6_cls.bias"].shape == (6,)
    st["m"]["conv6_cls.bias"][:] = 2.0
    st["t"] = 5
    tr.load_state(st)
    assert tr.state["t"] == 5 and (tr.state["m"]["conv6_cls.bias"] == 2.0).all()
    assert tr.current_learning_rate() == np.float32(np.float32(1e-3) / np.float32(1 + np.float32(0.5) * np.float32(0.5)))
    with pytest.raises(ValueError):
        tr.load_state({"m": {"conv6_cls.kernel": a}, "v": st["v"], "t": 0})
    assert tr._adam_ranges() == ((0, 768, True), (768, 774, False))  # the regulariser goes to the kernel only


def test_abi_symbols_statuses_and_sizes():
    """fails on a library without the entries"""
    L = _lib.lib()
    i, i64, f, vp = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
    want = {
        "ssal_icnet_head_grad_workspace_bytes": (i64, [i, i, i, i]),
        "ssal_icnet_head_grad_nhwc": (i, [vp, i, i, i, i, vp, vp, vp, f, f, i, vp, vp, vp, i64, vp]),
        "ssal_icnet_train_head_workspace_bytes": (i64, [vp, i, i, i]),
        "ssal_icnet_train_head_nhwc": (i, [vp, vp, i, i, i, i, vp, vp, vp, f, f, i, vp, vp, vp, i64, vp]),
        "ssal_icnet_update_head": (i, [vp, vp, vp, vp]),
    }
    for name, proto in want.items():
        assert _lib.PROTOTYPES[name] == proto, name
        assert hasattr(L, name)
    ws = L.ssal_icnet_head_grad_workspace_bytes
    k = 19
    # lq [n, 2h, 2w, K] + the re-laid-out kernel + 1024 partial rows of 129 K floats + their float64 pairs
    floor = 8 * 256 * 512 * k * 4 + (4096 + 64) * 4 + 1024 * 129 * k * 4 + 1024 * 16
    assert floor <= ws(8, 128, 256, k) <= floor + 4096
    assert ws(1, 1, 1, 2) > 0 and ws(1, 1, 1, 32) > 0
    assert ws(1, 8, 8, 1) == -1 and ws(1, 8, 8, 33) == -1 and ws(0, 8, 8, k) == -1 and ws(1, 0, 8, k) == -1
    p = ctypes.c_void_p(256)
    call = L.ssal_icnet_head_grad_nhwc
    assert call(p, 1, 1, 1, 33, p, p, p, 0.0, 0.0, 0, p, p, p, 1 << 30, None) == _lib.SSAL_EINVAL
    assert call(p, 0, 1, 1, k, p, p, p, 0.0, 0.0, 0, p, p, p, 1 << 30, None) == _lib.SSAL_EINVAL
    assert call(p, 1, 1, 1, k, p, p, p, 0.0, 0.0, -1, p, p, p, 1 << 30, None) == _lib.SSAL_EINVAL
    assert call(p, 1, 1, 1, k, None, p, p, 0.0, 0.0, 0, p, p, p, 1 << 30, None) == _lib.SSAL_EINVAL
    assert call(p, 1, (1 << 27) + 1, 1, k, p, p, p, 0.0, 0.0, 0, p, p, p, 1 << 30, None) == _lib.SSAL_EINVAL
    assert call(p, 1, 1, 1, k, p, p, p, 0.0, 0.0, 0, p, p, p, ws(1, 1, 1, k) - 512, None) == _lib.SSAL_ENOMEM
    # the images entry and the head update need a committed handle
    h = ctypes.c_void_p()
    _lib.check(L.ssal_icnet_create(3, k, ctypes.byref(h)))
    assert L.ssal_icnet_train_head_workspace_bytes(h, 1, 64, 64) == -1
    assert L.ssal_icnet_train_head_nhwc(h, p, 0, 1, 64, 64, p, p, p, 0.0, 0.0, 0, p, p, p, 1 << 30, None) == _lib.SSAL_ESTATE
    assert L.ssal_icnet_update_head(h, p, p, None) == _lib.SSAL_ESTATE
    assert L.ssal_icnet_update_head(None, p, p, None) == _lib.SSAL_EINVAL
    _lib.check(L.ssal_icnet_destroy(h))


def test_head_grad_fits_boundaries():
    """the workspace query is -1 exactly beyond the kernel's int limits: 8h + 1 / 8w + 1 and the count of 8 x 8 tiles of lq
    (= 4 x 4 pixels of sub12_sum)"""
    ws = _lib.lib().ssal_icnet_head_grad_workspace_bytes
    top = 1 << 27
    assert ws(1, top, 1, 2) > 0 and ws(1, top + 1, 1, 2) == -1
    assert ws(1, 1, top, 2) > 0 and ws(1, 1, top + 1, 2) == -1
    assert ws(1, top, 252, 2) > 0      # 2^25 x 63 tiles < 2^31
    assert ws(1, top, 253, 2) == -1    # 2^25 x 64 tiles = 2^31
    assert ws(1, 4 * 46340, 4 * 46340, 2) > 0 and ws(1, 4 * 46340 + 1, 4 * 46340 + 1, 2) == -1  # 46341^2 > 2^31 - 1


def test_adam_restatement_on_the_packed_head():
    """l2 reaches the kernel's 128 K floats and not the bias' K; both follow ApplyAdam"""
    k = 3
    rng = np.random.default_rng(0)
    head = rng.standard_normal(129 * k).astype(np.float32)
    g = np.zeros(129 * k, np.float32)
    z = np.zeros(129 * k, np.float32)
    w, m, v = iho.adam_head(head, z, z, g, k, 1e-3, 0.5, 0.5, 1e-8, 0.5, 0.5, l2=0.125)
    assert np.array_equal(m[:128 * k], np.float32(0.5) * (np.float32(0.125) * (np.float32(2.0) * head[:128 * k])))
    assert not m[128 * k:].any() and np.array_equal(w[128 * k:], head[128 * k:])
    g = rng.standard_normal(129 * k).astype(np.float32)
    w2, m2, v2 = iho.adam_head(head, z, z, g, k, 5e-4, 0.9, 0.99, 1e-8, np.float32(0.9), np.float32(0.99))
    wa, ma, va = iho.adam_step(head, z, z, g, 5e-4, 0.9, 0.99, 1e-8, np.float32(0.9), np.float32(0.99))
    assert np.array_equal(w2, wa) and np.array_equal(m2, ma) and np.array_equal(v2, va)  # no regulariser: one ApplyAdam
