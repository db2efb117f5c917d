"""The semi-supervised step of ICNet's output-layer trainer without a GPU: the four new symbols and
their ctypes signatures, the host-only workspace queries, the statuses given before a device is touched, the keyword
validation of SemiSupervisedICNetHeadTrainer, from_params' active_learning section, the state round trip with
ICNetHeadTrainer -- and ICNetHeadTrainer still refusing the keywords."""
import ctypes

import numpy as np
import pytest

import semanticsegmentationactivelearning_amd as ssal
from semanticsegmentationactivelearning_amd import _lib, training
from semanticsegmentationactivelearning_amd.training import ICNetHeadTrainer, SemiSupervisedICNetHeadTrainer

HYPER = {"learning_rate": 0.0005, "learning_rate_decay": 0.0,
         "optimizer": {"type": "Adam", "kwargs": {"beta1": 0.9, "beta2": 0.99}},
         "weight_reg": {"L2": 0.0002, "L1": 0.0, "glorot_scaling": False},
         "softmax": {"label_smoothing": 0.0, "loginverse_scaling": 1.02, "multiscale": False}}


def _icnet(k=19):
    net = ssal.ICNet(k)
    net.build((None, None, None, 3))
    return net


def test_abi_symbols_and_signatures():
    """fails on a library without the entries"""
    L = _lib.lib()
    i, i64, f, vp = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
    want = {
        "ssal_icnet_head_grad_semi_workspace_bytes": (i64, [i, i, i, i, i]),
        "ssal_icnet_head_grad_semi_nhwc": (i, [vp, vp, i, i, i, i, vp, vp, vp, vp, i, f, f, f, i, vp, vp, vp, vp, vp, i64, vp]),
        "ssal_icnet_train_head_semi_workspace_bytes": (i64, [vp, i, i, i, i]),
        "ssal_icnet_train_head_semi_nhwc": (i, [vp, vp, vp, i, i, i, i, vp, vp, vp, i, f, vp, f, f, i, vp, vp, vp, vp, vp, i64,
                                                vp]),
    }
    for name, proto in want.items():
        assert _lib.PROTOTYPES[name] == proto, name
        assert hasattr(L, name)
    assert "SemiSupervisedICNetHeadTrainer" in training.__all__
    # the argument order is the ENet semi entries' (max_workgroups aside): one assembly of the call serves both
    enet = _lib.PROTOTYPES["ssal_final_grad_semi_nhwc"][1]
    mine = want["ssal_icnet_head_grad_semi_nhwc"][1]
    assert mine[:14] == enet[:14] and mine[15:] == enet[14:]


def test_workspace_queries():
    """with_raw adds exactly one byte per loss pixel to the features query; the semi form adds the histogram replicas to the
    plain one; the -1 limits sit at icnet_head_fits' boundaries"""
    L = _lib.lib()
    semi, plain = L.ssal_icnet_head_grad_semi_workspace_bytes, L.ssal_icnet_head_grad_workspace_bytes
    for n, h, w, k in ((1, 1, 1, 2), (2, 3, 5, 19), (8, 128, 256, 19), (3, 7, 11, 32)):
        assert semi(n, h, w, k, 1) - semi(n, h, w, k, 0) == n * 8 * h * 8 * w
        assert plain(n, h, w, k) < semi(n, h, w, k, 0) <= plain(n, h, w, k) + 64 * 1024 * 8 + 512
    assert semi(1, 8, 8, 1, 0) == -1 and semi(1, 8, 8, 33, 1) == -1 and semi(0, 8, 8, 19, 0) == -1 and semi(1, 0, 8, 19, 0) == -1
    top = 1 << 27
    for raw in (0, 1):
        assert semi(1, top, 1, 2, raw) > 0 and semi(1, top + 1, 1, 2, raw) == -1
        assert semi(1, 1, top, 2, raw) > 0 and semi(1, 1, top + 1, 2, raw) == -1
        assert semi(1, top, 252, 2, raw) > 0 and semi(1, top, 253, 2, raw) == -1  # 2^25 x 64 tiles = 2^31
        assert semi(1, 4 * 46340, 4 * 46340, 2, raw) > 0 and semi(1, 4 * 46340 + 1, 4 * 46340 + 1, 2, raw) == -1
    h = ctypes.c_void_p()
    _lib.check(L.ssal_icnet_create(3, 19, ctypes.byref(h)))
    assert L.ssal_icnet_train_head_semi_workspace_bytes(h, 1, 64, 64, 0) == -1  # not committed
    assert L.ssal_icnet_train_head_semi_workspace_bytes(None, 1, 64, 64, 1) == -1
    _lib.check(L.ssal_icnet_destroy(h))


def test_statuses_before_any_device_work():
    L = _lib.lib()
    k = 19
    p = ctypes.c_void_p(256)
    ws = L.ssal_icnet_head_grad_semi_workspace_bytes
    big = 1 << 30

    def call(x=p, raw=None, n=1, h=1, w=1, classes=k, labels=p, mask=p, labelled=p, measure=0, mw=0, ws_bytes=big):
        return L.ssal_icnet_head_grad_semi_nhwc(x, raw, n, h, w, classes, p, labels, mask, labelled, measure, 0.5, 0.0, 0.0,
                                                mw, p, p, None, None, p, ws_bytes, None)

    assert call(x=None) == _lib.SSAL_EINVAL and b"NULL device pointer" in L.ssal_last_error()
    assert call(classes=1) == _lib.SSAL_EINVAL and call(classes=33) == _lib.SSAL_EINVAL
    assert b"classes must be in [2,32]" in L.ssal_last_error()
    assert call(n=0) == _lib.SSAL_EINVAL
    assert call(mw=-1) == _lib.SSAL_EINVAL and b"max_workgroups" in L.ssal_last_error()
    assert call(h=(1 << 27) + 1) == _lib.SSAL_EINVAL
    assert call(measure=3) == _lib.SSAL_ENOTIMPL and b"Uncertainty function not implemented" in L.ssal_last_error()
    assert call(measure=-1) == _lib.SSAL_ENOTIMPL
    assert call(labels=None, mask=None, labelled=None) == _lib.SSAL_EINVAL and b"may be NULL only" in L.ssal_last_error()
    assert call(ws_bytes=ws(1, 1, 1, k, 0) - 512) == _lib.SSAL_ENOMEM and b"workspace too small" in L.ssal_last_error()
    # a raw side needs the target plane too: 8 x 128 x 256 features at the size of the call without one
    assert call(raw=p, n=8, h=128, w=256, ws_bytes=ws(8, 128, 256, k, 0)) == _lib.SSAL_ENOMEM
    # the images entry needs a committed handle
    h = ctypes.c_void_p()
    _lib.check(L.ssal_icnet_create(3, k, ctypes.byref(h)))
    rc = L.ssal_icnet_train_head_semi_nhwc(h, p, None, 0, 1, 64, 64, p, p, p, 0, 0.5, p, 0.0, 0.0, 0, p, p, None, None, p, big,
                                           None)
    assert rc == _lib.SSAL_ESTATE
    rc = L.ssal_icnet_train_head_semi_nhwc(None, p, None, 0, 1, 64, 64, p, p, p, 0, 0.5, p, 0.0, 0.0, 0, p, p, None, None, p, big,
                                           None)
    assert rc == _lib.SSAL_EINVAL
    _lib.check(L.ssal_icnet_destroy(h))


def test_keyword_validation_before_any_device_work(monkeypatch):
    def no_gpu():
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    net = _icnet()
    tr = SemiSupervisedICNetHeadTrainer(net, 1e-3)
    x = np.zeros((2, 1, 2, 128), np.float32)
    lab, msk = np.zeros((2, 8, 16), np.uint8), np.ones((2, 8, 16), np.float32)
    img = np.zeros((2, 32, 32, 3), np.float32)
    ilab, imsk = np.zeros((2, 32, 32), np.uint8), np.ones((2, 32, 32), np.float32)
    cm = np.zeros((19, 19), np.int64)
    for call, args in ((tr.gradient_features, (x, lab, msk)), (tr.step_features, (x, lab, msk)), (tr.step, (img, ilab, imsk))):
        with pytest.raises(ValueError, match="labelled"):
            call(*args, labelled=np.ones(3, np.uint8))
        with pytest.raises(ValueError, match="confusion"):
            call(*args, confusion=cm.astype(np.int32))
        with pytest.raises(ValueError, match="confusion"):
            call(*args, confusion=np.zeros((19, 18), np.int64))
        with pytest.raises(ValueError, match="None only"):
            call(args[0], None, None, labelled=np.array([0, 1]))
        with pytest.raises(ValueError, match="None only"):
            call(args[0], None, None)
        with pytest.raises(NotImplementedError, match="Uncertainty function not implemented."):
            call(*args, labelled=np.array([0, 1]), measure="bald")
        with pytest.raises(ValueError, match="max_workgroups"):
            call(*args, labelled=np.array([0, 1]), max_workgroups=-1)
        with pytest.raises(ValueError):
            call(args[0], args[1][:, :4], args[2], labelled=np.array([0, 1]))
    with pytest.raises(NotImplementedError):
        SemiSupervisedICNetHeadTrainer(net, 1e-3, measure="bald")
    enet = ssal.ENet(19)
    enet.build((None, None, None, 3))
    with pytest.raises(NotImplementedError):
        SemiSupervisedICNetHeadTrainer(enet, 1e-3)


def test_from_params_active_learning_section():
    net = _icnet()
    tr = SemiSupervisedICNetHeadTrainer.from_params(net, {"hyperparams": HYPER,
                                                          "active_learning": {"measure": "margin", "threshold": 0.25}})
    assert (tr.measure, tr.threshold) == ("margin", 0.25)
    assert (tr.learning_rate, tr.beta1, tr.beta2, tr.l2, tr.weight) == (0.0005, 0.9, 0.99, 0.0002, 1.02)
    tr = SemiSupervisedICNetHeadTrainer.from_params(net, {"hyperparams": HYPER})
    assert (tr.measure, tr.threshold) == ("entropy", 0.0)
    # the keywords default to the trainer's: the verdict of _semi carries them
    assert tr._semi(2, None, None, np.array([0, 0]), None, None, None, False)[1:] == (_lib.MEASURES["entropy"], 0.0)
    tr = SemiSupervisedICNetHeadTrainer(net, 1e-3, measure="confidence", threshold=0.75)
    assert tr._semi(2, None, None, np.array([0, 0]), None, None, None, False)[1:] == (_lib.MEASURES["confidence"], 0.75)
    assert tr._semi(2, None, None, np.array([0, 0]), "margin", 0.5, None, False)[1:] == (_lib.MEASURES["margin"], 0.5)
    with pytest.raises(NotImplementedError):
        SemiSupervisedICNetHeadTrainer.from_params(net, {"hyperparams": dict(HYPER, softmax={"multiscale": True})})
    with pytest.raises(NotImplementedError):
        SemiSupervisedICNetHeadTrainer.from_params(net, {"hyperparams": dict(HYPER, weight_reg={"glorot_scaling": True})})


def test_state_round_trip_with_the_plain_trainer():
    net = _icnet(6)
    plain, semi = ICNetHeadTrainer(net, 1e-3), SemiSupervisedICNetHeadTrainer(net, 1e-3)
    rng = np.random.default_rng(0)
    st = plain.state
    for key in ("m", "v"):
        for name in st[key]:
            st[key][name] = rng.standard_normal(st[key][name].shape).astype(np.float32)
    st["t"] = 7
    semi.load_state(st)
    back = semi.state
    plain.load_state(back)
    again = plain.state
    assert back["t"] == again["t"] == 7
    for key in ("m", "v"):
        assert set(back[key]) == {"conv6_cls.kernel", "conv6_cls.bias"}
        for name in st[key]:
            assert np.array_equal(back[key][name], st[key][name]) and np.array_equal(again[key][name], st[key][name])
    assert semi.variable_names == plain.variable_names and semi._adam_ranges() == plain._adam_ranges()
    assert float(semi._b1p) == float(plain._b1p) and float(semi._b2p) == float(plain._b2p)


def test_the_plain_trainer_still_refuses(monkeypatch):
    def no_gpu():
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    tr = ICNetHeadTrainer(_icnet(), 1e-3)
    x = np.zeros((1, 1, 2, 128), np.float32)
    lab, msk = np.zeros((1, 8, 16), np.uint8), np.ones((1, 8, 16), np.float32)
    for kw in ({"labelled": np.array([1])}, {"confusion": np.zeros((19, 19), np.int64)}, {"return_pseudo_pixels": True}):
        with pytest.raises(NotImplementedError):
            tr.gradient_features(x, lab, msk, **kw)
        with pytest.raises(NotImplementedError):
            tr.step_features(x, lab, msk, **kw)
    for kw in ({"measure": "margin"}, {"threshold": 0.5}, {"features_raw": x}):
        with pytest.raises(TypeError):
            tr.gradient_features(x, lab, msk, **kw)
    assert ICNetHeadTrainer._C_FEATURES == ("ssal_icnet_head_grad", None)
