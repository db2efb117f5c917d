"""The semi-supervised step of ICNet's fusion and cascade trainers without a GPU: the eight new symbols
and their ctypes signatures, the host-only workspace queries, the statuses given before a device is touched, the keyword
validation of the two new trainers (a partial ``features_raw`` among it), from_params' active_learning section, the state
round trip with the parent classes -- and the parent classes still refusing the keywords."""
import ctypes

import numpy as np
import pytest

import semanticsegmentationactivelearning_amd as ssal
from semanticsegmentationactivelearning_amd import _lib, training
from semanticsegmentationactivelearning_amd.training import (ICNetCascadeTrainer, ICNetFusionTrainer,
                                                             SemiSupervisedICNetCascadeTrainer,
                                                             SemiSupervisedICNetFusionTrainer)

HYPER = {"learning_rate": 0.0005, "learning_rate_decay": 0.0,
         "optimizer": {"type": "Adam", "kwargs": {"beta1": 0.9, "beta2": 0.99}},
         "weight_reg": {"L2": 0.0002, "L1": 0.0, "glorot_scaling": False},
         "softmax": {"label_smoothing": 0.0, "loginverse_scaling": 1.02, "multiscale": False}}
PAIRS = ((ICNetFusionTrainer, SemiSupervisedICNetFusionTrainer), (ICNetCascadeTrainer, SemiSupervisedICNetCascadeTrainer))


def _icnet(k=19):
    net = ssal.ICNet(k)
    net.build((None, None, None, 3))
    return net


def test_abi_symbols_and_signatures():
    """fails on a library without the entries"""
    L = _lib.lib()
    i, i64, f, vp = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
    tail = [i, i, i, i, vp, vp, vp, vp, i, f, f, f, vp, i, vp, vp, vp, vp, vp, i64, vp]
    images = (i, [vp, vp, vp, i, i, i, i, vp, vp, vp, i, f, vp, f, f, vp, i, vp, vp, vp, vp, vp, i64, vp])
    want = {
        "ssal_icnet_fusion_grad_semi_workspace_bytes": (i64, [i, i, i, i, i]),
        "ssal_icnet_fusion_grad_semi_nhwc": (i, [vp] * 4 + tail),
        "ssal_icnet_train_fusion_semi_workspace_bytes": (i64, [vp, i, i, i, i]),
        "ssal_icnet_train_fusion_semi_nhwc": images,
        "ssal_icnet_cascade_grad_semi_workspace_bytes": (i64, [i, i, i, i, i]),
        "ssal_icnet_cascade_grad_semi_nhwc": (i, [vp] * 6 + tail),
        "ssal_icnet_train_cascade_semi_workspace_bytes": (i64, [vp, i, i, i, i]),
        "ssal_icnet_train_cascade_semi_nhwc": images,
    }
    for name, proto in want.items():
        assert _lib.PROTOTYPES[name] == proto, name
        assert hasattr(L, name)
    assert "SemiSupervisedICNetFusionTrainer" in training.__all__
    assert "SemiSupervisedICNetCascadeTrainer" in training.__all__
    assert SemiSupervisedICNetFusionTrainer.__mro__[1:3] == (training._SemiKeywords, ICNetFusionTrainer)
    assert SemiSupervisedICNetCascadeTrainer.__mro__[1:3] == (training._SemiKeywords, ICNetCascadeTrainer)
    # the argument order mirrors the head's semi entries: what a semi entry adds to its plain sibling sits after the training
    # features, after the mask and after the gradient, so one assembly of the call serves all of them
    for stem, feats in (("ssal_icnet_fusion_grad", 2), ("ssal_icnet_cascade_grad", 3)):
        plain, semi = _lib.PROTOTYPES[stem + "_nhwc"][1], _lib.PROTOTYPES[stem + "_semi_nhwc"][1]
        m = feats + 7  # features, n h w classes, params, labels, mask
        assert semi[:feats] == plain[:feats] and semi[feats:2 * feats] == [vp] * feats
        assert semi[2 * feats:feats + m] == plain[feats:m] and semi[feats + m:feats + m + 3] == [vp, i, f]
        assert semi[feats + m + 3:feats + m + 9] == plain[m:m + 6] and semi[feats + m + 9:feats + m + 11] == [vp, vp]
        assert semi[feats + m + 11:] == plain[m + 6:]
    for stem in ("ssal_icnet_train_fusion", "ssal_icnet_train_cascade"):
        assert _lib.PROTOTYPES[stem + "_semi_nhwc"][1][:12] == _lib.PROTOTYPES["ssal_icnet_train_head_semi_nhwc"][1][:12]


def test_workspace_queries():
    """with_raw adds exactly one byte per loss pixel; the semi form adds the histogram replicas to the plain one; the -1 limits
    sit at icnet_fusion_fits' / icnet_cascade_fits' boundaries, where the plain queries have them"""
    L = _lib.lib()
    for stem, up, top in (("ssal_icnet_fusion_grad", 16, 1 << 26), ("ssal_icnet_cascade_grad", 32, 1 << 25)):
        semi, plain = getattr(L, stem + "_semi_workspace_bytes"), getattr(L, stem + "_workspace_bytes")
        for n, h, w, k in ((1, 1, 1, 2), (2, 2, 3, 19), (8, 1024 // up, 2048 // up, 19), (3, 7, 11, 32)):
            assert semi(n, h, w, k, 1) - semi(n, h, w, k, 0) == n * up * h * up * w
            assert plain(n, h, w, k) < semi(n, h, w, k, 0) <= plain(n, h, w, k) + 64 * 1024 * 8 + 512
        assert semi(1, 8, 8, 1, 0) == -1 and semi(1, 8, 8, 33, 1) == -1 and semi(0, 8, 8, 19, 0) == -1
        assert semi(1, 0, 8, 19, 0) == -1 and semi(-1, 8, 8, 19, 1) == -1
        wide = 126 * 16 // up  # the last width at which `top` rows of features still give fewer than 2^31 head tiles
        for raw in (0, 1):
            assert semi(1, top, 1, 2, raw) > 0 and semi(1, top + 1, 1, 2, raw) == -1
            assert semi(1, 1, top, 2, raw) > 0 and semi(1, 1, top + 1, 2, raw) == -1
            assert semi(1, top, wide, 2, raw) > 0 and semi(1, top, wide + 1, 2, raw) == -1
            for dims in ((1, top, wide, 2), (1, top, wide + 1, 2), (1, top + 1, 1, 2), (4096, 1 << 13, 1 << 13, 19),
                         (4097, 1 << 13, 1 << 13, 19), (1, 46340 * 32 // up, 46340 * 32 // up, 2)):
                assert (semi(*dims, raw) == -1) == (plain(*dims) == -1), (stem, dims)
    h = ctypes.c_void_p()
    _lib.check(L.ssal_icnet_create(3, 19, ctypes.byref(h)))
    for stem in ("ssal_icnet_train_fusion", "ssal_icnet_train_cascade"):
        query = getattr(L, stem + "_semi_workspace_bytes")
        assert query(h, 1, 64, 64, 0) == -1  # not committed
        assert query(None, 1, 64, 64, 1) == -1
    _lib.check(L.ssal_icnet_destroy(h))


@pytest.mark.parametrize("stem,feats,up", [("ssal_icnet_fusion_grad", 2, 16), ("ssal_icnet_cascade_grad", 3, 32)])
def test_statuses_before_any_device_work(stem, feats, up):
    L = _lib.lib()
    k = 19
    p = ctypes.c_void_p(256)
    ws = getattr(L, stem + "_semi_workspace_bytes")
    entry = getattr(L, stem + "_semi_nhwc")
    big = 1 << 34

    def call(x=None, raw=None, n=1, h=1, w=1, classes=k, params=p, labels=p, mask=p, labelled=p, measure=0, stats=p, mw=0,
             loss=p, grad=p, ws_dev=p, ws_bytes=big):
        x = [p] * feats if x is None else x
        raw = [None] * feats if raw is None else raw
        return entry(*x, *raw, n, h, w, classes, params, labels, mask, labelled, measure, 0.5, 0.0, 0.0, stats, mw, loss, grad,
                     None, None, ws_dev, ws_bytes, None)

    for j in range(feats):
        assert call(x=[None if i == j else p for i in range(feats)]) == _lib.SSAL_EINVAL
        assert b"NULL device pointer" in L.ssal_last_error()
    for kw in ("params", "stats", "loss", "grad", "ws_dev"):
        assert call(**{kw: None}) == _lib.SSAL_EINVAL, kw
    assert call(classes=1) == _lib.SSAL_EINVAL and call(classes=33) == _lib.SSAL_EINVAL
    assert b"classes must be in [2,32]" in L.ssal_last_error()
    assert call(n=0) == _lib.SSAL_EINVAL
    assert call(mw=-1) == _lib.SSAL_EINVAL and b"max_workgroups" in L.ssal_last_error()
    assert call(h=(1 << 26) * 16 // up + 1) == _lib.SSAL_EINVAL and b"beyond" in L.ssal_last_error()
    assert call(measure=3) == _lib.SSAL_ENOTIMPL and b"Uncertainty function not implemented" in L.ssal_last_error()
    assert call(measure=-1) == _lib.SSAL_ENOTIMPL
    assert call(labels=None, mask=None, labelled=None) == _lib.SSAL_EINVAL and b"may be NULL only" in L.ssal_last_error()
    assert call(labels=None, labelled=None) == _lib.SSAL_EINVAL
    # the raw pointers come all or none
    for given in range(1, 2 ** feats - 1):
        raw = [p if given >> j & 1 else None for j in range(feats)]
        assert call(raw=raw) == _lib.SSAL_EINVAL and b"given together" in L.ssal_last_error(), raw
    assert call(ws_bytes=ws(1, 1, 1, k, 0) - 512) == _lib.SSAL_ENOMEM and b"workspace too small" in L.ssal_last_error()
    # a raw side needs the target plane too: a batch of 8 x 1024 x 2048 at the size of the call without one
    h, w = 1024 // up, 2048 // up
    assert call(raw=[p] * feats, n=8, h=h, w=w, ws_bytes=ws(8, h, w, k, 0)) == _lib.SSAL_ENOMEM
    # the images entry needs a committed handle
    images = getattr(L, stem.replace("icnet_", "icnet_train_").replace("_grad", "") + "_semi_nhwc")
    hd = ctypes.c_void_p()
    _lib.check(L.ssal_icnet_create(3, k, ctypes.byref(hd)))
    rest = (0, 1, 64, 64, p, p, p, 0, 0.5, p, 0.0, 0.0, p, 0, p, p, None, None, p, big, None)
    assert images(hd, p, None, *rest) == _lib.SSAL_ESTATE
    assert images(None, p, None, *rest) == _lib.SSAL_EINVAL
    _lib.check(L.ssal_icnet_destroy(hd))


def _inputs(semi_cls):
    """host stand-ins of (features, labels, mask) and (images, labels, mask) for a batch of two"""
    if issubclass(semi_cls, ICNetCascadeTrainer):
        feats = (np.zeros((2, 1, 2, 256), np.float32), np.zeros((2, 2, 4, 256), np.float32), np.zeros((2, 4, 8, 64), np.float32))
        up = 32
    else:
        feats = (np.zeros((2, 1, 2, 128), np.float32), np.zeros((2, 2, 4, 64), np.float32))
        up = 16
    lab, msk = np.zeros((2, up, 2 * up), np.uint8), np.ones((2, up, 2 * up), np.float32)
    img = np.zeros((2, 32, 32, 3), np.float32)
    return feats, lab, msk, (img, np.zeros((2, 32, 32), np.uint8), np.ones((2, 32, 32), np.float32))


@pytest.mark.parametrize("plain_cls,semi_cls", PAIRS)
def test_keyword_validation_before_any_device_work(monkeypatch, plain_cls, semi_cls):
    def no_gpu():
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    net = _icnet()
    tr = semi_cls(net, 1e-3)
    feats, lab, msk, images = _inputs(semi_cls)
    nf = len(feats)
    cm = np.zeros((19, 19), np.int64)
    for call, args in ((tr.gradient_features, feats + (lab, msk)), (tr.step_features, feats + (lab, msk)), (tr.step, images)):
        lead = len(args) - 2
        with pytest.raises(ValueError, match="labelled"):
            call(*args, labelled=np.ones(3, np.uint8))
        with pytest.raises(ValueError, match="confusion"):
            call(*args, confusion=cm.astype(np.int32))
        with pytest.raises(ValueError, match="confusion"):
            call(*args, confusion=np.zeros((19, 18), np.int64))
        with pytest.raises(ValueError, match="None only"):
            call(*args[:lead], None, None, labelled=np.array([0, 1]))
        with pytest.raises(ValueError, match="None only"):
            call(*args[:lead], None, None)
        with pytest.raises(NotImplementedError, match="Uncertainty function not implemented."):
            call(*args, labelled=np.array([0, 1]), measure="bald")
        with pytest.raises(ValueError, match="max_workgroups"):
            call(*args, labelled=np.array([0, 1]), max_workgroups=-1)
        with pytest.raises(ValueError):
            call(*args[:lead], args[lead][:, :4], args[lead + 1], labelled=np.array([0, 1]))
    # features_raw: the whole tuple features() returns, every member shaped like its counterpart
    for call in (tr.gradient_features, tr.step_features):
        for raw in (feats[:-1], feats[0], feats[:-1] + (None,), feats + feats[:1]):
            with pytest.raises(ValueError, match="whole or not at all"):
                call(*feats, lab, msk, labelled=np.array([0, 1]), features_raw=raw)
        with pytest.raises(ValueError, match="counterpart"):
            call(*feats, lab, msk, labelled=np.array([0, 1]), features_raw=feats[:-1] + (feats[-1][:, :1],))
        with pytest.raises(ValueError):  # the features themselves are still judged as the parent judges them
            call(*(feats[:-1] + (feats[-1][:, :1],)), lab, msk, labelled=np.array([0, 1]))
    with pytest.raises(NotImplementedError):
        semi_cls(net, 1e-3, measure="bald")
    enet = ssal.ENet(19)
    enet.build((None, None, None, 3))
    with pytest.raises(NotImplementedError):
        semi_cls(enet, 1e-3)
    assert nf == len(semi_cls._FEATURE_NAMES)


@pytest.mark.parametrize("plain_cls,semi_cls", PAIRS)
def test_from_params_active_learning_section(plain_cls, semi_cls):
    net = _icnet()
    tr = semi_cls.from_params(net, {"hyperparams": HYPER, "active_learning": {"measure": "margin", "threshold": 0.25}})
    assert (tr.measure, tr.threshold) == ("margin", 0.25)
    assert (tr.learning_rate, tr.beta1, tr.beta2, tr.l2, tr.weight) == (0.0005, 0.9, 0.99, 0.0002, 1.02)
    tr = semi_cls.from_params(net, {"hyperparams": HYPER})
    assert (tr.measure, tr.threshold) == ("entropy", 0.0)
    # the keywords default to the trainer's: the verdict of _semi carries them
    assert tr._semi(2, None, None, np.array([0, 0]), None, None, None, False)[1:] == (_lib.MEASURES["entropy"], 0.0)
    tr = semi_cls(net, 1e-3, measure="confidence", threshold=0.75)
    assert tr._semi(2, None, None, np.array([0, 0]), None, None, None, False)[1:] == (_lib.MEASURES["confidence"], 0.75)
    assert tr._semi(2, None, None, np.array([0, 0]), "margin", 0.5, None, False)[1:] == (_lib.MEASURES["margin"], 0.5)
    with pytest.raises(NotImplementedError):
        semi_cls.from_params(net, {"hyperparams": dict(HYPER, softmax={"multiscale": True})})
    with pytest.raises(NotImplementedError):
        semi_cls.from_params(net, {"hyperparams": dict(HYPER, weight_reg={"glorot_scaling": True})})


@pytest.mark.parametrize("plain_cls,semi_cls", PAIRS)
def test_state_round_trip_with_the_plain_trainer(plain_cls, semi_cls):
    net = _icnet(6)
    plain, semi = plain_cls(net, 1e-3), semi_cls(net, 1e-3)
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
        assert list(back[key]) == plain.variable_names
        for name in st[key]:
            assert np.array_equal(back[key][name], st[key][name]) and np.array_equal(again[key][name], st[key][name])
    assert semi.variable_names == plain.variable_names and semi._adam_ranges() == plain._adam_ranges()
    assert float(semi._b1p) == float(plain._b1p) and float(semi._b2p) == float(plain._b2p)
    assert semi_cls._C_FEATURES[0] == plain_cls._C_FEATURES[0] and semi_cls._C_IMAGES[0] == plain_cls._C_IMAGES[0]


@pytest.mark.parametrize("plain_cls,semi_cls", PAIRS)
def test_the_plain_trainers_still_refuse(monkeypatch, plain_cls, semi_cls):
    def no_gpu():
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    tr = plain_cls(_icnet(), 1e-3)
    feats, lab, msk, images = _inputs(semi_cls)
    for kw in ({"labelled": np.array([1, 1])}, {"confusion": np.zeros((19, 19), np.int64)}, {"return_pseudo_pixels": True}):
        with pytest.raises(NotImplementedError):
            tr.gradient_features(*feats, lab, msk, **kw)
        with pytest.raises(NotImplementedError):
            tr.step_features(*feats, lab, msk, **kw)
        with pytest.raises(NotImplementedError):
            tr.step(*images, **kw)
    for kw in ({"measure": "margin"}, {"threshold": 0.5}, {"features_raw": feats}):
        with pytest.raises(TypeError):
            tr.gradient_features(*feats, lab, msk, **kw)
    assert plain_cls._C_FEATURES[1] is None and plain_cls._C_IMAGES[1] is None
