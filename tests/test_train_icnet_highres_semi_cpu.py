"""The semi-supervised step of ICNet's high-resolution trainer without a GPU: the four new symbols and
their ctypes signatures, the host-only workspace queries, the statuses given before a device is touched (a partial raw triple
among them), the keyword validation of the new trainer (a partial or mis-shaped ``features_raw``), from_params' active_learning
section, the state round trip with the parent class, the parent still refusing the keywords -- and the route the raw side takes
for conv1_sub1 + conv2_sub1 (one k_front2 launch, or the two separate launches), pinned to launch_front2's guards restated in
tests/icnet_limits.py on both sides of the entries' own limit."""
import ctypes

import numpy as np
import pytest

import icnet_limits as lim
import semanticsegmentationactivelearning_amd as ssal
from semanticsegmentationactivelearning_amd import _lib, training
from semanticsegmentationactivelearning_amd.training import ICNetHighResTrainer, SemiSupervisedICNetHighResTrainer

HYPER = {"learning_rate": 0.0005, "learning_rate_decay": 0.0,
         "optimizer": {"type": "Adam", "kwargs": {"beta1": 0.9, "beta2": 0.99}},
         "weight_reg": {"L2": 0.0002, "L1": 0.0, "glorot_scaling": False},
         "softmax": {"label_smoothing": 0.0, "loginverse_scaling": 1.02, "multiscale": False}}
SEMI = SemiSupervisedICNetHighResTrainer


def _icnet(k=19, c_in=3):
    net = ssal.ICNet(k)
    net.build((None, None, None, c_in))
    return net


def test_abi_symbols_and_signatures():
    """fails on a library without the entries"""
    L = _lib.lib()
    i, i64, f, vp = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
    want = {
        "ssal_icnet_highres_grad_semi_workspace_bytes": (i64, [i, i, i, i, i]),
        "ssal_icnet_highres_grad_semi_nhwc": (i, [vp] * 6 + [i, i, i, i, vp, vp, vp, vp, i, f, f, f, vp, i, i, i, vp, vp, vp, vp,
                                                            vp, i64, vp]),
        "ssal_icnet_train_highres_semi_workspace_bytes": (i64, [vp, i, i, i, i]),
        "ssal_icnet_train_highres_semi_nhwc": (i, [vp, vp, vp, i, i, i, i, vp, vp, vp, i, f, vp, f, f, vp, i, vp, vp, vp, vp, vp,
                                                   i64, vp]),
    }
    for name, proto in want.items():
        assert _lib.PROTOTYPES[name] == proto, name
        assert hasattr(L, name)
    assert "SemiSupervisedICNetHighResTrainer" in training.__all__
    assert SEMI.__mro__[1:3] == (training._SemiKeywords, ICNetHighResTrainer)
    # the argument order mirrors the cascade's semi entries, applied to the plain highres entries: what a semi entry adds to its
    # plain sibling sits after the training inputs, after the mask and after the gradient
    plain, semi = _lib.PROTOTYPES["ssal_icnet_highres_grad_nhwc"][1], _lib.PROTOTYPES["ssal_icnet_highres_grad_semi_nhwc"][1]
    m = 3 + 7  # inputs, n h w classes, params, labels, mask
    assert semi[:3] == plain[:3] and semi[3:6] == [vp] * 3
    assert semi[6:3 + m] == plain[3:m] and semi[3 + m:3 + m + 3] == [vp, i, f]
    # weight, label_smoothing, stats, x_is_u8, c_in, max_workgroups, loss, grad where the plain entry has them
    assert semi[3 + m + 3:3 + m + 11] == plain[m:m + 8] and semi[3 + m + 11:3 + m + 13] == [vp, vp]
    assert semi[3 + m + 13:] == plain[m + 8:]
    assert _lib.PROTOTYPES["ssal_icnet_train_highres_semi_nhwc"] == _lib.PROTOTYPES["ssal_icnet_train_cascade_semi_nhwc"]
    assert SEMI._C_FEATURES == ("ssal_icnet_highres_grad", "ssal_icnet_highres_grad_semi")
    assert SEMI._C_IMAGES == ("ssal_icnet_train_highres", "ssal_icnet_train_highres_semi")


SHAPES = ((1, 1, 1, 2), (2, 2, 3, 19), (8, 32, 64, 19), (3, 7, 11, 32))


def test_workspace_queries():
    """with_raw adds exactly the cascade semi query's addition (one byte per loss pixel); semi minus plain equals the cascade's
    semi minus plain (there is no second set of feature slots); -1 wherever the plain query gives it, at icnet_highres_fits'
    boundaries among them"""
    L = _lib.lib()
    semi, plain = L.ssal_icnet_highres_grad_semi_workspace_bytes, L.ssal_icnet_highres_grad_workspace_bytes
    csemi, cplain = L.ssal_icnet_cascade_grad_semi_workspace_bytes, L.ssal_icnet_cascade_grad_workspace_bytes
    for n, h, w, k in SHAPES:
        assert semi(n, h, w, k, 1) - semi(n, h, w, k, 0) == csemi(n, h, w, k, 1) - csemi(n, h, w, k, 0) == n * 32 * h * 32 * w
        for raw in (0, 1):
            assert semi(n, h, w, k, raw) - plain(n, h, w, k) == csemi(n, h, w, k, raw) - cplain(n, h, w, k) > 0
    assert semi(1, 8, 8, 1, 0) == -1 and semi(1, 8, 8, 33, 1) == -1 and semi(0, 8, 8, 19, 0) == -1
    assert semi(1, 0, 8, 19, 0) == -1 and semi(-1, 8, 8, 19, 1) == -1
    top = 131072  # n h32 w32 < 2^17: n (32 h32) (32 w32) < 2^27 frame pixels
    for raw in (0, 1):
        assert semi(1, 1, top - 1, 2, raw) > 0 and semi(1, 1, top, 2, raw) == -1
        assert semi(1, top - 1, 1, 2, raw) > 0 and semi(1, top, 1, 2, raw) == -1
        assert semi(8, 128, 127, 19, raw) > 0 and semi(8, 128, 128, 19, raw) == -1
        assert semi(top - 1, 1, 1, 19, raw) > 0 and semi(top, 1, 1, 19, raw) == -1
        for dims in ((1, 1, top - 1, 2), (1, 1, top, 2), (1, 362, 362, 19), (1, 363, 362, 19), (31, 64, 64, 19), (32, 64, 64, 19),
                     (4097, 1 << 13, 1 << 13, 19), (1, 1 << 20, 1, 2)):
            assert (semi(*dims, raw) == -1) == (plain(*dims) == -1), dims
    h = ctypes.c_void_p()
    _lib.check(L.ssal_icnet_create(3, 19, ctypes.byref(h)))
    query = L.ssal_icnet_train_highres_semi_workspace_bytes
    assert query(h, 1, 64, 64, 0) == -1  # not committed
    assert query(None, 1, 64, 64, 1) == -1
    _lib.check(L.ssal_icnet_destroy(h))


def test_statuses_before_any_device_work():
    L = _lib.lib()
    k = 19
    p = ctypes.c_void_p(256)
    ws = L.ssal_icnet_highres_grad_semi_workspace_bytes
    entry = L.ssal_icnet_highres_grad_semi_nhwc
    big = 1 << 36

    def call(x=None, raw=None, n=1, h=1, w=1, classes=k, params=p, labels=p, mask=p, labelled=p, measure=0, stats=p, u8=0,
             c_in=3, mw=0, loss=p, grad=p, ws_dev=p, ws_bytes=big):
        x = [p] * 3 if x is None else x
        raw = [None] * 3 if raw is None else raw
        return entry(*x, *raw, n, h, w, classes, params, labels, mask, labelled, measure, 0.5, 0.0, 0.0, stats, u8, c_in, mw,
                     loss, grad, None, None, ws_dev, ws_bytes, None)

    for j in range(3):
        assert call(x=[None if i == j else p for i in range(3)]) == _lib.SSAL_EINVAL
        assert b"NULL device pointer" in L.ssal_last_error()
    for kw in ("params", "stats", "loss", "grad", "ws_dev"):
        assert call(**{kw: None}) == _lib.SSAL_EINVAL, kw
    assert call(classes=1) == _lib.SSAL_EINVAL and call(classes=33) == _lib.SSAL_EINVAL
    assert b"classes must be in [2,32]" in L.ssal_last_error()
    assert call(n=0) == _lib.SSAL_EINVAL
    assert call(mw=-1) == _lib.SSAL_EINVAL and b"max_workgroups" in L.ssal_last_error()
    assert call(h=131072) == _lib.SSAL_EINVAL and b"beyond" in L.ssal_last_error()
    for c_in in (1, 2, 5):
        assert call(c_in=c_in) == _lib.SSAL_EINVAL and b"3 or 4 input channels" in L.ssal_last_error()
    assert call(measure=3) == _lib.SSAL_ENOTIMPL and b"Uncertainty function not implemented" in L.ssal_last_error()
    assert call(measure=-1) == _lib.SSAL_ENOTIMPL
    assert call(labels=None, mask=None, labelled=None) == _lib.SSAL_EINVAL and b"may be NULL only" in L.ssal_last_error()
    assert call(labels=None, labelled=None) == _lib.SSAL_EINVAL
    # the raw triple comes whole or not at all
    for given in range(1, 7):
        raw = [p if given >> j & 1 else None for j in range(3)]
        assert call(raw=raw) == _lib.SSAL_EINVAL and b"given together" in L.ssal_last_error(), raw
    assert call(ws_bytes=ws(1, 1, 1, k, 0) - 512) == _lib.SSAL_ENOMEM and b"workspace too small" in L.ssal_last_error()
    # a raw side needs the target plane too: a batch of 8 x 1024 x 2048 at the size of the call without one
    assert call(raw=[p] * 3, n=8, h=32, w=64, ws_bytes=ws(8, 32, 64, k, 0)) == _lib.SSAL_ENOMEM
    # the images entry needs a committed handle
    images = L.ssal_icnet_train_highres_semi_nhwc
    hd = ctypes.c_void_p()
    _lib.check(L.ssal_icnet_create(3, k, ctypes.byref(hd)))
    rest = (0, 1, 64, 64, p, p, p, 0, 0.5, p, 0.0, 0.0, p, 0, p, p, None, None, p, big, None)
    assert images(hd, p, None, *rest) == _lib.SSAL_ESTATE
    assert images(None, p, None, *rest) == _lib.SSAL_EINVAL
    _lib.check(L.ssal_icnet_destroy(hd))


def _inputs(u8=False):
    """host stand-ins of (features with the frames, labels, mask) and (images, labels, mask) for a batch of two"""
    img = np.zeros((2, 32, 64, 3), np.uint8 if u8 else np.float32)
    feats = (np.zeros((2, 1, 2, 256), np.float32), np.zeros((2, 2, 4, 256), np.float32), img)
    lab, msk = np.zeros((2, 32, 64), np.uint8), np.ones((2, 32, 64), np.float32)
    return feats, lab, msk, (img, lab, msk)


def test_keyword_validation_before_any_device_work(monkeypatch):
    def no_gpu():
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    net = _icnet()
    tr = SEMI(net, 1e-3)
    feats, lab, msk, images = _inputs()
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
    # features_raw: the whole triple, every member shaped and typed like its counterpart
    u8 = np.zeros((2, 32, 64, 3), np.uint8)
    for call in (tr.gradient_features, tr.step_features):
        for raw in (feats[:-1], feats[0], feats[:-1] + (None,), (None,) + feats[1:], feats + feats[:1]):
            with pytest.raises(ValueError, match="whole or not at all"):
                call(*feats, lab, msk, labelled=np.array([0, 1]), features_raw=raw)
        for j in range(3):
            bad = tuple(t[:, :, :1] if i == j else t for i, t in enumerate(feats))
            with pytest.raises(ValueError, match="counterpart"):
                call(*feats, lab, msk, labelled=np.array([0, 1]), features_raw=bad)
        with pytest.raises(ValueError, match="dtype of images"):
            call(*feats, lab, msk, labelled=np.array([0, 1]), features_raw=feats[:2] + (u8,))
        with pytest.raises(ValueError, match="dtype of images"):
            call(*feats[:2], u8, lab, msk, labelled=np.array([0, 1]), features_raw=feats)
        with pytest.raises(ValueError, match="floating-point"):
            call(*feats, lab, msk, labelled=np.array([0, 1]), features_raw=(feats[0].astype(np.int32),) + feats[1:])
        with pytest.raises(ValueError):  # the inputs themselves are still judged as the parent judges them
            call(*(feats[:-1] + (feats[-1][:, :1],)), lab, msk, labelled=np.array([0, 1]))
    with pytest.raises(NotImplementedError):
        SEMI(net, 1e-3, measure="bald")
    enet = ssal.ENet(19)
    enet.build((None, None, None, 3))
    with pytest.raises(NotImplementedError):
        SEMI(enet, 1e-3)
    with pytest.raises(ValueError, match="3 or 4 input channels"):
        one = np.zeros((2, 32, 64, 1), np.float32)
        SEMI(_icnet(c_in=1), 1e-3).gradient_features(feats[0], feats[1], one, lab, msk, labelled=np.array([0, 1]))


def test_from_params_active_learning_section():
    net = _icnet()
    tr = SEMI.from_params(net, {"hyperparams": HYPER, "active_learning": {"measure": "margin", "threshold": 0.25}})
    assert (tr.measure, tr.threshold) == ("margin", 0.25)
    assert (tr.learning_rate, tr.beta1, tr.beta2, tr.l2, tr.weight) == (0.0005, 0.9, 0.99, 0.0002, 1.02)
    tr = SEMI.from_params(net, {"hyperparams": HYPER})
    assert (tr.measure, tr.threshold) == ("entropy", 0.0)
    assert tr._semi(2, None, None, np.array([0, 0]), None, None, None, False)[1:] == (_lib.MEASURES["entropy"], 0.0)
    tr = SEMI(net, 1e-3, measure="confidence", threshold=0.75)
    assert tr._semi(2, None, None, np.array([0, 0]), None, None, None, False)[1:] == (_lib.MEASURES["confidence"], 0.75)
    assert tr._semi(2, None, None, np.array([0, 0]), "margin", 0.5, None, False)[1:] == (_lib.MEASURES["margin"], 0.5)
    with pytest.raises(NotImplementedError):
        SEMI.from_params(net, {"hyperparams": dict(HYPER, softmax={"multiscale": True})})
    with pytest.raises(NotImplementedError):
        SEMI.from_params(net, {"hyperparams": dict(HYPER, weight_reg={"glorot_scaling": True})})


def test_state_round_trip_with_the_plain_trainer():
    net = _icnet(6)
    plain, semi = ICNetHighResTrainer(net, 1e-3), SEMI(net, 1e-3)
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
        assert list(back[key]) == plain.variable_names and len(back[key]) == 23
        for name in st[key]:
            assert np.array_equal(back[key][name], st[key][name]) and np.array_equal(again[key][name], st[key][name])
    assert semi.variable_names == plain.variable_names and semi._adam_ranges() == plain._adam_ranges()
    assert float(semi._b1p) == float(plain._b1p) and float(semi._b2p) == float(plain._b2p)


def test_the_plain_trainer_still_refuses(monkeypatch):
    def no_gpu():
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    tr = ICNetHighResTrainer(_icnet(), 1e-3)
    feats, lab, msk, images = _inputs()
    for kw in ({"labelled": np.array([1, 1])}, {"confusion": np.zeros((19, 19), np.int64)}, {"return_pseudo_pixels": True}):
        with pytest.raises(NotImplementedError, match="not implemented for ICNet's high-resolution trainer"):
            tr.gradient_features(*feats, lab, msk, **kw)
        with pytest.raises(NotImplementedError):
            tr.step_features(*feats, lab, msk, **kw)
        with pytest.raises(NotImplementedError):
            tr.step(*images, **kw)
    for kw in ({"measure": "margin"}, {"threshold": 0.5}, {"features_raw": feats}):
        with pytest.raises(TypeError):
            tr.gradient_features(*feats, lab, msk, **kw)
    assert ICNetHighResTrainer._C_FEATURES[1] is None and ICNetHighResTrainer._C_IMAGES[1] is None


# ---- the raw side's route -------------------------------------------------------------------------------------------------------
def _expected_route(c_in, n, h32, w32, ic_front, mfma=True):
    """launch_icnet_highres_targets' predicate restated: bit 0 of the knob on the matrix-core family, and launch_front2's own
    guards (tests/icnet_limits.py) on the frames [n, 32 h32, 32 w32, c_in]"""
    return "fused" if mfma and ic_front & 1 and lim.front2_fits(n, 32 * h32, 32 * w32, c_in, 1, 2) else "unfused"


ROUTE_SHAPES = [(1, 1, 1), (1, 3, 5), (2, 2, 3), (8, 32, 64), (1, 1, 131071), (1, 131071, 1), (1, 362, 362), (131071, 1, 1),
                (31, 64, 64), (1, 256, 511)]


@pytest.fixture
def shipped_knobs():
    knobs = _lib.get_knobs()
    yield knobs
    _lib.set_knob("ic_front", knobs["ic_front"])
    _lib.set_kernel_family(bool(knobs["kernel_family"]))


def test_raw_side_route(shipped_knobs):
    """the fused front wherever the entries admit the shape and bit 0 of ic_front is set; the separate launches under a cleared
    bit or the generic kernel family.  Of the two bounds the entries' own (n h w < 2^27 frame pixels) is the tighter one:
    launch_front2 refuses H W c_in 4 >= 2^31 or 2^31 tiles, which no admitted shape reaches, so the guard alone never sends a
    call to the separate launches -- the predicate restates it all the same."""
    assert shipped_knobs["ic_front"] & 1, "the shipped setting fuses the high-resolution front"
    for c_in in (3, 4):
        for n, h, w in ROUTE_SHAPES:
            assert n * h * w < 131072
            assert lim.front2_fits(n, 32 * h, 32 * w, c_in, 1, 2), (n, h, w)  # the tighter bound is the entries'
            for front in (3, 1, 2, 0):
                _lib.set_knob("ic_front", front)
                assert _lib.icnet_highres_raw_route(c_in, n, h, w) == _expected_route(c_in, n, h, w, front), (c_in, n, h, w, front)
            _lib.set_knob("ic_front", shipped_knobs["ic_front"])
            assert _lib.icnet_highres_raw_route(c_in, n, h, w) == "fused"
    # beyond the entries' limit the query refuses as they do, whatever launch_front2 would say
    for n, h, w in ((1, 1, 131072), (8, 128, 128), (131072, 1, 1)):
        with pytest.raises(ValueError, match="beyond"):
            _lib.icnet_highres_raw_route(3, n, h, w)
    assert (2 ** 27 - 1024) * 4 * 4 < 2 ** 31  # the largest admitted frame of four float channels, in launch_front2's bytes
    for c_in in (1, 2, 5):
        with pytest.raises(ValueError, match="3 or 4 input channels"):
            _lib.icnet_highres_raw_route(c_in, 1, 1, 1)
    _lib.set_kernel_family(False)
    assert _lib.icnet_highres_raw_route(3, 2, 2, 3) == "unfused"
    _lib.set_kernel_family(True)
    assert _lib.icnet_highres_raw_route(3, 2, 2, 3) == "fused"
