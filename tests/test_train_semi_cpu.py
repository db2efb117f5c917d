"""The semi-supervised output-layer step without a GPU: the new C entry points and their ctypes
signatures, the host-only workspace query and its limits, the statuses the entries give before they touch a device, and the
keyword validation of FinalLayerTrainer."""
import ctypes

import numpy as np
import pytest

import semanticsegmentationactivelearning_amd as ssal
from semanticsegmentationactivelearning_amd import _lib
from semanticsegmentationactivelearning_amd.training import FinalLayerTrainer

_vp, _i, _i64, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float

# include/ssal_enet.h, argument by argument
SIGNATURES = {
    "ssal_final_grad_semi_workspace_bytes": (_i64, [_i, _i, _i, _i]),
    # features, features_raw, n, h, w, classes, kernel, labels, mask, labelled, measure, threshold, weight, label_smoothing,
    # loss, grad, confusion, pseudo_pixels, ws, ws_bytes, stream
    "ssal_final_grad_semi_nhwc": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _f, _f, _f, _vp, _vp, _vp, _vp, _vp,
                                       _i64, _vp]),
    "ssal_enet_train_final_semi_workspace_bytes": (_i64, [_vp, _i, _i, _i, _i]),
    # net, x, x_raw, x_is_u8, n, h, w, labels, mask, labelled, measure, threshold, kernel, weight, label_smoothing, loss,
    # grad, confusion, pseudo_pixels, ws, ws_bytes, stream
    "ssal_enet_train_final_semi_nhwc": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _f, _vp, _f, _f, _vp, _vp,
                                             _vp, _vp, _vp, _i64, _vp]),
}


def test_new_symbols_exist_with_declared_signatures():
    L = _lib.lib()
    for name, (res, args) in SIGNATURES.items():
        assert name in _lib.PROTOTYPES, "%s is not declared in _lib.PROTOTYPES" % name
        assert _lib.PROTOTYPES[name] == (res, args), name
        fn = getattr(L, name)  # AttributeError if the library does not export it
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_semi_workspace_is_host_only_and_keeps_the_limits():
    L = _lib.lib()
    ws, plain = L.ssal_final_grad_semi_workspace_bytes, L.ssal_final_grad_workspace_bytes
    for n, h, w, k in ((1, 33, 65, 2), (3, 20, 17, 19), (8, 512, 1024, 19), (1, 64, 64, 32)):
        # the gradient's partials plus the confusion replicas
        assert ws(n, h, w, k) >= plain(n, h, w, k) > 0
    # the boundaries of final_grad_fits, as tests/test_train_final_cpu.py states them
    assert ws(1, (1 << 30) - 1, 1, 19) > 0
    assert ws(1, 1 << 30, 1, 19) == -1
    assert ws(1, 1, (1 << 30) - 1, 19) > 0
    assert ws(1, 1, 1 << 30, 19) == -1
    assert ws(1, 16 * 46340, 16 * 46340, 19) > 0
    assert ws(1, 16 * 46341, 16 * 46341, 19) == -1
    assert ws(1, 64, 64, 1) == -1 and ws(1, 64, 64, 33) == -1 and ws(1, 64, 64, 2) > 0 and ws(1, 64, 64, 32) > 0
    assert ws(0, 64, 64, 19) == -1 and ws(1, 0, 64, 19) == -1 and ws(1, 64, -1, 19) == -1
    # the image form needs a committed handle (its with_raw difference is checked on the GPU): none -> -1
    assert L.ssal_enet_train_final_semi_workspace_bytes(None, 1, 64, 64, 0) == -1
    assert L.ssal_enet_train_final_semi_workspace_bytes(None, 1, 64, 64, 1) == -1


def test_semi_entry_validates_without_a_gpu():
    L = _lib.lib()
    p = ctypes.c_void_p(16)

    def call(classes=19, h=8, measure=0, labels=p, labelled=p, ws_bytes=1 << 30, features=p):
        return L.ssal_final_grad_semi_nhwc(features, None, 1, h, 8, classes, p, labels, labels, labelled, measure, 0.5, 0.0,
                                           0.0, p, p, None, None, p, ws_bytes, None)

    assert call(classes=33) == _lib.SSAL_EINVAL and call(classes=1) == _lib.SSAL_EINVAL
    assert call(h=1 << 30) == _lib.SSAL_EINVAL
    assert call(h=0) == _lib.SSAL_EINVAL
    assert call(measure=3) == _lib.SSAL_ENOTIMPL
    assert b"Uncertainty function not implemented" in L.ssal_last_error()
    assert call(measure=-1) == _lib.SSAL_ENOTIMPL
    assert call(labels=None, labelled=None) == _lib.SSAL_EINVAL  # all labelled, but no planes
    assert call(features=None) == _lib.SSAL_EINVAL
    assert call(ws_bytes=64) == _lib.SSAL_ENOMEM
    assert b"workspace too small" in L.ssal_last_error()
    assert L.ssal_enet_train_final_semi_nhwc(None, p, None, 0, 1, 64, 64, p, p, p, 0, 0.5, p, 0.0, 0.0, p, p, None, None, p,
                                             1 << 30, None) == _lib.SSAL_EINVAL  # no handle


AL_PARAMS = {
    "active_learning": {"measure": "margin", "selection_size": 50, "threshold": 0.9},
    "hyperparams": {"learning_rate": 0.0005, "learning_rate_decay": 0.0,
                    "optimizer": {"type": "Adam", "kwargs": {"beta1": 0.9, "beta2": 0.99}},
                    "weight_reg": {"L2": 0.0002, "L1": 0.0},
                    "softmax": {"label_smoothing": 0.0, "loginverse_scaling": 1.02, "multiscale": False}}}


def _net(k=19):
    net = ssal.ENet(k)
    net.build((None, None, None, 3))
    return net


def test_from_params_reads_measure_and_threshold():
    tr = FinalLayerTrainer.from_params(_net(), AL_PARAMS)
    assert (tr.measure, tr.threshold) == ("margin", 0.9)
    tr = FinalLayerTrainer.from_params(_net(), AL_PARAMS["hyperparams"])  # the section alone: the defaults
    assert (tr.measure, tr.threshold) == ("entropy", 0.0)
    tr = FinalLayerTrainer(_net(), 1e-3)
    assert (tr.measure, tr.threshold) == ("entropy", 0.0)
    bad = dict(AL_PARAMS, active_learning={"measure": "bald", "threshold": 0.5})
    with pytest.raises(NotImplementedError, match="Uncertainty function not implemented."):
        FinalLayerTrainer.from_params(_net(), bad)


@pytest.mark.parametrize("method,lead", [("gradient_features", (2, 4, 4, 16)), ("step_features", (2, 4, 4, 16)),
                                         ("step", (2, 8, 8, 3))])
def test_keyword_validation_needs_no_device(method, lead):
    """an unknown measure, a `labelled` of the wrong length, a malformed `confusion` and missing planes are refused on the
    host, before any device work"""
    tr = FinalLayerTrainer(_net(), 1e-3)
    call = getattr(tr, method)
    x = np.zeros(lead, np.float32)
    lab = np.zeros((2, 8, 8), np.uint8)
    msk = np.ones((2, 8, 8), np.float32)
    with pytest.raises(NotImplementedError, match="Uncertainty function not implemented."):
        call(x, lab, msk, labelled=[1, 0], measure="bald")
    with pytest.raises(ValueError, match="labelled"):
        call(x, lab, msk, labelled=[1, 0, 1])
    with pytest.raises(ValueError, match="labelled"):
        call(x, lab, msk, labelled=np.ones((2, 1), np.uint8))
    with pytest.raises(ValueError, match="confusion"):
        call(x, lab, msk, confusion=np.zeros((19, 19), np.int32))
    with pytest.raises(ValueError, match="confusion"):
        call(x, lab, msk, confusion=np.zeros((18, 19), np.int64))
    with pytest.raises(ValueError, match="labels / mask may be None only"):
        call(x, None, None, labelled=[0, 1])
    with pytest.raises(ValueError, match="labels / mask may be None only"):
        call(x, None, None)
