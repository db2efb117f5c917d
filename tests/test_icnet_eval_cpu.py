"""ICNet's fused validation pass without a GPU: the two C-ABI symbols and their signatures, the
workspace query's refusals, and the refusals of ``ICNet.evaluate`` that shapes and dtypes decide -- raised on the host,
before any device work."""
import ctypes
import re
import os

import numpy as np
import pytest
import torch

import semanticsegmentationactivelearning_amd as ssal
from semanticsegmentationactivelearning_amd import _lib

_vp, _i, _i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_exist_with_the_documented_signatures():
    want = {
        "ssal_icnet_eval_workspace_bytes": (_i64, [_vp, _i, _i, _i]),
        # handle, x, x_is_u8, n, h, w, labels, mask, confusion, ws, ws_bytes, stream
        "ssal_icnet_evaluate_nhwc": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i64, _vp]),
    }
    L = _lib.lib()
    for name, proto in want.items():
        assert _lib.PROTOTYPES[name] == proto, name
        fn = getattr(L, name)  # AttributeError if the library does not export it
        assert fn.restype is proto[0] and list(fn.argtypes) == proto[1], name
    # ssal_enet_evaluate_nhwc_arith without the arithmetic argument
    enet = _lib.PROTOTYPES["ssal_enet_evaluate_nhwc_arith"][1]
    assert want["ssal_icnet_evaluate_nhwc"][1] == enet[:6] + enet[7:]
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "ssal_icnet.h")).read())
    assert "int64_t ssal_icnet_eval_workspace_bytes(const ssal_icnet *net, int n, int h, int w);" in header
    assert ("int ssal_icnet_evaluate_nhwc(ssal_icnet *net, const void *x_dev, int x_is_u8, int n, int h, int w, "
            "const uint8_t *labels_dev, const uint8_t *mask_dev, int64_t *confusion_dev, void *ws_dev, "
            "int64_t ws_bytes, void *stream);") in header


def test_workspace_query_refuses_bad_handles_dims_and_class_counts():
    L = _lib.lib()
    assert L.ssal_icnet_eval_workspace_bytes(None, 1, 64, 64) == -1
    h = _vp()
    for k in (1, 33, 0, -4):  # no handle exists for a class count outside [2, 32]: nothing to size
        assert L.ssal_icnet_create(3, k, ctypes.byref(h)) == _lib.SSAL_EINVAL
        assert L.ssal_icnet_eval_workspace_bytes(h, 1, 64, 64) == -1
    assert L.ssal_icnet_create(3, 19, ctypes.byref(h)) == _lib.SSAL_OK
    try:
        # committing uploads the weights (device work), so without a GPU the handle stays uncommitted: -1 for every size
        for n, hh, ww in ((1, 64, 64), (0, 64, 64), (1, 0, 64), (1, 64, -32), (1, 48, 64), (1, 64, 16)):
            assert L.ssal_icnet_eval_workspace_bytes(h, n, hh, ww) == -1, (n, hh, ww)
        # the entry refuses the same handle before it looks at a pointer
        assert L.ssal_icnet_evaluate_nhwc(h, None, 0, 1, 64, 64, None, None, None, None, 0, None) == _lib.SSAL_ESTATE
        assert L.ssal_icnet_evaluate_nhwc(None, None, 0, 1, 64, 64, None, None, None, None, 0, None) == _lib.SSAL_EINVAL
    finally:
        L.ssal_icnet_destroy(h)


def test_evaluate_shape_and_dtype_errors_are_raised_without_touching_the_gpu(monkeypatch):
    """a bad call never reaches the device: the checks run before the first thing that needs one"""
    def never(*a, **kw):
        raise AssertionError("the device was asked for")

    monkeypatch.setattr(_lib, "require_gpu", never)
    monkeypatch.setattr(_lib, "as_device_image", never)
    net = ssal.ICNet(19)
    net.build((None, None, None, 3))
    x = np.zeros((2, 64, 96, 3), np.float32)
    lab = np.zeros((2, 64, 96), np.uint8)
    with pytest.raises(ValueError, match="rank-4"):
        net.evaluate(x[0], lab[0])
    with pytest.raises(ValueError, match="divisible by 32"):
        net.evaluate(x[:, :40], lab[:, :40])
    with pytest.raises(ValueError, match="built for 3 input channels"):
        net.evaluate(np.zeros((2, 64, 96, 4), np.float32), lab)
    with pytest.raises(ValueError, match=r"labels must have shape \(2, 64, 96\)"):
        net.evaluate(x, lab[:, :, :-1])
    with pytest.raises(ValueError, match=r"mask must have shape \(2, 64, 96\)"):
        net.evaluate(x, lab, mask=lab[:1])
    with pytest.raises(ValueError, match=r"confusion must be a contiguous int64 \[19, 19\]"):
        net.evaluate(x, lab, confusion=torch.zeros((6, 6), dtype=torch.int64))
    with pytest.raises(ValueError, match=r"confusion must be a contiguous int64 \[19, 19\]"):
        net.evaluate(x, lab, confusion=torch.zeros((19, 19), dtype=torch.int32))
    with pytest.raises(ValueError, match=r"confusion must be a contiguous int64 \[19, 19\]"):
        net.evaluate(x, lab, confusion=np.zeros((19, 19), np.int64))
    # a well-formed call gets past the checks and only then asks for the device
    with pytest.raises(AssertionError, match="the device was asked for"):
        net.evaluate(x, lab, mask=lab, confusion=torch.zeros((19, 19), dtype=torch.int64))
    assert hasattr(net, "_evaluate_composed")
    assert "not implemented" not in ssal.ICNet.evaluate.__doc__
