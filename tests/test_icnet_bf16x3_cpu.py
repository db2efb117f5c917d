"""CPU side of ICNet's opt-in bf16x3 mode: the new C ABI symbols and every status they reach without a
device, the dry dispatch query over every convolution of ICNet, the host packer against the numpy layout (a stand-alone C++
program, also built with the host sanitizers), and the TEETH of the model tests/icnet_split_model.py -- the GPU gate
(tests/test_gpu_icnet_bf16x3.py: |kernel - value| <= bound) is worth what these assertions prove about value and bound."""
import ctypes
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import icnet_split_model as ism
import split_operand_model as som
import semanticsegmentationactivelearning_amd as ssal
from oracle import enet_oracle as orc
from semanticsegmentationactivelearning_amd import _lib, inference as inf

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "semanticsegmentationactivelearning_amd", "csrc")
F32, BF16X3, UNKNOWN = 0, 1, 7


# ---- symbols and statuses ----------------------------------------------------------------------------------------------------
def test_symbols_and_signatures():
    L = _lib.lib()
    i, vp, i64, f = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_float
    assert L.ssal_icnet_forward_nhwc_arith.argtypes == [vp, vp, i, i, i, i, i, vp, vp, i64, vp]
    assert L.ssal_icnet_score_nhwc_arith.argtypes == [vp, vp, i, i, i, i, i, f, i, vp, vp, vp, vp, vp, i64, vp]
    assert L.ssal_conv_bn_act_arith.argtypes == L.ssal_conv_bn_act.argtypes + [i]
    assert L.ssal_conv_bn_workspace_bytes_arith.argtypes == [i, i, i, i, i] and L.ssal_conv_bn_workspace_bytes_arith.restype == i64
    assert len(L.ssal_icnet_debug_conv_dispatch.argtypes) == 14
    for fn in (L.ssal_icnet_forward_nhwc_arith, L.ssal_icnet_score_nhwc_arith, L.ssal_conv_bn_act_arith,
               L.ssal_icnet_debug_conv_dispatch):
        assert fn.restype == i


def test_unknown_mode_is_einval_before_anything_else():
    """judged first: with every other argument NULL / zero the status is still the mode's"""
    L = _lib.lib()
    assert L.ssal_icnet_forward_nhwc_arith(None, None, 0, 0, 0, 0, UNKNOWN, None, None, 0, None) == _lib.SSAL_EINVAL
    assert b"arithmetic" in L.ssal_last_error()
    assert L.ssal_icnet_score_nhwc_arith(None, None, 0, 0, 0, 0, 9, 0.0, UNKNOWN, None, None, None, None, None, 0, None) == _lib.SSAL_EINVAL
    assert L.ssal_conv_bn_act_arith(None, 0, 0, 0, 0, None, 0, 0, 0, 0, 0, None, None, None, None, None, None, 0, 0, None, None, 0,
                                    None, UNKNOWN) == _lib.SSAL_EINVAL
    assert L.ssal_conv_bn_workspace_bytes_arith(1, 1, 32, 32, UNKNOWN) == -1
    k, nt = ctypes.c_int(), ctypes.c_int()
    assert L.ssal_icnet_debug_conv_dispatch(1, 8, 8, 32, 32, 1, 1, 1, 1, 0, 0, UNKNOWN, ctypes.byref(k), ctypes.byref(nt)) == _lib.SSAL_EINVAL


@pytest.mark.parametrize("arith", [F32, BF16X3])
def test_statuses_of_the_known_modes_without_a_device(arith):
    L = _lib.lib()
    # a NULL handle: the plain entries' own status
    assert L.ssal_icnet_forward_nhwc_arith(None, None, 0, 1, 32, 32, arith, None, None, 0, None) == _lib.SSAL_EINVAL
    assert L.ssal_icnet_score_nhwc_arith(None, None, 0, 1, 32, 32, 1, 0.0, arith, None, None, None, None, None, 0, None) == _lib.SSAL_EINVAL
    # an uncommitted handle: SSAL_ESTATE, as for ssal_icnet_forward_nhwc
    h = ctypes.c_void_p()
    assert L.ssal_icnet_create(3, 19, ctypes.byref(h)) == _lib.SSAL_OK
    try:
        assert L.ssal_icnet_forward_nhwc_arith(h, None, 0, 1, 32, 32, arith, None, None, 0, None) == _lib.SSAL_ESTATE
        assert L.ssal_icnet_score_nhwc_arith(h, None, 0, 1, 32, 32, 1, 0.0, arith, None, None, None, None, None, 0, None) == _lib.SSAL_ESTATE
    finally:
        L.ssal_icnet_destroy(h)
    # the operator hook: NULL pointers, then dims
    assert L.ssal_conv_bn_act_arith(None, 1, 8, 8, 32, None, 1, 1, 32, 1, 1, None, None, None, None, None, None, 0, 0, None, None, 0,
                                    None, arith) == _lib.SSAL_EINVAL
    k, nt = ctypes.c_int(), ctypes.c_int()
    assert L.ssal_icnet_debug_conv_dispatch(1, 8, 8, 32, 32, 1, 1, 1, 1, 0, 0, arith, None, ctypes.byref(nt)) == _lib.SSAL_EINVAL
    assert L.ssal_icnet_debug_conv_dispatch(0, 8, 8, 32, 32, 1, 1, 1, 1, 0, 0, arith, ctypes.byref(k), ctypes.byref(nt)) == _lib.SSAL_EINVAL
    assert L.ssal_icnet_debug_conv_dispatch(1, 8, 8, 32, 32, 9, 9, 1, 1, 0, 0, arith, ctypes.byref(k), ctypes.byref(nt)) == _lib.SSAL_EINVAL
    assert L.ssal_icnet_debug_conv_dispatch(1, 8, 8, 5, 32, 3, 3, 2, 1, 0, 0, arith, ctypes.byref(k), ctypes.byref(nt)) == _lib.SSAL_EINVAL


def test_workspace_sizes():
    """the exact mode's size is the plain query's; the mode adds the pre-split kernel: 1.5x the bytes of the padded fp32 kernel"""
    L = _lib.lib()
    for kh, cin, cout in ((1, 32, 32), (3, 64, 19), (3, 96, 160), (3, 3, 32)):
        base = L.ssal_conv_bn_workspace_bytes(kh, kh, cin, cout)
        assert L.ssal_conv_bn_workspace_bytes_arith(kh, kh, cin, cout, F32) == base
        extra = L.ssal_conv_bn_workspace_bytes_arith(kh, kh, cin, cout, BF16X3) - base
        if cin % 32:
            assert extra == 0
        else:
            assert extra == 6 * kh * kh * cin * (-(-cout // 32) * 32) + 256


def test_python_keyword_is_validated_like_enets():
    net = ssal.ICNet(19)
    x = np.zeros((1, 32, 32, 3), np.float32)
    with pytest.raises(ValueError, match=r"arithmetic must be one of \['bf16x3', 'f32'\]"):
        net(x, arithmetic="fp16")
    with pytest.raises(ValueError, match="arithmetic must be one of"):
        net.score(x, arithmetic="tf32")
    with pytest.raises(ValueError, match="arithmetic must be one of"):
        inf.predict(net, x, arithmetic="bf16")
    import inspect
    assert inspect.signature(net.score).parameters["arithmetic"].default == "f32"
    assert inspect.signature(net.__call__).parameters["arithmetic"].default == "f32"
    for fn in (net.score_regions, net.evaluate):
        assert "arithmetic" not in inspect.signature(fn).parameters


# ---- dispatch ------------------------------------------------------------------------------------------------------------------
EXACT_IN_THE_MODE = {"conv1_1_3x3_s2", "conv1_sub1",                        # k_conv_first
                     "conv1_2_3x3", "conv1_3_3x3", "conv2_1_3x3", "conv2_2_3x3", "conv2_3_3x3",  # k_conv3x3_c32
                     "conv_sub4", "conv_sub2",                              # the up-sampling forms
                     "conv6_cls"}                                           # k_conv1x1_up2_c128


@pytest.mark.parametrize("n,h,w", [(8, 1024, 2048), (2, 64, 128)])
def test_dispatch_over_every_convolution(n, h, w):
    convs = ism.icnet_convs()
    assert len(convs) == 3 + 3 * 16 + 5 + 8 and len({c["name"] for c in convs}) == len(convs)
    split = set()
    for c in convs:
        args = (n, h // c["div"], w // c["div"], c["cin"], c["cout"], c["k"], c["stride"], c["dil"], c["up2"], c["res"] is not None)
        exact = _lib.icnet_conv_dispatch(*args, arithmetic="f32")
        assert exact == ism.expected_dispatch(*args, arithmetic="f32"), c["name"]  # the launcher's rule before this mode existed
        assert exact[0] != "k_igemm_bf16x3"
        mode = _lib.icnet_conv_dispatch(*args, arithmetic="bf16x3")
        assert mode == ism.expected_dispatch(*args, arithmetic="bf16x3"), c["name"]
        if exact[0] == "k_igemm":  # exactly the plain implicit GEMM moves, at the same NT
            assert mode == ("k_igemm_bf16x3", exact[1]) and exact[1] in (1, 2, 4), c["name"]
            split.add(c["name"])
        else:
            assert mode == exact, c["name"]
    assert split == {c["name"] for c in convs} - EXACT_IN_THE_MODE
    if n == 8:  # NT as the ranking pass sees it
        nts = {c["name"]: _lib.icnet_conv_dispatch(n, h // c["div"], w // c["div"], c["cin"], c["cout"], c["k"], c["stride"], c["dil"],
                                                   c["up2"], c["res"] is not None, "bf16x3")[1] for c in convs}
        assert nts["conv2_1_1x1_reduce"] == 1 and nts["conv3_1_3x3"] == 2 and nts["conv4_1_1x1_increase"] == 4
        assert nts["conv5_4_k1"] == 2 and nts["conv3_sub1"] == 2 and nts["conv2_sub1"] == 1
    else:   # small maps never leave NT = 1
        assert {_lib.icnet_conv_dispatch(n, h // c["div"], w // c["div"], c["cin"], c["cout"], c["k"], c["stride"], c["dil"],
                                         c["up2"], c["res"] is not None, "bf16x3")[1] for c in convs if c["name"] in split} == {1}


def test_dispatch_of_the_gpu_test_shapes():
    """the NT = 2 / 4 shapes of tests/test_gpu_icnet_bf16x3.py and the shape that must stay exact"""
    assert _lib.icnet_conv_dispatch(1, 255, 258, 64, 64, 1, arithmetic="bf16x3") == ("k_igemm_bf16x3", 2)
    assert _lib.icnet_conv_dispatch(1, 255, 258, 64, 128, 1, arithmetic="bf16x3") == ("k_igemm_bf16x3", 4)
    assert _lib.icnet_conv_dispatch(1, 255, 258, 32, 64, 3, dilation=2, arithmetic="bf16x3") == ("k_igemm_bf16x3", 2)
    assert _lib.icnet_conv_dispatch(1, 255, 258, 32, 128, 3, dilation=2, arithmetic="bf16x3") == ("k_igemm_bf16x3", 4)
    assert _lib.icnet_conv_dispatch(1, 9, 15, 32, 160, 1, arithmetic="bf16x3") == ("k_igemm_bf16x3", 1)
    assert _lib.icnet_conv_dispatch(1, 9, 15, 32, 32, 3, arithmetic="bf16x3") == ("k_conv3x3_c32", 0)


# ---- the host packer -------------------------------------------------------------------------------------------------------------
def _build_packer(tmp_path, flags, name):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler builds the oracle's C code and this probe alike"
    exe = str(tmp_path / name)
    subprocess.check_call([cxx, "-O1", "-g"] + flags + ["-I", CSRC, os.path.join(HERE, "icnet_split_pack.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_host_pack_is_the_numpy_layout_unit_for_unit(tmp_path, flags):
    exe = _build_packer(tmp_path, flags, "icnet_split_pack")
    rng = np.random.default_rng(3)
    for kh, cin, cout in ((1, 32, 32), (3, 32, 19), (2, 48, 70)):  # padded columns; Cin / 16 odd; a non-square tap count
        k = (rng.normal(size=(kh, kh, cin, cout)) * np.exp2(rng.integers(-20, 20, (kh, kh, cin, cout)))).astype(np.float32)
        k.flat[::7] = 0.0
        k.tofile(str(tmp_path / "k.bin"))
        subprocess.check_call([exe, str(kh), str(kh), str(cin), str(cout), str(tmp_path / "k.bin"), str(tmp_path / "p.bin")])
        got = np.fromfile(str(tmp_path / "p.bin"), dtype=np.uint32)
        want = ism.pack_layout(k)
        assert got.size == want.size == kh * kh * (cin // 16) * -(-cout // 32) * 192 * 4
        assert np.array_equal(got, want.ravel()), (kh, cin, cout)
        assert not want[:, :, -1, :, [j + 32 * h for h in (0, 1) for j in range(cout % 32 or 32, 32)]].any()  # padded columns: zeros


# ---- the model: agreement with float64, and teeth ----------------------------------------------------------------------------------
def test_model_agrees_with_float64_within_its_anchor():
    rng = np.random.default_rng(5)
    x = rng.normal(size=(2, 5, 7, 64)).astype(np.float32)
    k = (rng.normal(size=(3, 3, 64, 19)) / 24).astype(np.float32)
    bias = rng.normal(size=19).astype(np.float32)
    res = rng.normal(size=(2, 3, 4, 19)).astype(np.float32)
    extra = {}
    v, b = ism.conv(x, k, stride=2, dil=2, bias=bias, res=res, relu=True, extra=extra)
    want = ism.exact64(x, k, stride=2, dil=2, bias=bias, res=res, relu=True)
    assert v.shape == want.shape == (2, 3, 4, 19) and (b > 0).all()
    assert (np.abs(v - want) <= extra["anchor"]).all()
    # the geometry is the oracle's (TF SAME, stride and dilation): the exact fp32 convolution lies within the same anchor
    y32 = orc.conv2d_same(x, k, stride=2, dil=2)
    y64 = ism.exact64(x, k, stride=2, dil=2)
    assert np.abs(y32 - y64).max() < 1e-5


@pytest.mark.parametrize("k,cin,cout,step", ism.LIVE_CASES, ids=lambda v: str(v))
def test_live_cases_have_teeth(k, cin, cout, step):
    """removing any one of the six products in the dense step moves the model by more than 2 x bound on at least half of the
    outputs that step reaches (section 5.4.1's condition: a kernel that loses the product cannot pass the GPU gate)"""
    x, w = ism.live_case(k, cin, cout, step)
    assert (x > 0).all() and (w >= 0).all()
    for t in som.split3(x)[1:] + som.split3(w.reshape(-1, cout)[16 * step:16 * step + 16])[1:]:
        assert (t > 0).all()  # large second and third terms everywhere in the dense step
    bn = ism.identity_bn(cout)
    v, b = ism.conv(x, w, bn=bn)
    w0 = w.reshape(-1, cout).copy()
    w0[16 * step:16 * step + 16] = 0
    reached = ism.conv(x, w0.reshape(w.shape), bn=bn)[0] != v
    assert reached.sum() >= 0.3 * v.size  # the tap of the step is inside the image for these outputs
    for ij in som.SIX:
        moved = np.abs(ism.conv(x, w, bn=bn, drop=ij, at=step)[0].astype(np.float64) - v) > 2 * b
        assert moved[reached].mean() >= 0.5, (ij, moved[reached].mean())
        assert not moved[~reached].any()


@pytest.mark.parametrize("k,cin,cout", ism.EXACT_CASES, ids=lambda v: str(v))
def test_exact_cases_are_exact_and_differ_from_fp32_where_predicted(k, cin, cout):
    x, w = ism.exact_case(k, cin, cout)
    bn = ism.identity_bn(cout)
    v, b = ism.conv(x, w, bn=bn)
    assert not b.any()  # the kernel must give these bits
    # all 64 subsets of the six products of one element pair are fp32 numbers: no order of summation can round
    xt = [t.astype(np.float64) for t in som.split3(x)]
    wt = [t.astype(np.float64) for t in som.split3(np.float32(ism.FAMILY))]
    prods = [xt[i - 1] * wt[j - 1] for i, j in som.SIX]
    for mask in range(64):
        s = sum(p for bit, p in enumerate(prods) if mask >> bit & 1) + np.zeros(x.shape)
        assert np.array_equal(s.astype(np.float32).astype(np.float64), s)
    # the value is the six-product sum, one ulp below the correctly rounded fp32 product, wherever a selector reaches the image
    col, _ = ism.im2col(x, k, k, 1, 1)
    rows = ism._selector_rows(k * k * cin, cout)
    picked = col[:, rows].reshape(v.shape)
    six = sum(prods)
    want = np.take_along_axis(ism.im2col(six, k, k, 1, 1)[0], np.broadcast_to(rows, (col.shape[0], cout)), axis=1).reshape(v.shape)
    assert np.array_equal(v.astype(np.float64), want)
    fp32 = orc.conv2d_same(x, w, stride=1, dil=1)
    assert np.array_equal(fp32 != v, picked != 0) and (picked != 0).mean() > 0.5
    assert np.array_equal(fp32[picked != 0], (picked.astype(np.float64) * np.float64(ism.FAMILY)).astype(np.float32)[picked != 0])
    # and losing any product of the selector's step shows as a different bit pattern there
    for ij in som.SIX:
        d = ism.conv(x, w, bn=bn, drop=ij)[0]
        assert np.array_equal(d != v, picked != 0)


def test_bound_rule_is_section_5_4_1s():
    """the bound walks the instructions in the kernel's order: a zero chunk costs nothing, the order of two chunks matters"""
    rng = np.random.default_rng(9)
    x = np.abs(rng.normal(size=(1, 3, 5, 64))).astype(np.float32)
    w = np.zeros((1, 1, 64, 32), np.float32)
    w[0, 0, :16] = np.abs(rng.normal(size=(16, 32))).astype(np.float32)
    b1 = ism.conv(x, w)[1]
    w2 = w.copy()
    w2[0, 0, 48:] = 0.0  # still zero: nothing changes
    assert np.array_equal(ism.conv(x, w2)[1], b1)
    big = w.copy()
    big[0, 0, 48:] = 100 * w[0, 0, :16]
    late = ism.conv(x, big)[1]
    early = ism.conv(x, np.ascontiguousarray(big[:, :, ::-1]))[1]  # the large chunk first: every later instruction is charged on it
    assert (early > late).mean() > 0.9
    assert som.R_MFMA == 17 and len(set(itertools.chain(som.SIX))) == 6
