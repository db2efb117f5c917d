"""The 128-channel bottleneck kernels on UNEQUAL dilation phases: the launcher sizes the grid and picks the kernel from the
largest of the d x d phase sub-images, the kernels recompute the phase's own size per tile (decode_tile) and key their
validity masks, the all-padding half-tile shortcut and the out-of-range buffer offsets off it.  The cases of
bottleneck_phase_cases.py (properties asserted without a GPU in test_bottleneck_phase_cases_cpu.py) put phases one row or
column short of the grid's, tiles that are empty, phases <= 16 wide inside a 32-wide tile, phases without rows (H < d) and
both sides of the Wp = 16 / 17 dispatch boundary in front of every kernel the default knobs reach, under bnk_w8 = 0, 1, 2, at
N = 1 and N = 3: the kernel named by the restated dispatch must be the one in the profile, and the WHOLE output tensor must
be the C oracle's bits.  Then the XCD tile order on the grids with empty tiles, the whole network on 152 x 536 frames
(19 x 67 maps: unequal phases at every dilation, eight-wave kernels at d = 1, 2, 4) and the bf16x3 mode within
test_gpu_bf16x3.py's bound."""
import time

import numpy as np
import pytest
import torch

import bottleneck_phase_cases as bpc
import test_gpu_bf16x3 as bf3
import test_gpu_parity as parity
from bottleneck_phase_cases import CASES, W8_SETTINGS, case_id, geometry
from helpers import frames, report_diff
from oracle import enet_oracle as orc
from semanticsegmentationactivelearning_amd import _lib

pytestmark = pytest.mark.gpu

_REF = {}  # case id -> (input [3,H,W,128], oracle output): computed once, shared by every test of the case, never written to


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    _lib.lib()
    yield
    torch.cuda.synchronize()


def _reference(P, case):
    key = case_id(case)
    if key not in _REF:
        t0 = time.perf_counter()
        x = np.random.default_rng(case.dil * 1000003 + case.h * 1009 + case.w).normal(size=(3, case.h, case.w, 128)).astype(np.float32)
        want = orc.bottleneck(P, case.layer, x, dil=case.dil, asym=case.asym)
        x.setflags(write=False)
        want.setflags(write=False)
        _REF[key] = (x, want)
        print("%s: oracle for 3 images in %.2f s" % (key, time.perf_counter() - t0))
    return _REF[key]


def _profiled(call):
    torch.cuda.synchronize()
    _lib.profile_collect()
    _lib.profile_enable(True)
    try:
        out = call()
        torch.cuda.synchronize()
        prof = _lib.profile_collect()
    finally:
        _lib.profile_enable(False)
    return out, prof


def _layer(net, case):
    layer = getattr(net, case.layer)
    assert layer.dilation_rate[0] == case.dil and bool(layer.asymmetric) == case.asym
    return layer


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_phase_case_runs_the_expected_kernel_and_equals_the_oracle(enet_c3k19, case, n):
    net, P = enet_c3k19
    layer = _layer(net, case)
    x, want = _reference(P, case)
    xd = torch.from_numpy(x[:n].copy()).cuda()
    wd = torch.from_numpy(want[:n].copy())
    start = _lib.get_knobs()["bnk_w8"]
    got = {}
    try:
        for setting in W8_SETTINGS:
            _lib.set_knob("bnk_w8", setting)
            got[setting] = _profiled(lambda: layer(xd, training=False))
    finally:
        _lib.set_knob("bnk_w8", start)
    for setting in W8_SETTINGS:
        y, prof = got[setting]
        g = geometry(case, setting)
        tag = "%s N=%d bnk_w8=%d" % (case_id(case), n, setting)
        ran = sorted(k for k in prof if k in bpc.KERNELS)
        print("%s: %s (%d of %d tiles per image empty)" % (tag, ran, len(g.empty_tiles), g.tiles_per_image))
        assert ran == [g.kernel], "%s: expected %s, profile holds %s" % (tag, g.kernel, sorted(prof))
        assert prof[g.kernel]["launches"] == 1, prof[g.kernel]
        assert y.shape == wd.shape
        assert torch.equal(y.cpu(), wd), "%s (%s): %d elements differ from the oracle" % (
            tag, g.kernel, int((y.cpu() != wd).sum()))


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("case", bpc.xcd_cases(), ids=case_id)
def test_xcd_tile_order_gives_the_same_bits_on_grids_with_empty_tiles(enet_c3k19, case, n):
    """bnk_xcd = 1 pads the grid to a multiple of eight and adds its own empty workgroups on top of the per-phase ones"""
    net, P = enet_c3k19
    layer = _layer(net, case)
    x, want = _reference(P, case)
    xd = torch.from_numpy(x[:n].copy()).cuda()
    wd = torch.from_numpy(want[:n].copy())
    start = _lib.get_knobs()
    got = {}
    try:
        for setting in W8_SETTINGS:
            _lib.set_knob("bnk_w8", setting)
            for xcd in (0, 1):
                _lib.set_knob("bnk_xcd", xcd)
                assert _lib.get_knobs()["bnk_xcd"] == xcd
                got[setting, xcd] = _profiled(lambda: layer(xd, training=False))
    finally:
        _lib.set_knob("bnk_w8", start["bnk_w8"])
        _lib.set_knob("bnk_xcd", start["bnk_xcd"])
    for setting in W8_SETTINGS:
        g = geometry(case, setting)
        assert g.empty_tiles
        for xcd in (0, 1):
            y, prof = got[setting, xcd]
            tag = "%s N=%d bnk_w8=%d bnk_xcd=%d" % (case_id(case), n, setting, xcd)
            assert sorted(k for k in prof if k in bpc.KERNELS) == [g.kernel], "%s: %s" % (tag, sorted(prof))
            assert torch.equal(y.cpu(), wd), "%s (%s) differs from the oracle" % (tag, g.kernel)
        assert torch.equal(got[setting, 0][0], got[setting, 1][0])


def test_whole_network_on_unequal_phases_at_every_dilation(enet_c3k19):
    """2 x 152 x 536 frames: the sixteen 128-channel blocks see 19 x 67 maps -- largest phase 67 / 34 / 17 wide at dilation 1 /
    2 / 4 (eight-wave kernels), 9 / 5 wide at 8 / 16 (k_bottleneck_o4) -- with unequal phases at every dilation above 1"""
    net, P = enet_c3k19
    n, h, w = 2, 152, 536
    x = frames(range(20, 20 + n), h, w, 3)
    xd = parity.dev(x)
    names = ["Bottleneck%d_%d" % (s, i) for s in (2, 3) for i in range(1, 9)]
    layers = [getattr(net, name) for name in names]
    assert all(tuple(layer.proj_kernel.shape) == (1, 1, 128, 32) for layer in layers)
    start = _lib.get_knobs()["bnk_w8"]
    assert start == 2  # the shipping default
    parity._check_forward(net, P, x, "%dx%dx%d" % (n, h, w))  # logits and three endpoints bit-identical to the oracle
    scores, profs = {}, {}
    try:
        for setting in W8_SETTINGS:
            _lib.set_knob("bnk_w8", setting)
            _, profs[setting] = _profiled(lambda: net(xd, training=False))
            for measure in ("entropy", "margin", "confidence"):
                s = net.score(xd, measure)
                assert s.dtype == torch.float64
                scores[setting, measure] = s.clone()
    finally:
        _lib.set_knob("bnk_w8", start)
    for setting in W8_SETTINGS:
        want = {}
        for layer in layers:
            k = bpc.kernel_for(layer.dilation_rate[0], bool(layer.asymmetric), h // 8, w // 8, setting)[0]
            want[k] = want.get(k, 0) + 1
        ran = {k: v["launches"] for k, v in profs[setting].items() if k in bpc.KERNELS}
        print("bnk_w8=%d: %s" % (setting, ran))
        assert ran == want, "bnk_w8=%d: %s, expected %s" % (setting, ran, want)
        for measure in ("entropy", "margin", "confidence"):
            assert torch.equal(scores[setting, measure].view(torch.int64), scores[0, measure].view(torch.int64)), \
                "bnk_w8=%d %s" % (setting, measure)
    assert "k_bottleneck_w8" in profs[2] and "k_bottleneck_asym_w8" in profs[2], sorted(profs[2])


@pytest.mark.parametrize("case", bpc.bf16x3_cases(), ids=case_id)
def test_split_operand_mode_on_unequal_phases(enet_c3k19, case):
    """arithmetic="bf16x3" on the unequal-phase cases: test_gpu_bf16x3.py's comparison and bound (TOL_LAYER), unchanged"""
    net, P = enet_c3k19
    layer = _layer(net, case)
    assert _lib.layer_dispatch("regular", 128, 128, 32, case.asym, case.h, case.w, arithmetic="bf16x3") == "fused_bf16x3"
    x, want = _reference(P, case)
    xd = torch.from_numpy(x.copy()).cuda()
    got = layer(xd, training=False, arithmetic="bf16x3").cpu().numpy()
    exact = layer(xd, training=False).cpu().numpy()
    print("%s bf16x3: max |d| = %.3e (bound %.1e)" % (case_id(case), float(np.abs(got.astype(np.float64) - want).max()), bf3.TOL_LAYER))
    report_diff(case.layer + " bf16x3 vs oracle", got, want, exact=False, atol=bf3.TOL_LAYER)
    report_diff(case.layer + " default mode still bit-exact", exact, want)
    assert not np.array_equal(got, exact), "the opt-in mode produced the exact kernel's bits: not dispatched?"
