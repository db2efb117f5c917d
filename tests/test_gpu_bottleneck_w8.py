"""The 128-channel bottlenecks on eight-wave workgroups (knob bnk_w8: k_bottleneck_w8, k_bottleneck_asym_w8) produce the
bits of today's kernels (bnk_w8 = 0) and of the C oracle: single layers through ssal_enet_run_layer at one exact tile, ragged
in both axes, interior tiles with neighbours on all sides and narrower than a tile -- for a dilated layer the same shapes
times the dilation, so that its phase sub-images are a single tile, ragged, and (17 x 31) smaller than a tile with a halo
ring of SAME-padding zeros -- at N = 1 and N = 3; then the whole network's scores under every setting of the knob.
Every dilated shape here is a multiple of the dilation, so all its phases are the same size; the unequal-phase geometries
(phases a row or column short of the grid's, empty tiles, phases <= 16 wide under the 32-wide tile, H < dilation, both sides
of the Wp = 16 / 17 dispatch boundary) are in tests/test_gpu_bottleneck_phases.py, their case table in
tests/bottleneck_phase_cases.py (checked without a GPU by tests/test_bottleneck_phase_cases_cpu.py)."""
import numpy as np
import pytest
import torch

from oracle import enet_oracle as orc
from semanticsegmentationactivelearning_amd import _lib, synthetic as syn

pytestmark = pytest.mark.gpu

SHAPES = [(8, 32), (9, 33), (24, 96), (17, 31)]
REGULAR = [("Bottleneck2_1", 1), ("Bottleneck2_2", 2), ("Bottleneck2_4", 4), ("Bottleneck2_6", 8)]
ASYM = ["Bottleneck2_3", "Bottleneck3_7"]
# (layer, h, w, knob value that moves the layer to its eight-wave kernel, that kernel's profile row)
CASES = [(name, d * h, d * w, 1, "k_bottleneck_w8") for name, d in REGULAR for h, w in SHAPES] + \
        [(name, h, w, 2, "k_bottleneck_asym_w8") for name in ASYM for h, w in SHAPES]

_REF = {}  # (layer, h, w) -> (input [3,h,w,128], oracle output): computed once, shared by the N = 1 and N = 3 cases


def _reference(P, layer, name, h, w):
    key = (name, h, w)
    if key not in _REF:
        x = np.random.default_rng(h * 1000 + w).normal(size=(3, h, w, 128)).astype(np.float32)
        _REF[key] = (x, orc.bottleneck(P, name, x, dil=layer.dilation_rate[0], asym=layer.asymmetric))
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


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("name,h,w,setting,kernel", CASES)
def test_eight_wave_layer_equals_todays_kernel_and_oracle(enet_c3k19, name, h, w, setting, kernel, n):
    net, P = enet_c3k19
    layer = getattr(net, name)
    assert layer.dilation_rate[0] == dict(REGULAR).get(name, 1) and layer.asymmetric == (name in ASYM)
    x, want = _reference(P, layer, name, h, w)
    xd = torch.from_numpy(x[:n]).cuda()
    start = _lib.get_knobs()["bnk_w8"]
    try:
        _lib.set_knob("bnk_w8", 0)
        old, prof_old = _profiled(lambda: layer(xd, training=False))
        _lib.set_knob("bnk_w8", setting)
        new, prof_new = _profiled(lambda: layer(xd, training=False))
    finally:
        _lib.set_knob("bnk_w8", start)
    tag = "%s %dx%dx%d" % (name, n, h, w)
    assert kernel not in prof_old and kernel in prof_new, "%s: %s / %s" % (tag, sorted(prof_old), sorted(prof_new))
    assert torch.equal(new, old), "%s: bnk_w8=%d differs from bnk_w8=0" % (tag, setting)
    assert torch.equal(new.cpu(), torch.from_numpy(want[:n])), "%s: bnk_w8=%d differs from the oracle" % (tag, setting)
    assert torch.equal(old.cpu(), torch.from_numpy(want[:n])), "%s: bnk_w8=0 differs from the oracle" % (tag,)


@pytest.mark.parametrize("name,kernel,old_kernel", [("Bottleneck2_1", "k_bottleneck_w8", "k_bottleneck_mfma<32>"),
                                                    ("Bottleneck2_2", "k_bottleneck_w8", "k_bottleneck_mfma<32>"),
                                                    ("Bottleneck2_3", "k_bottleneck_asym_w8", "k_bottleneck_mfma_asym16x")])
def test_eight_wave_kernels_stop_at_2_pow_28_elements(enet_c3k19, name, kernel, old_kernel):
    """the eight-wave kernels take images of at most 2^28 floats: 1020 x 2056 x 128 is the last ragged shape inside (every byte
    offset they form stays below 2^30) and must equal the four-wave kernel's bits; one row more runs the four-wave kernel"""
    net, _ = enet_c3k19
    layer = getattr(net, name)
    w = 2056
    assert 1020 * w * 128 <= 2 ** 28 < 1021 * w * 128
    assert _lib.get_knobs()["bnk_w8"] == 2  # the shipping default
    x = torch.randn((1, 1021, w, 128), device="cuda", generator=torch.Generator("cuda").manual_seed(28))
    _, prof = _profiled(lambda: layer(x, training=False))
    assert old_kernel in prof and kernel not in prof, sorted(prof)
    x = x[:, :1020].contiguous()
    new, prof = _profiled(lambda: layer(x, training=False))
    assert kernel in prof and old_kernel not in prof, sorted(prof)
    try:
        _lib.set_knob("bnk_w8", 0)
        old = layer(x, training=False)
    finally:
        _lib.set_knob("bnk_w8", 2)
    assert torch.equal(new, old), "%s 1020x%d: bnk_w8=2 differs from bnk_w8=0" % (name, w)


def test_whole_network_scores_same_bits_under_every_setting(enet_c3k19):
    net, _ = enet_c3k19
    x = syn.synth_frames_device(0, 2, 64, 128, 3)
    start = _lib.get_knobs()["bnk_w8"]
    got = {}
    try:
        for setting in (0, 1, 2):
            _lib.set_knob("bnk_w8", setting)
            assert _lib.get_knobs()["bnk_w8"] == setting
            for measure in ("entropy", "margin", "confidence"):
                s = net.score(x, measure)
                assert s.dtype == torch.float64
                got[setting, measure] = s.clone()
    finally:
        _lib.set_knob("bnk_w8", start)
    for (setting, measure), s in got.items():
        assert torch.equal(s.view(torch.int64), got[0, measure].view(torch.int64)), "bnk_w8=%d %s" % (setting, measure)
