"""CPU tests of the layer dispatch at the per-image size limits of the fused ENet kernels (include/ssal_enet.h:
ssal_debug_layer_dispatch, a host-only query of the same decision the layer calls make).

Every fused kernel computes offsets inside one image in 32 bits.  The limits below are restated here from the kernels'
offset arithmetic (csrc/ssal_bottleneck_mfma.hip, ssal_bottleneck_mfma16.hip, ssal_bottleneck_bf16x3.hip: the *_fits
functions), independently of the library, and each is pinned on both sides: the last admitted shape and one row more.
A later edit to a dispatch predicate that admits a shape its kernel cannot address fails here, without a GPU.
tests/test_gpu_large_shapes.py runs the same boundaries on the device."""
import ctypes

import pytest

from helpers import make_model
from semanticsegmentationactivelearning_amd import _lib

# per-image limits, H x W = the layer's input (the image for the Initial + Bottleneck1_0 launch)
LIMITS = {
    "regular128": lambda h, w: h * w * 128 <= 2 ** 29,       # k_bottleneck_mfma*: int byte offsets, 0x80000000 sentinel
    "regular64": lambda h, w: h * w * 64 <= 2 ** 29,         # k_bottleneck16<.., 64, 16>
    "regular16": lambda h, w: h * w * 16 <= 2 ** 29,         # k_bottleneck16<.., 16, 4>
    "down128": lambda h, w: h * w * 128 < 2 ** 31,           # k_downsample_mfma: y [H/2,W/2,128] in bytes
    "down64": lambda h, w: h * w * 64 < 2 ** 31,             # k_downsample16
    "up64": lambda h, w: 4 * h * w * 64 <= 2 ** 29,          # k_upsample_mfma: y [2H,2W,64] in bytes <= 2^31
    "up16": lambda h, w: 4 * h * w * 16 < 2 ** 31,           # k_upsample16 (64-bit offsets)
    "initial": lambda h, w: h * w * 16 < 2 ** 31,            # k_initial_down16 (64-bit offsets)
    "regular128_bf16x3": lambda h, w: h * w * 128 <= 2 ** 29,
    "down128_bf16x3": lambda h, w: h * w * 64 <= 2 ** 29,
    "up64_bf16x3": lambda h, w: 4 * h * w * 64 <= 2 ** 29,
}

# (layer, limit key, kernel, ragged W, the table's near-limit H, above-limit H)
CASES = [
    ("Bottleneck2_1", "regular128", "k_bottleneck_mfma<32>", 2056, 2040, 2048),
    ("Bottleneck2_2", "regular128", "k_bottleneck_mfma<32>", 2056, 2040, 2048),
    ("Bottleneck2_3", "regular128", "k_bottleneck_mfma_asym16x", 2056, 2040, 2048),
    ("Bottleneck1_1", "regular64", "k_bottleneck16<32,64,16>", 4104, 2040, 2048),
    ("Bottleneck5_1", "regular16", "k_bottleneck16<32,16,4>", 8200, 4088, 4096),
    ("Bottleneck2_0", "down128", "k_downsample_mfma", 4112, 4080, 4096),
    ("Bottleneck1_0", "down64", "k_downsample16", 8224, 4080, 4096),
    ("Bottleneck4_0", "up64", "k_upsample_mfma", 2056, 1020, 1024),
    ("Bottleneck5_0", "up16", "k_upsample16", 8224, 4080, 4096),
]


@pytest.fixture(scope="module")
def forms():
    """layer name -> (kind, cin, cout, f, asym) of the ENet the library is built for"""
    net, _ = make_model(19, 3, seed=0)
    out = {}
    for name, *_ in CASES:
        layer = getattr(net, name)
        kind = {"Bottleneck": "regular", "BottleneckDownsample": "down", "BottleneckUpsample": "up"}[type(layer).__name__]
        kh, kw, cin, f = layer.proj_kernel.shape
        out[name] = (kind, cin, layer.output_channels, f, bool(getattr(layer, "asymmetric", False)))
    return out


def dispatch(form, h, w, arithmetic="f32"):
    return _lib.layer_dispatch(*form, h, w, arithmetic=arithmetic)


def last_admitted_h(limit, w):
    h = 1
    while limit(2 * h, w):
        h *= 2
    lo, hi = h, 2 * h  # limit(lo) holds, limit(hi) does not
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if limit(mid, w) else (lo, mid)
    return lo


@pytest.fixture(autouse=True)
def _default_switches():
    _lib.set_kernel_family(True)
    yield
    _lib.set_kernel_family(True)
    _lib.set_knob("fuse_ends", 3)


@pytest.mark.parametrize("name,key,kernel,w,h_near,h_above", CASES)
def test_fused_dispatch_stops_at_the_kernel_limit(forms, name, key, kernel, w, h_near, h_above):
    form, limit = forms[name], LIMITS[key]
    h = last_admitted_h(limit, w)
    assert limit(h, w) and not limit(h + 1, w)
    assert dispatch(form, h, w) == "fused", "%s (%s) at %dx%d: the last shape its limit admits" % (name, kernel, h, w)
    assert dispatch(form, h + 1, w) == "generic", "%s (%s) at %dx%d: one row past its limit" % (name, kernel, h + 1, w)
    # the table of tests/test_gpu_large_shapes.py: near the limit -> fused, above -> generic
    assert h_near <= h < h_above
    assert dispatch(form, h_near, w) == "fused" and dispatch(form, h_above, w) == "generic"
    # exactly at the limit's power of two (square-ish shapes): inclusive limits admit it, strict ones do not
    for hh, ww in ((2048, 2048), (2048, 4096), (4096, 4096), (4096, 8192), (8192, 8192)):
        assert dispatch(form, hh, ww) == ("fused" if limit(hh, ww) else "generic"), (name, hh, ww)


def test_upsample_128_to_64_limit_is_the_kernels_not_the_old_predicate(forms):
    """k_upsample_mfma addresses y [2H,2W,64] with int byte offsets and the 0x80000000 sentinel: 4 * H * W * 64 <= 2^29.
    The dispatch used to admit 4 * H * W * 64 < 2^31, where the sentinel lands inside the output (2 .. 4 GB) or
    num_records wraps (past 4 GB)."""
    form = forms["Bottleneck4_0"]
    w = 2056
    old_last = last_admitted_h(lambda h, w_: 4 * h * w_ * 64 < 2 ** 31, w)
    assert old_last == 4080
    for h in (1021, 1024, 2040, 2048, old_last):
        assert dispatch(form, h, w) == "generic", (h, w)
    assert dispatch(form, 1020, w) == "fused"
    # whole frames: Bottleneck4_0 runs at frame / 8
    assert dispatch(form, 8192 // 8, 16448 // 8) == "generic"
    assert dispatch(form, 8184 // 8, 16392 // 8) == "fused"


@pytest.mark.parametrize("name,key,w", [("Bottleneck2_1", "regular128_bf16x3", 2056),
                                        ("Bottleneck2_3", "regular128_bf16x3", 2056),
                                        ("Bottleneck2_0", "down128_bf16x3", 4112),
                                        ("Bottleneck4_0", "up64_bf16x3", 2056)])
def test_bf16x3_dispatch_needs_its_own_launcher_limit(forms, name, key, w):
    """shapes outside the bf16x3 launcher's limit run the exact fp32 kernel (fused where its own limit admits them)"""
    form, limit = forms[name], LIMITS[key]
    fp32_key = key.replace("_bf16x3", "")
    h = last_admitted_h(limit, w)
    assert dispatch(form, h, w, "bf16x3") == "fused_bf16x3", (name, h, w)
    past = dispatch(form, h + 1, w, "bf16x3")
    assert past == dispatch(form, h + 1, w, "f32") == ("fused" if LIMITS[fp32_key](h + 1, w) else "generic"), (name, h + 1, w)


def test_bf16x3_downsample_gap_takes_the_exact_fused_kernel(forms):
    """Bottleneck2_0: the bf16x3 launcher admits H * W * 64 <= 2^29, k_downsample_mfma H * W * 128 < 2^31; in between
    arithmetic='bf16x3' used to fail with SSAL_EHIP"""
    form = forms["Bottleneck2_0"]
    assert dispatch(form, 2040, 4112, "bf16x3") == "fused_bf16x3"
    for h, w in ((2041, 4112), (2048, 4112), (4080, 4112)):
        assert dispatch(form, h, w, "bf16x3") == "fused", (h, w)
    assert dispatch(form, 4096, 4112, "bf16x3") == "generic"
    assert dispatch(form, 8192 // 4, 16448 // 4, "bf16x3") == "fused"  # the 8192 x 16448 frame's Bottleneck2_0


def test_layers_without_a_bf16x3_kernel_ignore_the_mode(forms):
    for name in ("Bottleneck1_0", "Bottleneck1_1", "Bottleneck5_0", "Bottleneck5_1"):
        for h, w in ((64, 128), (256, 512), (4096, 8224)):
            assert dispatch(forms[name], h, w, "bf16x3") == dispatch(forms[name], h, w, "f32"), (name, h, w)


def test_initial_down16_limit():
    limit = LIMITS["initial"]
    w = 16392
    h = last_admitted_h(limit, w)
    assert (h, w) == (8188, 16392)
    assert _lib.layer_dispatch("initial", 3, 16, 16, False, 8184, w) == "fused"
    assert _lib.layer_dispatch("initial", 3, 16, 16, False, h, w) == "fused"
    assert _lib.layer_dispatch("initial", 3, 16, 16, False, h + 1, w) == "generic"
    assert _lib.layer_dispatch("initial", 3, 16, 16, False, 8192, 16384) == "generic"  # h * w * 16 == 2^31: strict
    assert _lib.layer_dispatch("initial", 2, 16, 16, False, 64, 128) == "generic"  # no fused form for 2 channels
    _lib.set_knob("fuse_ends", 2)
    assert _lib.layer_dispatch("initial", 3, 16, 16, False, 64, 128) == "generic"


def test_bench_shapes_keep_every_fused_kernel(forms):
    """batch of 1024 x 2048 frames: every layer keeps its fused kernel (the bf16x3 mode its split kernels)"""
    h, w = 1024, 2048
    at = {"Bottleneck1_0": (h // 2, w // 2), "Bottleneck1_1": (h // 4, w // 4), "Bottleneck2_0": (h // 4, w // 4),
          "Bottleneck2_1": (h // 8, w // 8), "Bottleneck2_2": (h // 8, w // 8), "Bottleneck2_3": (h // 8, w // 8),
          "Bottleneck4_0": (h // 8, w // 8), "Bottleneck5_0": (h // 4, w // 4), "Bottleneck5_1": (h // 2, w // 2)}
    for name, (lh, lw) in at.items():
        assert dispatch(forms[name], lh, lw) == "fused", name
        want = "fused_bf16x3" if name in ("Bottleneck2_0", "Bottleneck2_1", "Bottleneck2_2", "Bottleneck2_3",
                                          "Bottleneck4_0") else "fused"
        assert dispatch(forms[name], lh, lw, "bf16x3") == want, name
    assert _lib.layer_dispatch("initial", 3, 16, 16, False, h, w) == "fused"


def test_generic_family_switch_and_argument_errors(forms):
    _lib.set_kernel_family(False)
    for name in forms:
        assert dispatch(forms[name], 64, 128) == "generic"
        assert dispatch(forms[name], 64, 128, "bf16x3") == "generic"
    assert _lib.layer_dispatch("initial", 3, 16, 16, False, 64, 128) == "generic"
    _lib.set_kernel_family(True)
    with pytest.raises(ValueError):
        _lib.layer_dispatch("regular", 128, 128, 32, False, 0, 8)
    with pytest.raises(ValueError):
        _lib.layer_dispatch("down", 64, 128, 16, False, 8, 8, arithmetic="fp16")
    out = ctypes.c_int(-1)
    with pytest.raises(ValueError, match="kind"):
        _lib.check(_lib.lib().ssal_debug_layer_dispatch(7, 16, 16, 4, 0, 8, 8, 0, ctypes.byref(out)))
