"""GPU tests of the fused ENet kernels at their per-image size limits.

Every fused kernel computes offsets inside one image in 32 bits, and the raw-buffer kernels mark lanes outside the image
with the offset 0x80000000; each launcher admits the shapes its offset arithmetic can address (the *_fits functions next to
the kernels) and the layer dispatch asks the same function (tests/test_fused_limits_cpu.py pins the decision on the CPU).
Here each layer runs on the device at the last shapes its fused kernel takes and at the first ones it does not, on ragged
tiles (W not a multiple of 32 on the tiled axis: the idle lanes of the border tiles are the ones that write through the
sentinel).  Per case:
  * the profile shows the kernel that ran (fused below the limit, none of the fused kernels above it);
  * the fused family equals the generic family (64-bit indexing) bit for bit over the whole tensor, pooling indices too;
  * the C oracle on a few-tile window at the image's highest-offset corner (and, for the upsample blocks, around output
    element 2^29) equals the device output inside the window (crop_oracle; test_crop_oracle_equals_the_full_oracle shows
    that the cropping itself is exact).
The multi-GB tensors are built on the device from seeded generators and freed before the next case; the model is a
module-local instance whose workspaces go away at module teardown."""
import gc

import numpy as np
import pytest
import torch

from helpers import make_model, report_diff
from oracle import enet_oracle as orc
from semanticsegmentationactivelearning_amd import _lib, synthetic as syn

pytestmark = pytest.mark.gpu

FUSED_PREFIXES = ("k_bottleneck", "k_downsample", "k_upsample", "k_initial_down16")
TOL_CONF = 1e-4   # tests/test_gpu_bf16x3.py: per-pixel confidence of the bf16x3 mode against the exact path
TOL_SCORE = 1e-6  # tests/test_gpu_bf16x3.py: per-image float64 score


@pytest.fixture(scope="module")
def model():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    _lib.lib()
    gc.collect()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    box = {"m": make_model(19, 3, seed=0)}
    yield box
    box.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    assert torch.cuda.memory_allocated() == base, "device memory left behind: %d bytes" % (torch.cuda.memory_allocated() - base)


@pytest.fixture(autouse=True)
def _free_between_cases():
    yield
    _lib.set_kernel_family(True)
    gc.collect()
    torch.cuda.empty_cache()


def _gen(seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return g


def randn(shape, seed):
    return torch.randn(shape, generator=_gen(seed), device="cuda", dtype=torch.float32)


def window_argmax(n, h, w, c, seed):
    """pooling-derived unpool indices for an upsample block with an [n,h,w,c] input: a random window code dy*2 + dx per
    (pixel, channel), as the reference's per-image index (y * 2w + x) * c + ch with y = 2i + dy, x = 2j + dx"""
    arg = torch.randint(0, 4, (n, h, w, c), generator=_gen(seed), device="cuda", dtype=torch.int64)
    dx = arg & 1
    arg.div_(2, rounding_mode="floor").mul_(2 * w).add_(dx).mul_(c)  # (dy * 2w + dx) * c
    del dx
    arg.add_((torch.arange(h, device="cuda", dtype=torch.int64) * (4 * w * c)).view(1, h, 1, 1))
    arg.add_((torch.arange(w, device="cuda", dtype=torch.int64) * (2 * c)).view(1, 1, w, 1))
    arg.add_(torch.arange(c, device="cuda", dtype=torch.int64).view(1, 1, 1, c))
    return arg


def profiled(call):
    """(call(), {kernel: ...}) of the launches the call made"""
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


def assert_path(tag, prof, kernel):
    """kernel = the fused kernel that must have run; None = none of the fused kernels may have run"""
    fused = sorted(k for k in prof if k.startswith(FUSED_PREFIXES))
    if kernel is None:
        assert not fused, "%s: above the limit, yet fused kernels ran: %s" % (tag, fused)
        assert "k_conv" in prof, "%s: the generic kernels did not run: %s" % (tag, sorted(prof))
    else:
        assert kernel in prof, "%s: %s did not run (profile: %s)" % (tag, kernel, sorted(prof))


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t


def assert_same_bits(tag, got, want):
    """bit-for-bit equality on the device; on a mismatch: count and first index, without copying the tensors"""
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s %s != %s %s" % (tag, got.shape, got.dtype,
                                                                                      want.shape, want.dtype)
    a, b = _bits(got.contiguous()), _bits(want.contiguous())
    if torch.equal(a, b):
        return
    ne = (a != b).view(-1)
    count = int(ne.sum())
    first = int(torch.argmax(ne.to(torch.uint8)))
    idx = tuple(int(i) for i in np.unravel_index(first, tuple(got.shape)))
    raise AssertionError("%s: %d / %d elements differ, first at flat index %d %s: got %r want %r"
                         % (tag, count, got.numel(), first, idx, got.reshape(-1)[first].item(), want.reshape(-1)[first].item()))


# ---- the oracle on a window ------------------------------------------------------------------------------------------
def _host(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def crop_interior(h, w, r0, c0, hc, wc, m):
    """(top, bottom, left, right) inside an hc x wc crop at (r0, c0) of an h x w plane where a run on the crop alone is
    exact: m pixels are dropped along crop edges that are not image edges (the zero padding there is not the image)"""
    return (0 if r0 == 0 else m, hc if r0 + hc == h else hc - m, 0 if c0 == 0 else m, wc if c0 + wc == w else wc - m)


def crop_oracle(P, layer, x, r0, c0, hc, wc, img=0, arg=None):
    """The C oracle on the hc x wc crop at (r0, c0) of image img of the layer input x ([n,h,w,c], device or host).
    -> ((rows, cols) of the layer OUTPUT the result covers, the oracle output there, and for a downsample block its
    pooling indices there in the full image's index form (y * w + x) * c + ch).  arg: an upsample block's indices."""
    n, h, w, c = x.shape
    kind, name = type(layer).__name__, layer.name
    xc = _host(x[img:img + 1, r0:r0 + hc, c0:c0 + wc])
    if kind == "Bottleneck":
        d = layer.dilation_rate[0]
        y = orc.bottleneck(P, name, xc, dil=d, asym=layer.asymmetric)
        t, b, l, r = crop_interior(h, w, r0, c0, hc, wc, 2 if layer.asymmetric else d)
        return (slice(r0 + t, r0 + b), slice(c0 + l, c0 + r)), y[0, t:b, l:r], None
    if kind == "BottleneckDownsample":
        assert r0 % 2 == 0 and c0 % 2 == 0 and hc % 2 == 0 and wc % 2 == 0
        y, a = orc.bottleneck_down(P, name, xc)
        t, b, l, r = crop_interior(h // 2, w // 2, r0 // 2, c0 // 2, hc // 2, wc // 2, 2)
        a = a.astype(np.int64)
        px, ch = a // c, a % c
        a = ((px // wc + r0) * w + (px % wc + c0)) * c + ch  # crop-relative -> the full image's index
        rows, cols = slice(r0 // 2 + t, r0 // 2 + b), slice(c0 // 2 + l, c0 // 2 + r)
        return (rows, cols), y[0, t:b, l:r], a[0, t:b, l:r]
    assert kind == "BottleneckUpsample"
    co = layer.output_channels
    ac = _host(arg[img:img + 1, r0:r0 + hc, c0:c0 + wc]).astype(np.int64)
    px, ch = ac // co, ac % co
    ac = ((px // (2 * w) - 2 * r0) * (2 * wc) + (px % (2 * w) - 2 * c0)) * co + ch  # full image -> crop-relative
    y = orc.bottleneck_up(P, name, xc, ac)
    t, b, l, r = crop_interior(h, w, r0, c0, hc, wc, 2)
    return (slice(2 * (r0 + t), 2 * (r0 + b)), slice(2 * (c0 + l), 2 * (c0 + r))), y[0, 2 * t:2 * b, 2 * l:2 * r], None


def check_window(tag, P, layer, x, y, r0, c0, hc, wc, img=0, arg=None, amax=None):
    (rows, cols), want, want_amax = crop_oracle(P, layer, x, r0, c0, hc, wc, img, arg)
    report_diff("%s window (%d, %d) %dx%d vs oracle" % (tag, r0, c0, hc, wc), _host(y[img, rows, cols]), want)
    if want_amax is not None:
        report_diff("%s window argmax vs oracle" % tag, _host(amax[img, rows, cols]), want_amax)


HC, WC = 36, 104  # input window: a few 8 x 32 tiles plus the margin


def windows(layer, h, w):
    """input windows to check: the highest-offset corner; for an upsample block also the one around output element 2^29"""
    out = [(h - HC, w - WC)]
    if type(layer).__name__ == "BottleneckUpsample":
        p = (1 << 29) // layer.output_channels  # output pixel of element 2^29
        if p < 4 * h * w:
            yi, xi = p // (2 * w) // 2, p % (2 * w) // 2
            out.append((min(max(yi - HC // 2, 0), h - HC) // 2 * 2, min(max(xi - WC // 2, 0), w - WC) // 2 * 2))
    return out


def test_crop_oracle_equals_the_full_oracle(model):
    """the window check itself: at small shapes, the oracle on a crop (interior) equals the oracle on the whole input, for
    every layer form below, at windows touching the image corners, edges and none"""
    net, P = model["m"]
    rng = np.random.default_rng(40)
    for name, h, w in (("Bottleneck2_2", 48, 120), ("Bottleneck2_3", 44, 112), ("Bottleneck1_1", 40, 108),
                       ("Bottleneck2_0", 44, 112), ("Bottleneck1_0", 40, 108), ("Bottleneck4_0", 40, 108),
                       ("Bottleneck5_0", 40, 108)):
        layer = getattr(net, name)
        kind = type(layer).__name__
        cin = layer.proj_kernel.shape[2]
        x = rng.normal(size=(1, h, w, cin)).astype(np.float32)
        arg = amax = None
        if kind == "Bottleneck":
            y = orc.bottleneck(P, name, x, dil=layer.dilation_rate[0], asym=layer.asymmetric)
        elif kind == "BottleneckDownsample":
            y, amax = orc.bottleneck_down(P, name, x)
        else:
            _, arg = orc.maxpool2x2_argmax(rng.normal(size=(1, 2 * h, 2 * w, layer.output_channels)).astype(np.float32))
            y = orc.bottleneck_up(P, name, x, arg)
        hc, wc = 24, 64
        for r0, c0 in ((h - hc, w - wc), (0, 0), (8, 20), (0, w - wc), (h - hc, 0)):
            check_window(name + " full", P, layer, x, y, r0, c0, hc, wc, arg=arg, amax=amax)


# ---- single layers at their limits -----------------------------------------------------------------------------------
# (layer, n, h, w, fused kernel or None = above the limit)
CASES = [
    ("Bottleneck2_1", 1, 2040, 2056, "k_bottleneck_mfma<32>"), ("Bottleneck2_1", 2, 2040, 2056, "k_bottleneck_mfma<32>"),
    ("Bottleneck2_2", 1, 2040, 2056, "k_bottleneck_mfma<32>"), ("Bottleneck2_3", 1, 2040, 2056, "k_bottleneck_mfma_asym16x"),
    ("Bottleneck2_1", 1, 2048, 2056, None), ("Bottleneck2_2", 1, 2048, 2056, None), ("Bottleneck2_3", 1, 2048, 2056, None),
    ("Bottleneck1_1", 1, 2040, 4104, "k_bottleneck16<32,64,16>"), ("Bottleneck1_1", 1, 2048, 4104, None),
    ("Bottleneck5_1", 1, 4088, 8200, "k_bottleneck16<32,16,4>"), ("Bottleneck5_1", 1, 4096, 8200, None),
    ("Bottleneck2_0", 1, 4080, 4112, "k_downsample_mfma"), ("Bottleneck2_0", 1, 4096, 4112, None),
    ("Bottleneck1_0", 1, 4080, 8224, "k_downsample16"), ("Bottleneck1_0", 1, 4096, 8224, None),
    # Bottleneck4_0 above k_upsample_mfma's limit: 1024 x 2056 and 2040 x 2056 put the 0x80000000 sentinel inside the output
    # (at 1024 x 2056 the tile that owns element 2^29 runs after nearly every ragged tile; at 2040 x 2056 half the ragged
    # tiles run after it), 2048 x 2056 wraps num_records (> 4 GB)
    ("Bottleneck4_0", 1, 1020, 2056, "k_upsample_mfma"), ("Bottleneck4_0", 1, 1024, 2056, None),
    ("Bottleneck4_0", 1, 2040, 2056, None), ("Bottleneck4_0", 1, 2048, 2056, None),
    ("Bottleneck5_0", 1, 4080, 8224, "k_upsample16"), ("Bottleneck5_0", 1, 4096, 8224, None),
]


def _layer_inputs(layer, n, h, w, seed):
    kind = type(layer).__name__
    x = randn((n, h, w, layer.proj_kernel.shape[2]), seed)
    arg = window_argmax(n, h, w, layer.output_channels, seed + 1) if kind == "BottleneckUpsample" else None
    return x, arg


def _call(layer, x, arg, arithmetic="f32"):
    if arg is not None:
        return layer(x, arg, training=False, arithmetic=arithmetic)
    return layer(x, training=False, arithmetic=arithmetic)


@pytest.mark.parametrize("name,n,h,w,kernel", CASES)
def test_layer_at_its_fused_limit(model, name, n, h, w, kernel):
    net, P = model["m"]
    layer = getattr(net, name)
    tag = "%s %dx%dx%d" % (name, n, h, w)
    x, arg = _layer_inputs(layer, n, h, w, seed=h + w)
    try:
        _lib.set_kernel_family(True)
        fused, prof = profiled(lambda: _call(layer, x, arg))
        assert_path(tag, prof, kernel)
        _lib.set_kernel_family(False)
        generic, prof = profiled(lambda: _call(layer, x, arg))
        assert_path(tag + " generic family", prof, None)
    finally:
        _lib.set_kernel_family(True)
    down = type(layer).__name__ == "BottleneckDownsample"
    y, amax = fused if down else (fused, None)
    assert_same_bits(tag + " fused family vs generic", y, generic[0] if down else generic)
    if down:
        assert_same_bits(tag + " pooling argmax, fused family vs generic", amax, generic[1])
    del generic
    for r0, c0 in windows(layer, h, w):
        check_window(tag, P, layer, x, y, r0, c0, HC, WC, img=n - 1, arg=arg, amax=amax)


@pytest.mark.parametrize("name,h,w", [("Bottleneck2_0", 4080, 4112), ("Bottleneck4_0", 1024, 2056)])
def test_bf16x3_outside_its_launcher_limit_runs_the_exact_kernels(model, name, h, w):
    """Bottleneck2_0 at 4080 x 4112 lies above the bf16x3 downsample's limit and inside k_downsample_mfma's; Bottleneck4_0 at
    1024 x 2056 above both upsample limits: arithmetic='bf16x3' runs the exact fp32 kernels and equals the f32 call"""
    net, _ = model["m"]
    layer = getattr(net, name)
    tag = "%s %dx%d bf16x3" % (name, h, w)
    x, arg = _layer_inputs(layer, 1, h, w, seed=7)
    got, prof = profiled(lambda: _call(layer, x, arg, arithmetic="bf16x3"))
    assert not [k for k in prof if "bf16x3" in k], "%s: a bf16x3 kernel ran: %s" % (tag, sorted(prof))
    assert_path(tag, prof, "k_downsample_mfma" if name == "Bottleneck2_0" else None)
    want = _call(layer, x, arg)
    if isinstance(got, tuple):
        assert_same_bits(tag + " vs f32", got[0], want[0])
        assert_same_bits(tag + " argmax vs f32", got[1], want[1])
    else:
        assert_same_bits(tag + " vs f32", got, want)


# ---- whole frames ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(8184, 16392), (8192, 16448)])
def test_whole_frame_fused_family_equals_generic(model, h, w):
    """8184 x 16392: the Initial + Bottleneck1_0 launch, Bottleneck4_0 and Bottleneck5_1 just inside their limits.
    8192 x 16448: Bottleneck4_0 at 1024 x 2056 (above k_upsample_mfma's limit), Bottleneck2_0 at 2048 x 4112 (above the
    bf16x3 downsample's)"""
    net, _ = model["m"]
    x = syn.synth_frames_device(0, 1, h, w, 3)
    inside = (h, w) == (8184, 16392)

    def score(**kw):
        return net.score(x, "entropy", return_label=True, return_confidence=True, **kw)

    try:
        _lib.set_kernel_family(True)
        (s1, e1), prof = profiled(score)
        _lib.set_kernel_family(False)
        s2, e2 = score()
    finally:
        _lib.set_kernel_family(True)
    for k in ("k_upsample_mfma", "k_initial_down16", "k_bottleneck16<32,16,4>"):
        assert (k in prof) == inside, "%dx%d: %s %s" % (h, w, k, "missing" if inside else "ran above its limit")
    for k in ("k_downsample_mfma", "k_bottleneck_mfma<32>", "k_upsample16"):
        assert k in prof, "%dx%d: %s did not run" % (h, w, k)
    assert_same_bits("%dx%d score" % (h, w), s1, s2)
    assert_same_bits("%dx%d label" % (h, w), e1["label"], e2["label"])
    assert_same_bits("%dx%d confidence" % (h, w), e1["confidence"], e2["confidence"])
    del s2, e2
    if not inside:
        s3, e3 = score(arithmetic="bf16x3")
        d_conf = float((e3["confidence"] - e1["confidence"]).abs().max())
        d_score = float((s3 - s1).abs().max())
        assert d_conf <= TOL_CONF, "bf16x3 confidence differs from the exact path by %g" % d_conf
        assert d_score <= TOL_SCORE, "bf16x3 score differs from the exact path by %g" % d_score
