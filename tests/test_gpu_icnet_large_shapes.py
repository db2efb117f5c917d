"""GPU tests of ICNet's convolution kernels at their 32-bit offset guards (tests/icnet_limits.py restates the guards,
tests/test_icnet_limits_cpu.py pins the dispatch to them and proves the part references below exact on the CPU).

Every kernel reaches its tensors through raw buffer resources and 32-bit byte offsets, with 0xFFFFFFFF as the out-of-range
offset of padding taps and idle lanes.  Here each launcher runs at the last shape it admits (and the first one it does not), on
ragged tiles, with tensors whose byte offsets have bit 31 set.  Per case, in this order:
  1. the kernel that ran: the dry query before the call, the launch profile after it, and the guard the shape sits under;
  2. whole-tensor bit equality on the device against the same operator on parts whose offsets all stay below 2^31: one call per
     image for the launch-wide limits, row bands of at most a quarter of the image for the per-image limits (axis_plan's margins);
  3. the C oracle, bit for bit, on windows at the highest-offset corner of the last image and around the output element and the
     input pixel whose byte offset is 2^31 (bf16x3: the window is gated against the split model's value and bound instead).
Largest voffset (+ scalar offset) against num_records, per kernel (the reading asked for before the first device run):
  k_igemm / k_igemm_bf16x3   x: last pixel's row N H W Cin 4 - Cin 4 + 16 col4 (< 2^32 - 16384 - 4) + soffset 128 (Cin / 32 - 1)
                             <= 8064, added by the hardware behind the range check: the sum stays below 2^32 - 8 KiB, never wraps,
                             and 0xFFFFFFFF >= num_records for every admitted size.  y / res: (M - 1) Cout 4 + 4 co < num_records
                             = M Cout 4 < 2^32 - 256; m itself < M + 255 < 2^31.  nbase = n x (Hs Ws Cin 4): the image bytes reach
                             2^31 only for N = 1 (n = 0), where the int product wraps to the same unsigned value.
  k_conv3x3_c32              per image: x ((iy W + ix) 128 + 16 q) < H W 128 < 2^31, y ((oy W + ox) Cout + co) 4 < 2^31 (int);
                             lanes past the image form larger ints but select 0xFFFFFFFF.
  k_conv1x1_up2_c128         per image: x (sy Ws + sx) 512 + 16 q < Hs Ws 512 < 2^31; y < 4 Hs Ws Cout 4 < 2^31.
  k_conv_first               64-bit indices, no buffer resource.
The multi-GB tensors are built on the device from seeded generators and freed before the next case."""
import gc
import time

import numpy as np
import pytest
import torch

import icnet_limits as lim
import icnet_split_model as ism
import semanticsegmentationactivelearning_amd as ssal
from semanticsegmentationactivelearning_amd import _lib, synthetic as syn
from semanticsegmentationactivelearning_amd.models.util import conv_ops as cops
from test_gpu_icnet_bf16x3 import gate
from test_gpu_large_shapes import assert_same_bits, profiled, randn

pytestmark = pytest.mark.gpu

WIN_H, WIN_W = 20, 40  # output window: a few 8 x 16 tiles


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    _lib.lib()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    yield
    gc.collect()
    torch.cuda.synchronize()
    print("\nlarge ICNet shapes: %.1f s, peak device memory %.2f GiB" % (time.time() - t0, torch.cuda.max_memory_allocated() / 2 ** 30))
    torch.cuda.empty_cache()
    assert torch.cuda.memory_allocated() <= base, "device memory left behind: %d bytes" % (torch.cuda.memory_allocated() - base)


@pytest.fixture(autouse=True)
def _free_between_cases():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _params(form, seed):
    cin, cout, k, stride, dil, up2, res, relu, bias = form
    rng = np.random.default_rng(seed)
    kern = (rng.normal(size=(k, k, cin, cout)) / np.sqrt(k * k * cin)).astype(np.float32)
    if cin % 32:
        kern = (rng.normal(size=(k, k, cin, cout)) / 5).astype(np.float32)
    return kern, (None if bias else lim.bn_params(rng, cout)), (rng.normal(size=cout).astype(np.float32) if bias else None)


def _run(x, kern, form, bn, b, res, arithmetic):
    cin, cout, k, stride, dil, up2, _, relu, _ = form
    return cops.conv_bn_act(x, kern, stride, dil, bn=bn, bias=b, residual=res, relu=relu, upsample2x=up2, arithmetic=arithmetic)


def _windows(form, n, h, w, ho, wo):
    """output windows (image, rows, cols): the highest-offset corner of the last image; around the output element and around the
    input pixel whose byte offset is 2^31, where the tensor reaches it"""
    cin, cout, k, stride, dil, up2, *_ = form
    out = [(n - 1, (max(ho - WIN_H, 0), ho), (max(wo - WIN_W, 0), wo))]
    p = 2 ** 31 // (4 * cout)  # output pixel of byte offset 2^31
    if p < n * ho * wo:
        img, oy, ox = p // (ho * wo), p % (ho * wo) // wo, p % wo
        out.append((img, lim.clamp_window(oy, WIN_H, ho), lim.clamp_window(ox, WIN_W, wo)))
    q = 2 ** 31 // (4 * cin)   # input pixel of byte offset 2^31
    if q < n * h * w:
        img, iy, ix = q // (h * w), q % (h * w) // w, q % w
        f = 2 if up2 else 1
        out.append((img, lim.clamp_window(iy * f // stride, WIN_H, ho), lim.clamp_window(ix * f // stride, WIN_W, wo)))
    return out


def _bf16x3_model(xc, kern, stride, dil, bn, bias, rc, relu, up2):
    assert not up2
    return ism.conv(xc, kern, stride, dil, bn, bias, rc, relu)


def check_case(tag, form, n, h, w, row, parts, arithmetic=None, seed=1, bit31=True):
    """form = (cin, cout, k, stride, dil, up2, res, relu, bias); row: the profile row that must appear; parts: "images" / "bands" """
    cin, cout, k, stride, dil, up2, has_res, relu, bias = form
    arith = arithmetic or "f32"
    ho, wo = lim.out_dims(h, w, k, stride, dil, up2)
    # 1. the kernel: predicates, dry query
    want = lim.expected(n, h, w, cin, cout, k, stride, dil, up2, has_res, arith)
    assert want is not None and lim.profile_row(*want) == row, (tag, want, row)
    assert _lib.icnet_conv_dispatch(n, h, w, cin, cout, k, stride, dil, up2, has_res, arith) == want, tag
    in_bytes, out_bytes = n * h * w * cin * 4, n * ho * wo * cout * 4
    print("%s: %s, input %d B, output %d B (2^32 - %d / 2^32 - %d)" % (tag, row, in_bytes, out_bytes, 2 ** 32 - in_bytes, 2 ** 32 - out_bytes))
    # bit31: the launch-wide limits admit offsets with bit 31 set; the per-image guards exist to keep every offset below 2^31
    assert (max(in_bytes, out_bytes) - 4 >= 2 ** 31) == bit31, "%s: byte offsets with bit 31 set: expected %s" % (tag, bit31)
    kern, bn, b = _params(form, seed)
    x = randn((n, h, w, cin), seed + 10) if cin % 32 == 0 else torch.rand((n, h, w, cin), generator=torch.Generator(device="cuda").manual_seed(seed), device="cuda")
    res = randn((n, ho, wo, cout), seed + 11) if has_res else None
    y, prof = profiled(lambda: _run(x, kern, form, bn, b, res, arithmetic))
    assert row in prof and prof[row]["launches"] == 1, "%s: %s did not run once (profile: %s)" % (tag, row, sorted(prof))
    assert len([r for r in prof if r.startswith("k_")]) == 1, "%s: more than one kernel: %s" % (tag, sorted(prof))
    # 2. the whole tensor against the operator on parts
    if parts == "images":
        assert n > 1 and in_bytes // n < 2 ** 31 and out_bytes // n < 2 ** 31
        for i in range(n):
            part = _run(x[i:i + 1], kern, form, bn, b, None if res is None else res[i:i + 1], arithmetic)
            assert_same_bits("%s image %d vs its own call" % (tag, i), y[i:i + 1], part)
            del part
    else:
        for img in range(n):
            for rows in lim.bands(ho, 4):
                i0, i1, oa = lim.axis_plan(h, k, stride, dil, up2, *rows)
                xb = x[img:img + 1, i0:i1].contiguous()
                ph = lim.out_dims(i1 - i0, w, k, stride, dil, up2)[0]
                rb = None if res is None else res[img:img + 1, oa:oa + ph].contiguous()
                part = _run(xb, kern, form, bn, b, rb, arithmetic)
                assert_same_bits("%s image %d rows %s vs the band's own call" % (tag, img, rows), y[img:img + 1, rows[0]:rows[1]],
                                 part[:, rows[0] - oa:rows[1] - oa])
                del part, xb, rb
    # 3. the oracle on windows
    for img, rows, cols in _windows(form, n, h, w, ho, wo):
        fx = lambda r0, r1, c0, c1: x[img:img + 1, r0:r1, c0:c1].cpu().numpy()
        fr = None if res is None else (lambda r0, r1, c0, c1: res[img:img + 1, r0:r1, c0:c1].cpu().numpy())
        got = y[img:img + 1, rows[0]:rows[1], cols[0]:cols[1]].cpu().numpy()
        wtag = "%s window image %d rows %s cols %s" % (tag, img, rows, cols)
        if arithmetic == "bf16x3":
            value, bound = lim.window_oracle(fx, fr, h, w, kern, stride, dil, bn, b, relu, up2, rows, cols, conv=_bf16x3_model)
            gate(wtag, got, np.ascontiguousarray(value), np.ascontiguousarray(bound))
        else:
            want_w = lim.window_oracle(fx, fr, h, w, kern, stride, dil, bn, b, relu, up2, rows, cols)
            ne = got.view(np.uint32) != np.ascontiguousarray(want_w).view(np.uint32)
            assert not ne.any(), "%s: %d of %d elements differ from the C oracle" % (wtag, ne.sum(), ne.size)


def check_refused(form, n, h, w, arithmetic=None):
    """the first refused shape: ValueError with the launchers' message, nothing launched"""
    cin, cout, k, stride, dil, up2, has_res, relu, bias = form
    assert lim.expected(n, h, w, cin, cout, k, stride, dil, up2, has_res, arithmetic or "f32") is None
    kern, bn, b = _params(form, 3)
    ho, wo = lim.out_dims(h, w, k, stride, dil, up2)
    x = torch.empty((n, h, w, cin), device="cuda")  # never read
    res = torch.empty((n, ho, wo, cout), device="cuda") if has_res else None

    def call():
        with pytest.raises(ValueError, match=lim.REFUSED):
            _run(x, kern, form, bn, b, res, arithmetic)

    _, prof = profiled(call)
    assert not prof, "refused, yet launched: %s" % sorted(prof)


def last_h(form, n, w):
    cin, cout, k, stride, dil, up2, *_ = form
    return lim.last_admitted(lambda v: lim.igemm_fits(n, v, w, cin, cout, k, stride, dil, up2))


# form = (cin, cout, k, stride, dil, up2, res, relu, bias)
IN_1X1 = (32, 32, 1, 1, 1, False, False, True, False)
OUT_1X1 = (32, 128, 1, 1, 1, False, True, True, False)
DIL2 = (64, 64, 3, 1, 2, False, True, True, False)
S2 = (32, 64, 3, 2, 1, False, False, True, False)
UP2 = (256, 128, 3, 1, 2, True, True, True, False)
HEAD = (128, 19, 1, 1, 1, True, False, False, True)
C32 = (32, 32, 3, 1, 1, False, False, True, False)
C32_64 = (32, 64, 3, 1, 1, False, True, True, False)
FIRST = (3, 32, 3, 2, 1, False, False, True, False)

# (id, form, n, w, profile row): the height is the last one the launch-wide guard admits at this n, w
LAUNCH_WIDE = [
    ("igemm_input_side_1x1", IN_1X1, 3, 4095, "k_igemm<1>"),
    ("igemm_output_side_1x1_res", OUT_1X1, 3, 1023, "k_igemm<4>"),
    ("igemm_taps_dil2_res", DIL2, 3, 2047, "k_igemm<2>"),
    ("igemm_taps_stride2_odd_map", S2, 3, 4095, "k_igemm<2>"),
    ("igemm_up2_adjacent_loader", UP2, 3, 510, "k_igemm<4,up2>"),
    ("igemm_up2_per_pixel_loader", UP2, 3, 511, "k_igemm<4,up2>"),
]


@pytest.mark.parametrize("tag,form,n,w,row", LAUNCH_WIDE, ids=[c[0] for c in LAUNCH_WIDE])
def test_igemm_at_its_launch_wide_limit(tag, form, n, w, row):
    h = last_h(form, n, w)
    if tag == "igemm_input_side_1x1":
        assert (n, h, w) == (3, 2731, 4095)
    if tag == "igemm_taps_stride2_odd_map":
        assert h % 2 == 1 and w % 2 == 1
    if form is UP2:
        assert (lim.out_dims(h, w, 3, 1, 2, True)[1] % 4 == 0) == (w == 510)
    check_case("%s %dx%dx%d" % (tag, n, h, w), form, n, h, w, row, "images")


@pytest.mark.parametrize("tag,form,n,w,row", LAUNCH_WIDE[:3], ids=[c[0] for c in LAUNCH_WIDE[:3]])
def test_igemm_bf16x3_at_its_launch_wide_limit(tag, form, n, w, row):
    h = last_h(form, n, w)
    check_case("%s bf16x3 %dx%dx%d" % (tag, n, h, w), form, n, h, w, row.replace("k_igemm<", "k_igemm_bf16x3<"), "images",
               arithmetic="bf16x3")


@pytest.mark.parametrize("form,n,w,arithmetic", [(IN_1X1, 3, 4095, None), (OUT_1X1, 3, 1023, None), (IN_1X1, 3, 4095, "bf16x3")],
                         ids=["input_side", "output_side", "input_side_bf16x3"])
def test_first_refused_shape_raises_and_launches_nothing(form, n, w, arithmetic):
    h = last_h(form, n, w) + 1
    if form is IN_1X1:
        assert 3 * 2731 * 4096 * 128 >= lim.IGEMM_IN_LIMIT  # the issue's example is refused too
    check_refused(form, n, h, w, arithmetic)


def test_head_form_above_the_fast_kernels_limit():
    """conv6_cls's form on a 2048 x 2048 source: H W 512 == 2^31, the first shape k_conv1x1_up2_c128 refuses -> k_igemm<1,up2>"""
    assert not lim.conv1x1_up2_c128_fits(1, 2048, 2048, 19) and lim.conv1x1_up2_c128_fits(1, 2048, 2047, 19)
    check_case("head 1x2048x2048", HEAD, 1, 2048, 2048, "k_igemm<1,up2>", "bands", bit31=False)


@pytest.mark.parametrize("w", [2047, 2045])
def test_conv1x1_up2_c128_at_its_limit(w):
    h = lim.last_admitted(lambda v: lim.conv1x1_up2_c128_fits(1, v, w, 19))
    assert (2 * w) % lim.HT_W and (w == 2047 or (2 * h) % lim.HT_H)  # ragged tiles
    check_case("k_conv1x1_up2_c128 1x%dx%d" % (h, w), HEAD, 1, h, w, "k_conv1x1_up2_c128", "bands", bit31=False)


@pytest.mark.parametrize("form,w", [(C32, 4095), (C32_64, 2047)], ids=["cout32", "cout64_res"])
def test_conv3x3_c32_at_its_limit(form, w):
    cout = form[1]
    h = lim.last_admitted(lambda v: lim.conv3x3_c32_fits(1, v, w, cout))
    assert h * w < (2 ** 24 if cout == 32 else 2 ** 23) <= (h + 1) * w and w % lim.HT_W and h % lim.HT_H
    check_case("k_conv3x3_c32 cout %d 1x%dx%d" % (cout, h, w), form, 1, h, w, "k_conv3x3_c32", "bands", bit31=False)


def test_conv3x3_c32_form_above_its_limit():
    assert not lim.conv3x3_c32_fits(1, 4096, 4096, 32)
    check_case("3x3 32->32 1x4096x4096", C32, 1, 4096, 4096, "k_igemm<1>", "bands", bit31=False)


def test_first_conv_beyond_four_gib():
    """k_conv_first (64-bit indices) with an output above 2^32 bytes on an odd map; its launcher's own limit (2^31 tiles) holds no
    device tensor: tests/test_icnet_limits_cpu.py::test_first_conv_boundary"""
    n, h, w = 1, 8193, 16385
    assert 4097 * 8193 * 32 * 4 > 2 ** 32
    check_case("first conv 1x%dx%d" % (h, w), FIRST, n, h, w, "k_conv_first", "bands")


# ---- the network ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net19():
    box = {}
    net = ssal.ICNet(19)
    net.build((None, None, None, 3))
    syn.randomize_icnet(net, seed=0)
    box["net"], box["P"] = net, syn.icnet_params_dict(net)
    yield box
    box["net"]._release_device_state()
    box.clear()
    gc.collect()
    torch.cuda.empty_cache()


def _workspace_bytes(net, n, h, w):
    handle = net._sync_handle()
    return int(_lib.lib().ssal_icnet_workspace_bytes(handle, n, h, w))


def test_network_refuses_two_pow_27_pixels(net19):
    net = net19["net"]
    assert not lim.api_admits(32, 2048, 2048) and lim.api_admits(31, 2048, 2048) and lim.api_admits(1, 8192, 16352)
    x = torch.zeros((32, 2048, 2048, 3), dtype=torch.uint8, device="cuda")
    _, prof = profiled(lambda: pytest.raises(ValueError, net.score, x, "margin").match(lim.API_REFUSED))
    assert not prof, "refused, yet launched: %s" % sorted(prof)


def test_batch_below_the_api_limit_equals_its_chunks(net19):
    """31 x 2048 x 2048 uint8: conv1_sub1's output = conv2_sub1's input is 3.9 GiB; scores and labels equal the same call on
    chunks of at most 4 images, bit for bit"""
    net = net19["net"]
    n, h, w = 31, 2048, 2048
    assert lim.api_admits(n, h, w) and n * (h // 2) * (w // 2) * 32 * 4 > 2 ** 31
    print("workspace bytes of %d x %d x %d: %d" % (n, h, w, _workspace_bytes(net, n, h, w)))
    x = torch.randint(0, 256, (n, h, w, 3), generator=torch.Generator(device="cuda").manual_seed(31), device="cuda", dtype=torch.uint8)
    (s, e), prof = profiled(lambda: net.score(x, "margin", return_label=True))
    for row in ("k_front2<s2>", "k_front2<s1>", "k_conv3x3_c32", "k_conv1x1_up2_c128"):
        assert row in prof, "%s did not run (profile: %s)" % (row, sorted(prof))
    label = e["label"]
    for i in range(0, n, 4):
        sc, ec = net.score(x[i:i + 4], "margin", return_label=True)
        assert_same_bits("scores of images %d.." % i, s[i:i + 4], sc)
        assert_same_bits("labels of images %d.." % i, label[i:i + 4], ec["label"])


def test_one_frame_below_the_api_limit_every_layer_against_the_oracle(net19):
    """8192 x 16352: after the forward call every convolution's output window at the highest-offset corner of its endpoint equals
    the C oracle on the crop of its input endpoint; the score call (the fused fronts, the dual launch) gives the labels of the
    forward logits"""
    net, P = net19["net"], net19["P"]
    n, h, w = 1, 8192, 16352
    assert lim.api_admits(n, h, w) and not lim.api_admits(n, h, w + 32)
    print("workspace bytes of %d x %d x %d: %d" % (n, h, w, _workspace_bytes(net, n, h, w)))
    x = syn.synth_frames_device(0, n, h, w, 3)
    logits, prof = profiled(lambda: net(x))
    for row in ("k_conv3x3_c32", "k_conv1x1_up2_c128", "k_conv_first"):
        assert row in prof, "%s did not run (profile: %s)" % (row, sorted(prof))
    for c in ism.icnet_convs():
        hh, ww = h // c["div"], w // c["div"]
        k, stride, dil, up2 = c["k"], c["stride"], c["dil"], c["up2"]
        want_kernel = lim.expected(n, hh, ww, c["cin"], c["cout"], k, stride, dil, up2, c["res"] is not None)
        assert want_kernel is not None and lim.profile_row(*want_kernel) in prof, (c["name"], want_kernel)
        src = x if c["src"] is None else net.endpoint(c["src"])
        out = net.endpoint(ism.output_endpoint(c["name"]))
        res = None if c["res"] is None else net.endpoint(c["res"])
        ho, wo = lim.out_dims(hh, ww, k, stride, dil, up2)
        assert tuple(out.shape) == (n, ho, wo, c["cout"]), c["name"]
        rows, cols = (max(ho - 12, 0), ho), (max(wo - 24, 0), wo)
        kern = P[c["name"] + ".kernel"]
        bn = tuple(P["%s.%s" % (c["name"], a)] for a in ("mean", "variance", "gamma", "beta")) \
            if c["name"] + ".gamma" in P else None
        bias = P.get(c["name"] + ".bias") if bn is None else None
        sub = c["div"] if c["src"] is None else 1  # conv1_1_3x3_s2 reads data_sub2 = the image's even pixels
        fx = lambda r0, r1, c0, c1: src[0:1, sub * r0:sub * r1:sub, sub * c0:sub * c1:sub].cpu().numpy()
        fr = None if res is None else (lambda r0, r1, c0, c1: res[0:1, r0:r1, c0:c1].cpu().numpy())
        want = lim.window_oracle(fx, fr, hh, ww, kern, stride, dil, bn, bias, c["relu"], up2, rows, cols)
        got = out[0:1, rows[0]:rows[1], cols[0]:cols[1]].cpu().numpy()
        ne = got.view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)
        assert not ne.any(), "%s: %d of %d window elements differ from the C oracle" % (c["name"], ne.sum(), ne.size)
    label_fwd = logits.argmax(dim=-1).to(torch.uint8)
    del logits
    (s, e), prof = profiled(lambda: net.score(x, "margin", return_label=True))
    for row in ("k_front2<s2>", "k_front2<s1>", "k_conv3x3_c32", "k_conv1x1_up2_c128"):
        assert row in prof, "%s did not run in the score call (profile: %s)" % (row, sorted(prof))
    assert any(r.endswith(",dual>") for r in prof), "no dual launch in the score call: %s" % sorted(prof)
    assert_same_bits("labels: score call vs argmax of the forward logits", e["label"], label_fwd)
