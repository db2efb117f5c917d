"""CPU tests of ICNet's convolution dispatch at the 32-bit offset guards of its kernels (include/ssal_icnet.h:
ssal_icnet_debug_conv_dispatch, a host-only query of the decision launch_igemm and the stand-alone operator make).

Every ICNet inference convolution reaches its tensors through raw buffer resources and 32-bit byte offsets; each launcher admits
the shapes its offset arithmetic can address.  tests/icnet_limits.py restates those guards as literal predicates, independently
of the library; here the dry query is pinned to them on both sides of every boundary, the network entry's own limit is checked
against every layer's launcher, and the references "on parts" of tests/test_gpu_icnet_large_shapes.py (an image of a batch, a
row band, a corner window) are proved exact against the C oracle on the whole input at small shapes."""
import numpy as np
import pytest

import icnet_limits as lim
import icnet_split_model as ism
from semanticsegmentationactivelearning_amd import _lib


def dispatch(n, h, w, cin, cout, k, stride=1, dil=1, up2=False, res=False, arithmetic="f32"):
    """the dry query: (kernel, NT), or None where it refuses with the launchers' message"""
    try:
        return _lib.icnet_conv_dispatch(n, h, w, cin, cout, k, stride, dil, up2, res, arithmetic)
    except ValueError as e:
        assert lim.REFUSED in str(e), str(e)
        return None


def both_sides(form, n, w, fits, arithmetic="f32"):
    """h = the last height `fits` admits at this n, w: -> (h, answer at h, answer at h + 1), each checked against lim.expected"""
    cin, cout, k, stride, dil, up2, res = form
    h = lim.last_admitted(lambda v: fits(n, v, w))
    assert fits(n, h, w) and not fits(n, h + 1, w)
    out = []
    for hh in (h, h + 1):
        got = dispatch(n, hh, w, cin, cout, k, stride, dil, up2, res, arithmetic)
        assert got == lim.expected(n, hh, w, cin, cout, k, stride, dil, up2, res, arithmetic), (form, n, hh, w, got)
        out.append(got)
    return (h,) + tuple(out)


# ---- the fast kernels: last admitted, first refused, and what the first refused shape falls to ----------------------------------
def test_conv1x1_up2_c128_boundary():
    form = (128, 19, 1, 1, 1, True, False)
    for w in (2047, 2045, 2048):
        h, near, above = both_sides(form, 1, w, lambda n, h_, w_: lim.conv1x1_up2_c128_fits(n, h_, w_, 19))
        assert near == ("k_conv1x1_up2_c128", 0) and above == ("k_igemm_up2", 1), (h, w)
        assert h * w * 512 < 2 ** 31 <= (h + 1) * w * 512  # the source image binds (Cout <= 32: 16 Cout <= 512)
    assert dispatch(1, 2048, 2047, 128, 19, 1, up2=True) == ("k_conv1x1_up2_c128", 0)
    assert dispatch(1, 2048, 2048, 128, 19, 1, up2=True) == ("k_igemm_up2", 1)   # H W 512 == 2^31: strict
    # the output condition binds nowhere a source image fits: 4 H W Cout 4 <= H W 512 for Cout <= 32
    assert all(16 * c <= 512 for c in range(1, 33))
    assert dispatch(1, 64, 64, 128, 19, 1, up2=True, res=True) == ("k_igemm_up2", 1)  # a residual: the generic form


@pytest.mark.parametrize("cout,limit", [(32, 2 ** 24), (64, 2 ** 23), (19, 2 ** 24)])
def test_conv3x3_c32_boundary(cout, limit):
    form = (32, cout, 3, 1, 1, False, cout == 64)
    for w in (4095, 2047, 4096):
        h, near, above = both_sides(form, 1, w, lambda n, h_, w_: lim.conv3x3_c32_fits(n, h_, w_, cout))
        assert h * w < limit <= (h + 1) * w
        assert near == ("k_conv3x3_c32", 0), (h, w)
        assert above == ("k_igemm", lim.igemm_nt(1, h + 1, w, cout, 3, 1, 1, False)), (h, w)
    side = int(limit ** 0.5) if cout != 64 else None
    if side:
        assert dispatch(1, side, side - 1, 32, cout, 3) == ("k_conv3x3_c32", 0)
        assert dispatch(1, side, side, 32, cout, 3)[0] == "k_igemm"  # H W == the limit: strict


# ---- k_igemm: the launch-wide limits, exact and bf16x3 ---------------------------------------------------------------------------
IGEMM_FORMS = [
    # (cin, cout, k, stride, dil, up2, res), n, w, the side that binds
    ((32, 32, 1, 1, 1, False, False), 3, 4095, "in"),
    ((32, 128, 1, 1, 1, False, True), 3, 1023, "out"),
    ((64, 64, 3, 1, 2, False, True), 3, 2047, "in"),
    ((32, 64, 3, 2, 1, False, False), 3, 4095, "in"),
    ((256, 128, 3, 1, 2, True, True), 3, 510, "out"),
    ((256, 128, 3, 1, 2, True, True), 3, 511, "out"),
    ((2048, 32, 1, 1, 1, False, False), 1, 511, "in"),
]


@pytest.mark.parametrize("form,n,w,side", IGEMM_FORMS)
@pytest.mark.parametrize("arithmetic", ["f32", "bf16x3"])
def test_igemm_boundary(form, n, w, side, arithmetic):
    cin, cout, k, stride, dil, up2, res = form
    h, near, above = both_sides(form, n, w, lambda n_, h_, w_: lim.igemm_fits(n_, h_, w_, cin, cout, k, stride, dil, up2), arithmetic)
    assert above is None, "first refused shape %dx%dx%d got %r" % (n, h + 1, w, above)
    nt = lim.igemm_nt(n, h, w, cout, k, stride, dil, up2)
    plain = "k_igemm_up2" if up2 else "k_igemm"
    assert dispatch(n, h, w, cin, cout, k, stride, dil, up2, res) == (plain, nt)
    # bf16x3: the split kernel at the same NT exactly where the exact path runs the plain kernel (and the packed kernel fits)
    assert lim.bf16x3_packed_fits(cin, cout, k)
    assert near == (("k_igemm_bf16x3" if arithmetic == "bf16x3" and not up2 else plain), nt)
    ho, wo = lim.out_dims(h, w, k, stride, dil, up2)
    in_bytes, out_bytes = n * h * w * cin * 4, n * ho * wo * cout * 4
    in_next = n * (h + 1) * w * cin * 4
    ho1, wo1 = lim.out_dims(h + 1, w, k, stride, dil, up2)
    if side == "in":
        assert in_bytes < lim.IGEMM_IN_LIMIT <= in_next and out_bytes < lim.IGEMM_OUT_LIMIT
    else:
        assert out_bytes < lim.IGEMM_OUT_LIMIT <= n * ho1 * wo1 * cout * 4 and in_next < lim.IGEMM_IN_LIMIT
    assert max(in_bytes, out_bytes) > 2 ** 31  # offsets with bit 31 set exist


def test_igemm_channel_limit_and_the_unreachable_pixel_limit():
    assert dispatch(1, 8, 8, 2048, 32, 1) == ("k_igemm", 1)
    assert dispatch(1, 8, 8, 2080, 32, 1) is None
    assert dispatch(1, 8, 8, 2048, 32, 1, arithmetic="bf16x3") == ("k_igemm_bf16x3", 1)
    assert dispatch(1, 8, 8, 2080, 32, 1, arithmetic="bf16x3") is None
    # M >= 2^31 - 256 cannot be reached: M Cout 4 < 2^32 - 256 binds first for every Cout >= 1
    for cout in (1, 2, 19, 32, 2048):
        m_out = (lim.IGEMM_OUT_LIMIT - 1) // (4 * cout)  # the largest M the output condition admits
        assert m_out < lim.IGEMM_M_LIMIT
    assert (lim.IGEMM_OUT_LIMIT - 1) // 4 == 2 ** 30 - 65 < lim.IGEMM_M_LIMIT


def test_first_conv_boundary():
    """k_conv_first indexes in 64 bits; its launcher refuses only a grid of 2^31 workgroups (one per 8 x 32 output tile).  The last
    admitted shape holds 2^31 - 1 tiles, at least 140 bytes of input and output each: no device holds it, so the boundary is pinned
    here and the device case runs the largest output the test machine is asked for (above 2^32 bytes)."""
    assert dispatch(1, 8193, 16385, 3, 32, 3, 2) == ("k_conv_first", 0)
    assert lim.conv_first_fits(2 ** 30 - 1, 1, 66) and not lim.conv_first_fits(2 ** 30, 1, 66)   # two tiles per image
    assert dispatch(2 ** 30 - 1, 1, 66, 3, 32, 3, 2) == ("k_conv_first", 0)
    assert dispatch(2 ** 30, 1, 66, 3, 32, 3, 2) is None
    assert dispatch(2 ** 31 - 1, 1, 64, 3, 32, 3, 2) == ("k_conv_first", 0)  # one tile per image: n itself is the limit
    assert (2 ** 31 - 1) * (3 * 4 + 32 * 4) > 288 * 10 ** 9  # bytes of the smallest last-admitted case > the device's memory
    with pytest.raises(ValueError):
        _lib.icnet_conv_dispatch(1, 16, 16, 3, 64, 3, 2)   # not the first-layer form


def test_front2_and_dual_guards_hold_for_every_network_call():
    """launch_front2 refuses H W Cin 4 >= 2^31 and launch_igemm_dual a tensor beyond the launch-wide limits: below the network
    entry's n h w < 2^27 neither can happen (Cin <= 4; the dual launch's largest tensor is conv2_1's 128-channel output at 1/8)"""
    top = lim.API_PIXEL_LIMIT - 1024  # h, w multiples of 32: n h w is a multiple of 1024
    for cin in (1, 3, 4):
        assert top * cin * 4 < 2 ** 31
        assert lim.front2_fits(1, 8192, 16352, cin, 1, 2) and lim.front2_fits(31, 2048, 2048, cin, 2, 1)
    assert not lim.front2_fits(1, 8192, 16384, 4, 1, 2)  # the API refuses this frame first
    for nm, cin, mid, cout, stride, dil, proj in ism._BNECKS:
        if proj:
            div = {"conv2_1": 8, "conv3_1": 16, "conv4_1": 32, "conv5_1": 32}[nm]
            for n, h, w in ((1, 8192, 16352), (31, 2048, 2048)):
                assert lim.igemm_dual_fits(n, h // div, w // div, mid, cout, cin, stride), nm


# ---- the network entry against every layer's launcher ---------------------------------------------------------------------------
NETWORK_SHAPES = [(1, 8192, 16352), (31, 2048, 2048), (1, 4096, 32736), (1, 32, 4194272), (7, 2048, 9344), (4095, 32, 1024),
                  (127, 1024, 1024)]


def test_api_limit_arithmetic():
    assert not lim.api_admits(1, 8192, 16384) and not lim.api_admits(32, 2048, 2048) and not lim.api_admits(2, 8192, 8192)
    for n, h, w in NETWORK_SHAPES:
        assert lim.api_admits(n, h, w), (n, h, w)
        assert n * h * w >= lim.API_PIXEL_LIMIT - 4 * 2 ** 20 or (n, h, w) in ((31, 2048, 2048), (127, 1024, 1024))
    # conv2_sub1's input, the largest tensor of a pass, is 32 bytes per input pixel: the last admitted call leaves it 32 KiB
    # below 4 GiB, inside launch_igemm's limit of 2^32 - 16384
    assert (lim.API_PIXEL_LIMIT - 1024) * 32 == 2 ** 32 - 32768 < lim.IGEMM_IN_LIMIT


@pytest.mark.parametrize("n,h,w", NETWORK_SHAPES)
@pytest.mark.parametrize("arithmetic", ["f32", "bf16x3"])
def test_every_layer_of_an_admitted_call_has_a_kernel(n, h, w, arithmetic):
    """no shape the network entry admits is refused by one of its layers' launchers"""
    for c in ism.icnet_convs():
        hh, ww = h // c["div"], w // c["div"]
        args = (n, hh, ww, c["cin"], c["cout"], c["k"], c["stride"], c["dil"], c["up2"], c["res"] is not None)
        got = dispatch(*args, arithmetic=arithmetic)
        assert got is not None, "%s at %dx%dx%d: the API admits the call, the launcher refuses the layer" % (c["name"], n, h, w)
        assert got == lim.expected(*args, arithmetic=arithmetic), (c["name"], got)


def test_fast_kernels_of_the_network_cases():
    """which per-image guard the two network cases of the GPU file sit under"""
    # one 8192 x 16352 frame: conv1_2 / conv1_3 (1/4) and conv6_cls (source 1/8) keep their fast kernels
    assert dispatch(1, 2048, 4088, 32, 32, 3) == ("k_conv3x3_c32", 0) and dispatch(1, 2048, 4088, 32, 64, 3) == ("k_conv3x3_c32", 0)
    assert dispatch(1, 1024, 2044, 128, 19, 1, up2=True) == ("k_conv1x1_up2_c128", 0)
    assert dispatch(31, 512, 512, 32, 32, 3) == ("k_conv3x3_c32", 0) and dispatch(31, 256, 256, 128, 19, 1, up2=True) == ("k_conv1x1_up2_c128", 0)
    assert 31 * 1024 * 1024 * 32 * 4 > 2 ** 31 and 4096 * 8176 * 32 * 4 > 2 ** 31  # conv2_sub1's input in both


# ---- the references on parts are exact --------------------------------------------------------------------------------------------
PART_FORMS = [
    # (name, cin, cout, k, stride, dil, up2, res, relu, bias), h, w
    (("1x1", 32, 32, 1, 1, 1, False, False, True, False), 21, 27),
    (("3x3", 32, 32, 3, 1, 1, False, True, True, False), 22, 27),
    (("3x3 dil 2", 32, 32, 3, 1, 2, False, True, True, False), 23, 26),
    (("3x3 dil 4", 32, 32, 3, 1, 4, False, False, True, False), 25, 29),
    (("3x3 s2 even", 32, 32, 3, 2, 1, False, False, True, False), 24, 30),
    (("3x3 s2 odd", 32, 32, 3, 2, 1, False, False, True, False), 25, 31),
    (("1x1 s2", 32, 32, 1, 2, 1, False, False, False, False), 25, 30),
    (("3x3 dil 2 up2", 32, 32, 3, 1, 2, True, True, True, False), 12, 15),
    (("1x1 up2 head", 128, 19, 1, 1, 1, True, False, False, True), 11, 14),
    (("first", 3, 32, 3, 2, 1, False, False, True, False), 25, 30),
    (("first odd", 3, 32, 3, 2, 1, False, False, True, False), 24, 31),
]


def _small_case(form, n, h, w, seed):
    name, cin, cout, k, stride, dil, up2, res, relu, bias = form
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, h, w, cin)).astype(np.float32)
    kern = (rng.normal(size=(k, k, cin, cout)) / np.sqrt(k * k * cin)).astype(np.float32)
    bn = None if bias else lim.bn_params(rng, cout)
    b = rng.normal(size=cout).astype(np.float32) if bias else None
    ho, wo = lim.out_dims(h, w, k, stride, dil, up2)
    r = rng.normal(size=(n, ho, wo, cout)).astype(np.float32) if res else None
    return x, kern, bn, b, r, (ho, wo)


def _same(tag, got, want):
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "%s: %d elements differ" % (tag, (got != want).sum())


@pytest.mark.parametrize("form,h,w", PART_FORMS, ids=[f[0][0] for f in PART_FORMS])
def test_part_references_equal_the_oracle_on_the_whole_input(form, h, w):
    name, cin, cout, k, stride, dil, up2, res, relu, bias = form
    x, kern, bn, b, r, (ho, wo) = _small_case(form, 2, h, w, seed=h * 100 + w)
    whole = lim.oracle_conv(x, kern, stride, dil, bn, b, r, relu, up2)
    # an image of the batch
    for i in range(2):
        _same(name + " image", lim.oracle_conv(x[i:i + 1], kern, stride, dil, bn, b, None if r is None else r[i:i + 1], relu, up2),
              whole[i:i + 1])
    img = 1
    fx = lambda r0, r1, c0, c1: x[img:img + 1, r0:r1, c0:c1]
    fr = None if r is None else (lambda r0, r1, c0, c1: r[img:img + 1, r0:r1, c0:c1])
    # row bands (full width), every cut
    covered = 0
    for rows in lim.bands(ho, 4) + [(a, a + 1) for a in range(ho)]:
        got = lim.window_oracle(fx, fr, h, w, kern, stride, dil, bn, b, relu, up2, rows, (0, wo))
        _same("%s band %s" % (name, rows), got, whole[img:img + 1, rows[0]:rows[1]])
        covered += rows[1] - rows[0]
    assert covered == 2 * ho
    # windows: the four corners, the edges, the interior, single elements
    for rows in ((0, 5), (ho - 5, ho), (3, 8), (ho // 2, ho // 2 + 1)):
        for cols in ((0, 6), (wo - 6, wo), (2, 9), (wo // 2, wo // 2 + 1)):
            got = lim.window_oracle(fx, fr, h, w, kern, stride, dil, bn, b, relu, up2, rows, cols)
            _same("%s window %s %s" % (name, rows, cols), got, whole[img:img + 1, rows[0]:rows[1], cols[0]:cols[1]])


def test_part_margins_are_needed():
    """the margins of axis_plan are not slack: one row less at a cut changes the result (so a wrong margin would show)"""
    form = ("3x3 dil 2 up2", 32, 32, 3, 1, 2, True, False, True, False)
    x, kern, bn, b, r, (ho, wo) = _small_case(form, 1, 12, 15, seed=5)
    whole = lim.oracle_conv(x, kern, 1, 2, bn, b, None, True, True)
    i0, i1, oa = lim.axis_plan(12, 3, 1, 2, True, 8, 12)
    assert (i0, i1, oa) == (3, 8, 6)  # seen rows 6 .. 13 -> source rows 3 .. 6 and one more below the cut
    short = lim.oracle_conv(x[:, i0:i1 - 1], kern, 1, 2, bn, b, None, True, True)
    assert not np.array_equal(short[:, 8 - oa:12 - oa], whole[:, 8:12])
    # stride 2 on an odd map: a part that starts on an odd row pads differently
    assert lim.axis_plan(25, 3, 2, 1, False, 5, 9) == (8, 19, 4)
    assert lim.same_geometry(25, 3, 2, 1)[1] == 1 == lim.same_geometry(19 - 8, 3, 2, 1)[1] != lim.same_geometry(18 - 8, 3, 2, 1)[1]
