"""TEST INFRASTRUCTURE ONLY -- the 32-bit offset guards of ICNet's convolution launchers, restated as literal predicates, and
the references "on parts" that the large-shape GPU tests compare against.  Nothing here touches a device or parses the library's
source; tests/test_icnet_limits_cpu.py pins the dry query ``_lib.icnet_conv_dispatch`` to the predicates on both sides of every
boundary and proves the part references exact at small shapes, tests/test_gpu_icnet_large_shapes.py runs the boundaries.

Guards (csrc/ssal_icnet_kernels.hip: igemm_choose, launch_igemm_dual, conv_first_fits; ssal_icnet_front.hip: launch_front2;
ssal_icnet_bf16x3.hip: launch_igemm_bf16x3; ssal_icnet_api.hip: check_dims).  H, W are the dims of the tensor in memory."""
import numpy as np

from oracle import enet_oracle as orc
from oracle import icnet_oracle as ico

HT_H, HT_W = 8, 16        # output tile of k_conv3x3_c32 / k_conv1x1_up2_c128
CF_TH, CF_TW = 8, 32      # output tile of k_conv_first
FR_TH, FR_TW = 8, 16      # output tile of k_front2
BX_CHUNK_BYTES = 3072     # one packed bf16x3 chunk: 16 channels x 32 columns x 3 terms x 2 bytes
IGEMM_IN_LIMIT = 2 ** 32 - 16384   # bytes of the input tensor of one launch (the margin: the per-chunk scalar offset)
IGEMM_OUT_LIMIT = 2 ** 32 - 256    # bytes of the output tensor of one launch
IGEMM_M_LIMIT = 2 ** 31 - 256      # output pixels of one launch
API_PIXEL_LIMIT = 2 ** 27          # n * h * w of a network call
REFUSED = "no kernel takes this convolution"
API_REFUSED = "batch too large"


def cdiv(a, b):
    return -(-a // b)


def same_geometry(size, k, stride, dil):
    """TF SAME along one axis: (out, pad_before)"""
    out = cdiv(size, stride)
    return out, max((out - 1) * stride + (k - 1) * dil + 1 - size, 0) // 2


def out_dims(h, w, k, stride, dil, up2):
    hh, ww = (2 * h, 2 * w) if up2 else (h, w)
    return same_geometry(hh, k, stride, dil)[0], same_geometry(ww, k, stride, dil)[0]


def conv1x1_up2_c128_form(cin, cout, k, stride, up2, has_res):
    return k == 1 and cin == 128 and cout <= 32 and stride == 1 and up2 and not has_res


def conv1x1_up2_c128_fits(n, h, w, cout):
    return 4 * h * w * cout * 4 < 2 ** 31 and h * w * 512 < 2 ** 31 and n * cdiv(2 * w, HT_W) * cdiv(2 * h, HT_H) < 2 ** 31


def conv3x3_c32_form(cin, k, stride, dil, up2):
    return k == 3 and cin == 32 and stride == 1 and dil == 1 and not up2


def conv3x3_c32_fits(n, h, w, cout):
    return h * w * max(cout, 32) * 4 < 2 ** 31 and n * cdiv(w, HT_W) * cdiv(h, HT_H) * cdiv(cout, 32) < 2 ** 31


def igemm_fits(n, h, w, cin, cout, k, stride, dil, up2):
    """the launch-wide conditions of k_igemm (every form) and k_igemm_bf16x3"""
    ho, wo = out_dims(h, w, k, stride, dil, up2)
    m = n * ho * wo
    return cin <= 2048 and n * h * w * cin * 4 < IGEMM_IN_LIMIT and m * cout * 4 < IGEMM_OUT_LIMIT and m < IGEMM_M_LIMIT


def igemm_dual_fits(n, h, w, cin, cout, cin_s, stride_s):
    m = n * h * w
    return (max(cin, cin_s) <= 2048 and n * h * stride_s * w * stride_s * cin_s * 4 < IGEMM_IN_LIMIT
            and n * h * w * cin * 4 < IGEMM_IN_LIMIT and m * cout * 4 < IGEMM_OUT_LIMIT and m < IGEMM_M_LIMIT)


def bf16x3_packed_fits(cin, cout, k):
    return k * k * (cin // 16) * cdiv(cout, 32) * BX_CHUNK_BYTES < 2 ** 32 - 16384


def conv_first_fits(n, h, w, sub=1):
    ho, wo = (h // sub + 1) // 2, (w // sub + 1) // 2
    return h >= sub and w >= sub and n * cdiv(wo, CF_TW) * cdiv(ho, CF_TH) < 2 ** 31


def front2_fits(n, h, w, cin, sub, stride2):
    h2, w2 = h // sub // 2 // stride2, w // sub // 2 // stride2
    return n * cdiv(w2, FR_TW) * cdiv(h2, FR_TH) < 2 ** 31 and h * w * cin * 4 < 2 ** 31


def api_admits(n, h, w):
    return n > 0 and h > 0 and w > 0 and h % 32 == 0 and w % 32 == 0 and n * h * w < API_PIXEL_LIMIT


def igemm_nt(n, h, w, cout, k, stride, dil, up2, concurrency=1):
    ho, wo = out_dims(h, w, k, stride, dil, up2)
    tiles_m, nb32 = cdiv(n * ho * wo, 128), cdiv(cout, 32)
    nt = 4 if nb32 % 4 == 0 else 2 if nb32 % 2 == 0 else 1
    while nt > 1 and tiles_m * (nb32 // nt) < 512 // concurrency:
        nt >>= 1
    return nt


def expected(n, h, w, cin, cout, k, stride=1, dil=1, up2=False, has_res=False, arithmetic="f32"):
    """(kernel, NT) as ``_lib.icnet_conv_dispatch`` names them, or None where every launcher refuses the shape"""
    if cin % 32:
        return ("k_conv_first", 0) if conv_first_fits(n, h, w) else None
    if conv1x1_up2_c128_form(cin, cout, k, stride, up2, has_res) and conv1x1_up2_c128_fits(n, h, w, cout):
        return "k_conv1x1_up2_c128", 0
    if conv3x3_c32_form(cin, k, stride, dil, up2) and conv3x3_c32_fits(n, h, w, cout):
        return "k_conv3x3_c32", 0
    if not igemm_fits(n, h, w, cin, cout, k, stride, dil, up2):
        return None
    nt = igemm_nt(n, h, w, cout, k, stride, dil, up2)
    return ("k_igemm_up2" if up2 else "k_igemm_bf16x3" if arithmetic == "bf16x3" else "k_igemm"), nt


def profile_row(kernel, nt):
    """the launch profile's row name of a dry-query answer"""
    return {"k_igemm": "k_igemm<%d>" % nt, "k_igemm_up2": "k_igemm<%d,up2>" % nt,
            "k_igemm_bf16x3": "k_igemm_bf16x3<%d>" % nt}.get(kernel, kernel)


def last_admitted(pred, lo=1):
    """largest v >= lo with pred(v), for a pred that holds up to a threshold"""
    assert pred(lo)
    hi = lo
    while pred(2 * hi):
        hi *= 2
    lo, hi = hi, 2 * hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if pred(mid) else (lo, mid)
    return lo


# ---- the operator on a part of its input ---------------------------------------------------------------------------------------
def axis_plan(size, k, stride, dil, up2, o0, o1):
    """One axis of a convolution on a part.  size: the axis of the tensor in memory; [o0, o1): the output indices wanted.
    -> (i0, i1, oa): run the operator on input[i0:i1]; element j of that run's output is output oa + j of the whole, exactly,
    for every oa + j in [o0, o1).  The margins, per form:
      stride 1            (k - 1) / 2 * dil input rows beyond the wanted outputs at a cut edge (the SAME padding of the part
                          replaces rows that exist in the whole; at an image edge it IS the whole's padding)
      stride 2 (k 3 / 1)  TF SAME pads (size odd: 1, even: 0) before: the part starts on an EVEN row and ends on a row of the
                          parity of `size`, so that its own pad_before is the whole's; one row beyond the last tap where cut
      upsample2x          the convolution sees resize_bilinear(x, 2x): seen row 2 s + 1 = lerp(x[s], x[min(s + 1, last)]), so a part
                          cut below source row s1 - 1 has a wrong last seen row: one extra source row below a cut"""
    seen = 2 * size if up2 else size
    out, pb = same_geometry(seen, k, stride, dil)
    assert 0 <= o0 < o1 <= out and (stride == 1 or (stride == 2 and k in (1, 3) and dil == 1 and not up2))
    a = max(o0 * stride - pb, 0)                                  # first seen row a wanted output reads
    b = min((o1 - 1) * stride - pb + (k - 1) * dil + 1, seen)     # one past the last
    if stride == 2:
        a -= a % 2
        b += (seen - b) % 2
        assert same_geometry(b - a, k, 2, 1)[1] == pb
        return a, b, a // 2
    if up2:
        s0, s1 = a // 2, min((b - 1) // 2 + 2, size)
        return s0, s1, 2 * s0
    return a, b, a


def part_plan(h, w, k, stride, dil, up2, rows, cols):
    """both axes: ((i0, i1, oa) of the rows, the same of the columns)"""
    return axis_plan(h, k, stride, dil, up2, *rows), axis_plan(w, k, stride, dil, up2, *cols)


def bands(ho, parts=4):
    """output row bands of at most a quarter of the image (ragged: the cuts are no multiples of a tile)"""
    step = max(ho // parts - 3, 1)
    cuts = list(range(0, ho, step)) + [ho]
    return [(a, b) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]


def oracle_conv(x, k, stride, dil, bn, bias, res, relu, up2):
    """the C oracle of the operator (tests/test_icnet_gpu.py: _oracle_conv)"""
    if up2:
        x = ico.resize_bilinear(x, 2 * x.shape[1], 2 * x.shape[2])
    y = orc.conv2d_same(x, k, stride=stride, dil=dil)
    if bn is not None:
        s, t = orc.bn_fold(*bn)
        return ico.affine_add_relu(y, s, t, res, relu)
    return ico.affine_add_relu(y, None, bias, res, relu)


def window_oracle(fetch_x, fetch_res, h, w, kern, stride, dil, bn, bias, relu, up2, rows, cols, conv=None):
    """The C oracle on the output window rows x cols of one image.  fetch_x(r0, r1, c0, c1) / fetch_res(...) -> numpy
    [1, r1 - r0, c1 - c0, C] crops of that image's input / residual (fetch_res None: no residual).
    conv: another model of the operator with oracle_conv's signature (returns what it returns, cropped on its leading axes)."""
    k = kern.shape[0]
    (i0, i1, oa), (j0, j1, ob) = part_plan(h, w, k, stride, dil, up2, rows, cols)
    xc = np.ascontiguousarray(fetch_x(i0, i1, j0, j1), np.float32)
    ph, pw = out_dims(i1 - i0, j1 - j0, k, stride, dil, up2)
    rc = None if fetch_res is None else np.ascontiguousarray(fetch_res(oa, oa + ph, ob, ob + pw), np.float32)
    got = (conv or oracle_conv)(xc, kern, stride, dil, bn, bias, rc, relu, up2)
    sl = (slice(None), slice(rows[0] - oa, rows[1] - oa), slice(cols[0] - ob, cols[1] - ob))
    if isinstance(got, tuple):
        return tuple(g[sl] for g in got)
    return got[sl]


def clamp_window(center, length, size):
    """[lo, hi) of `length` outputs around `center`, inside [0, size)"""
    length = min(length, size)
    lo = min(max(center - length // 2, 0), size - length)
    return lo, lo + length


def bn_params(rng, c):
    return (rng.normal(0, 0.1, c).astype(np.float32), rng.uniform(0.5, 1.5, c).astype(np.float32),
            rng.uniform(0.8, 1.2, c).astype(np.float32), rng.normal(0, 0.1, c).astype(np.float32))
