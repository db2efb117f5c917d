"""TEST INFRASTRUCTURE ONLY -- a model of ONE ICNet convolution under the opt-in ``arithmetic="bf16x3"`` mode
(csrc/ssal_icnet_bf16x3.hip: k_igemm_bf16x3), in plain numpy with float64 sums, built on tests/split_operand_model.py (split3,
the six products, the bound rule of DESIGN.md section 5.4.1, fma32); it imports nothing from the library.

  split     activations (registers, after the fragment read) and the kernel (host, at commit) by split3
  products  K order = taps (kh, kw) ascending, 32-channel chunks ascending inside a tap, two K = 16 steps per chunk -- i.e. K = 16
            steps in ascending (tap, channel) order; per step and output element the six products SIX, summed in float64 over
            the whole K loop and rounded to fp32 once
  epilogue  fmaf(acc, scale, shift) with one rounding (fma32), + res (one fp32 addition), ReLU as ``v > 0 ? v : 0``

``conv`` returns ``(value, bound)``; ``bound`` is section 5.4.1's rule unchanged (running A += sum |x||w| in instruction order,
R_MFMA = 17, min(17, n + 1) for sparse instructions, nothing for all-zero chunks); it is 0 where the kernel must give the
model's bits.  ``drop=(i, j)`` removes the product x_i w_j, ``at=step`` restricts that to one K = 16 step (id = tap * Cin / 16 + c).

The module also lists ICNet's convolutions with their shapes (``icnet_convs``) and restates the convolution launcher's choice of
kernel (``expected_dispatch``), and builds the live-chunk and exact cases of the CPU and GPU tests."""
import numpy as np

import split_operand_model as som
from oracle import enet_oracle as orc

STAGE = "conv"


def same_geometry(h, w, kh, kw, stride, dil):
    """TF SAME: (ho, wo, pad_top, pad_left)"""
    ho, wo = -(-h // stride), -(-w // stride)
    th = max((ho - 1) * stride + (kh - 1) * dil + 1 - h, 0)
    tw = max((wo - 1) * stride + (kw - 1) * dil + 1 - w, 0)
    return ho, wo, th // 2, tw // 2


def im2col(x, kh, kw, stride, dil):
    """[N, H, W, C] -> ([N Ho Wo, KH KW C] tap-major, zero outside the image; (N, Ho, Wo))"""
    n, h, w, c = x.shape
    ho, wo, pt, pl = same_geometry(h, w, kh, kw, stride, dil)
    col = np.zeros((n, ho, wo, kh * kw, c), x.dtype)
    oy, ox = np.arange(ho), np.arange(wo)
    for a in range(kh):
        for b in range(kw):
            iy, ix = oy * stride - pt + a * dil, ox * stride - pl + b * dil
            vy, vx = (iy >= 0) & (iy < h), (ix >= 0) & (ix < w)
            if vy.any() and vx.any():
                col[:, np.flatnonzero(vy)[:, None], np.flatnonzero(vx)[None, :], a * kw + b] = x[:, iy[vy][:, None], ix[vx][None, :]]
    return col.reshape(n * ho * wo, kh * kw * c), (n, ho, wo)


def steps(kh, kw, cin):
    """the K = 16 steps in the kernel's order: (id, k indices of the tap-major K axis, all columns)"""
    return [(t * (cin // 16) + c, np.arange(t * cin + 16 * c, t * cin + 16 * c + 16), None)
            for t in range(kh * kw) for c in range(cin // 16)]


def fold(cout, bn=None, bias=None):
    """(scale, shift) as ssal_icnet_commit folds them: batch-norm (mean, variance, gamma, beta), or scale 1 and the bias"""
    if bn is not None:
        s, t = orc.bn_fold(*bn)
        return np.asarray(s, np.float32), np.asarray(t, np.float32)
    return np.ones(cout, np.float32), (np.zeros(cout, np.float32) if bias is None else np.asarray(bias, np.float32))


def conv(x, k, stride=1, dil=1, bn=None, bias=None, res=None, relu=False, drop=None, at=None, extra=None):
    """k_igemm_bf16x3 + its epilogue: x [N, H, W, Cin] fp32, k [KH, KW, Cin, Cout] -> (value fp32 [N, Ho, Wo, Cout], bound)"""
    x, k = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(k, np.float32)
    kh, kw, cin, cout = k.shape
    assert cin % 32 == 0 and x.shape[-1] == cin
    ctl = som._Ctl(drop, None if drop is None else (STAGE, at), extra)
    col, (n, ho, wo) = im2col(x, kh, kw, stride, dil)
    acc = som._gemm(som._Act(col), k.reshape(kh * kw * cin, cout), steps(kh, kw, cin), True, ctl, STAGE)
    s, t = fold(cout, bn, bias)
    out = som._affine(acc, s, t)
    if res is not None:
        out = som._add(out, som._Act(np.asarray(res, np.float32).reshape(-1, cout)))
    if relu:  # v > 0 ? v : +0: 1-Lipschitz, no rounding
        out = som._Act(np.where(out.v > 0, out.v, np.float32(0.0)), out.b, out.a)
    if extra is not None:
        extra["anchor"] = out.a.reshape(n, ho, wo, cout)
    return out.v.reshape(n, ho, wo, cout), out.b.reshape(n, ho, wo, cout)


def exact64(x, k, stride=1, dil=1, bn=None, bias=None, res=None, relu=False):
    """the same convolution in float64 (what the mode approximates)"""
    k = np.asarray(k, np.float64)
    kh, kw, cin, cout = k.shape
    col, (n, ho, wo) = im2col(np.asarray(x, np.float64), kh, kw, stride, dil)
    s, t = fold(cout, bn, bias)
    v = (col @ k.reshape(-1, cout)) * s.astype(np.float64) + t.astype(np.float64)
    if res is not None:
        v = v + np.asarray(res, np.float64).reshape(-1, cout)
    return (np.maximum(v, 0.0) if relu else v).reshape(n, ho, wo, cout)


# ---- cases with teeth (tests/test_icnet_bf16x3_cpu.py proves them, tests/test_gpu_icnet_bf16x3.py runs them) ------------------
from split_operand_cases import FAMILY, rich, unit_variance  # noqa: E402

CASE_SHAPE = (1, 9, 15)                     # M = 135: one full 128-row tile and a 7-row tail
CASE_CONVS = ((3, 64, 32), (1, 96, 32))     # (k, Cin, Cout): 36 and 6 K = 16 steps
LIVE_CASES = [(k, cin, cout, st) for k, cin, cout in CASE_CONVS for st in range(k * k * cin // 16)]
EXACT_CASES = list(CASE_CONVS)


def identity_bn(cout):
    """batch-norm vectors that fold to scale 1, shift 0 exactly"""
    return (np.zeros(cout, np.float32), np.full(cout, unit_variance(), np.float32), np.ones(cout, np.float32),
            np.zeros(cout, np.float32))


def _selector_rows(kk, cout, avoid=None):
    """one K index per output column, spread over the K axis, none inside K = 16 step `avoid`"""
    rows = (np.arange(cout) * 37 + 11) % kk
    if avoid is not None:
        inside = rows // 16 == avoid
        rows[inside] = (rows[inside] + 16) % kk
    return rows


def live_case(k, cin, cout, step):
    """-> (x, kernel): all-positive data whose second and third split terms are large, K = 16 step `step` dense, and in the rest
    ONE three-term selector weight per output column (every further instruction that adds to the accumulator after the dense
    step is charged 2 u A by the bound rule: one selector per column keeps 2 x bound below the smallest of the six products)"""
    rng = np.random.default_rng(1000 * k + cin + 7 * step)
    kk = k * k * cin
    w = np.zeros((kk, cout), np.float32)
    w[16 * step:16 * step + 16] = rich(rng, (16, cout), -4, -3)
    w[_selector_rows(kk, cout, avoid=step), np.arange(cout)] = rich(rng, (cout,), -4, -3)
    x = rich(rng, CASE_SHAPE + (cin,), -1, 1)
    return x, w.reshape(k, k, cin, cout)


def exact_case(k, cin, cout):
    """-> (x, kernel): one selector weight FAMILY per output column, data +-FAMILY 2^e: every subset of the six products is an
    fp32 number, the bound is 0, and the value differs from the exact fp32 product wherever a selector reaches the image"""
    rng = np.random.default_rng(77 * k + cin)
    kk = k * k * cin
    w = np.zeros((kk, cout), np.float32)
    w[_selector_rows(kk, cout), np.arange(cout)] = FAMILY
    shape = CASE_SHAPE + (cin,)
    e = rng.integers(-3, 4, shape).astype(np.float32)
    sign = np.where(rng.integers(0, 2, shape) > 0, np.float32(1), np.float32(-1))
    return (sign * FAMILY * np.exp2(e)).astype(np.float32), w.reshape(k, k, cin, cout)


# ---- ICNet's convolutions and the launcher's rule, restated ------------------------------------------------------------------
_BNECKS = (("conv2_1", 64, 32, 128, 1, 1, True), ("conv2_2", 128, 32, 128, 1, 1, False), ("conv2_3", 128, 32, 128, 1, 1, False),
           ("conv3_1", 128, 64, 256, 2, 1, True), ("conv3_2", 256, 64, 256, 1, 1, False), ("conv3_3", 256, 64, 256, 1, 1, False),
           ("conv3_4", 256, 64, 256, 1, 1, False), ("conv4_1", 256, 128, 512, 1, 2, True), ("conv4_2", 512, 128, 512, 1, 2, False),
           ("conv4_3", 512, 128, 512, 1, 2, False), ("conv4_4", 512, 128, 512, 1, 2, False), ("conv4_5", 512, 128, 512, 1, 2, False),
           ("conv4_6", 512, 128, 512, 1, 2, False), ("conv5_1", 512, 256, 1024, 1, 4, True),
           ("conv5_2", 1024, 256, 1024, 1, 4, False), ("conv5_3", 1024, 256, 1024, 1, 4, False))


def icnet_convs(c_in=3, classes=19):
    """every convolution of the per-layer (forward) schedule (ICNET_SPEC.md; ssal_icnet_api.hip: run_trunk): dicts with name, k,
    cin, cout, stride, dil, div (the input tensor is [n, h / div, w / div, cin]), up2, src / res (endpoint names; src None = the
    image), relu"""
    out = []

    def add(name, k, cin, cout, div, src, stride=1, dil=1, up2=False, res=None, relu=True):
        out.append(dict(name=name, k=k, cin=cin, cout=cout, stride=stride, dil=dil, div=div, up2=up2, src=src, res=res, relu=relu))

    add("conv1_1_3x3_s2", 3, c_in, 32, 2, None, stride=2)
    add("conv1_2_3x3", 3, 32, 32, 4, "conv1_1_3x3_s2")
    add("conv1_3_3x3", 3, 32, 64, 4, "conv1_2_3x3")
    cur, div = "pool1_3x3_s2", 8
    for i, (nm, cin, mid, cout, stride, dil, proj) in enumerate(_BNECKS):
        if i == 4:
            cur, div = "conv3_1_sub4", 32
        odiv = div * stride
        shortcut = cur
        if proj:
            add(nm + "_1x1_proj", 1, cin, cout, div, cur, stride=stride, relu=False)
            shortcut = nm + "_1x1_proj"
        add(nm + "_1x1_reduce", 1, cin, mid, div, cur, stride=stride)
        add(nm + "_3x3", 3, mid, mid, odiv, nm + "_1x1_reduce", dil=dil)
        add(nm + "_1x1_increase", 1, mid, cout, odiv, nm + "_3x3", res=shortcut)
        cur, div = nm, odiv
    add("conv5_4_k1", 1, 1024, 256, 32, "conv5_3_sum")
    add("conv1_sub1", 3, c_in, 32, 1, None, stride=2)
    add("conv2_sub1", 3, 32, 32, 2, "conv1_sub1", stride=2)
    add("conv3_sub1", 3, 32, 64, 4, "conv2_sub1", stride=2)
    add("conv3_1_sub2_proj", 1, 256, 128, 16, "conv3_1", relu=False)
    add("conv_sub4", 3, 256, 128, 32, "conv5_4_k1", dil=2, up2=True, res="conv3_1_sub2_proj")
    add("conv3_sub1_proj", 1, 64, 128, 8, "conv3_sub1", relu=False)
    add("conv_sub2", 3, 128, 128, 16, "sub24_sum", dil=2, up2=True, res="conv3_sub1_proj")
    add("conv6_cls", 1, 128, classes, 8, "sub12_sum", up2=True, relu=False)
    return out


OUTPUT_OF = {"conv_sub4": "sub24_sum", "conv_sub2": "sub12_sum"}  # endpoint that holds a convolution's output, where not its name


def output_endpoint(name):
    return OUTPUT_OF.get(name, name[:-len("_1x1_increase")] if name.endswith("_1x1_increase") else name)


def expected_dispatch(n, h, w, cin, cout, k, stride, dil, up2, has_res, arithmetic="f32", concurrency=1):
    """(kernel name, NT): the convolution launcher's rule (ssal_icnet_kernels.hip: launch_igemm) restated from its text;
    bf16x3 replaces the plain implicit-GEMM kernel and nothing else"""
    if cin % 32:
        return "k_conv_first", 0
    if k == 1 and cin == 128 and cout <= 32 and stride == 1 and up2 and not has_res:
        return "k_conv1x1_up2_c128", 0
    if k == 3 and cin == 32 and stride == 1 and dil == 1 and not up2:
        return "k_conv3x3_c32", 0
    hh, ww = (2 * h, 2 * w) if up2 else (h, w)
    ho, wo, _, _ = same_geometry(hh, ww, k, k, stride, dil)
    tiles_m = -(-(n * ho * wo) // 128)
    nb32 = -(-cout // 32)
    nt = 4 if nb32 % 4 == 0 else 2 if nb32 % 2 == 0 else 1
    while nt > 1 and tiles_m * (nb32 // nt) < 512 // concurrency:
        nt >>= 1
    if up2:
        return "k_igemm_up2", nt
    return ("k_igemm_bf16x3" if arithmetic == "bf16x3" else "k_igemm"), nt


def pack_layout(kernel):
    """the pre-split kernel as bf16x3::pack_igemm lays it out: uint32 [tap][Cin/16][CoutP/32][term][lane][4 dwords], dword m of
    lane (j = lane & 31, h = lane >> 5) = bf16 terms of ci = 16 c + 8 h + 2 m (low half) and + 2 m + 1 (high half), co = 32 nt + j"""
    kernel = np.ascontiguousarray(kernel, np.float32)
    kh, kw, cin, cout = kernel.shape
    nb32 = -(-cout // 32)
    wp = np.zeros((kh * kw, cin, nb32 * 32), np.float32)
    wp[:, :, :cout] = kernel.reshape(kh * kw, cin, cout)
    terms = np.stack([t.view(np.uint32) >> 16 for t in som.split3(wp)])             # [term][tap][ci][co]
    t6 = terms.reshape(3, kh * kw, cin // 16, 2, 4, 2, nb32, 32)                    # term, tap, c, h, m, half, nt, j
    dw = t6[:, :, :, :, :, 0] | (t6[:, :, :, :, :, 1] << 16)                        # term, tap, c, h, m, nt, j
    return np.ascontiguousarray(dw.transpose(1, 2, 5, 0, 3, 6, 4)).reshape(kh * kw, cin // 16, nb32, 3, 64, 4)
