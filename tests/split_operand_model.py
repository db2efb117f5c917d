"""TEST INFRASTRUCTURE ONLY -- a model of the opt-in ``arithmetic="bf16x3"`` mode's OWN arithmetic (csrc/ssal_bottleneck_bf16x3.hip,
csrc/ssal_bf16x3.h), in plain numpy with float64 sums.  It imports nothing from the library; the exact-fp32 parts of the
blocks (max-pool residual, pooling indices, unpool_2d, the batch-norm fold) are the parity oracle's.

One block under the mode, stage by stage as the kernels evaluate it:

  split     x = f1 + f2 + f3 by three truncations to the leading 16 bits (split1 / split_host), each remainder exact in fp32.
            Split sites: every kernel tensor (host, at commit), the block input (registers), the projected tile (stored
            pre-split in LDS), the (5,1) result of the asymmetric block (stored pre-split over the projected tile), the
            convolution output after BN + PReLU (registers, operand of the expansion).
  products  per K = 16 chunk the six products x3w1, x2w2, x1w3, x2w1, x1w2, x1w1 (x = activation term, w = kernel term) are
            summed over the stage's chunks in float64 and rounded to fp32 once: the centre ``value`` of the stage.
  epilogue  prelu1(fmaf(acc, s, t), alpha) with (s, t) = oracle bn_fold; prelu1(fmaf(e, s, t) + residual, alpha) at the end;
            every fmaf is evaluated with ONE rounding (round-to-odd in float64, then to fp32).

``bound`` is a forward bound on |kernel - value| of a correct kernel, propagated with the values:

  convolution stage   bound_out = |W|^T bound_in + allowance.  The allowance walks the stage's MFMA instructions in the
                      kernel's order (chunk by chunk, small terms first) with a running A += sum |x_i||w_j| of the
                      instruction and charges r u A per instruction, u = 2^-24.  r = fp32 roundings one
                      v_mfma_f32_32x32x16_bf16 may make per output element: the products are exact (8 x 8 significant bits), so
                      at most one rounding per product added plus one for the accumulator, R_MFMA = 17; adding an exact zero
                      never rounds, so an output element whose instruction holds n < 16 non-zero products is charged
                      min(17, n + 1) and one with none (a chunk of zeros) nothing; nor is an instruction charged that adds a
                      single non-zero product to an accumulator that is still exact when the sum is an fp32 number.
  fmaf / add / PReLU  pass bound_in through their slope (|s|, 1, max(1, |alpha|)) and add u |result| for the kernel's own
                      rounding -- nothing where bound_in is 0: the same correctly rounded operation on the same inputs gives
                      the same bits.

``drop=(i, j)`` removes the product x_i w_j (1-based, as named above); ``at=(stage, chunk)`` restricts that to one stage
(chunk None) or to one K-chunk of it.  They exist for the CPU tests that prove the GPU cases have teeth.  ``extra`` (a dict)
receives ``anchor``: the same bound with every rounding of the model itself charged plus the dropped terms x2w3 + x3w2 + x3w3
propagated the same way -- what the model may differ from the float64 evaluation of the exact block by."""
import numpy as np

from oracle import enet_oracle as orc

U = 2.0 ** -24
R_MFMA = 17
SIX = ((3, 1), (2, 2), (1, 3), (2, 1), (1, 2), (1, 1))  # (activation term, kernel term), small terms first
_MASK = np.uint32(0xffff0000)


def _trunc(x):
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) & _MASK).view(np.float32)


def split3(x):
    """three fp32 arrays, each with 16 zero low bits, f1 + f2 + f3 == x exactly (split1 / ssal::bf16x3::split_host)"""
    x = np.ascontiguousarray(x, np.float32)
    f1 = _trunc(x)
    r1 = x - f1
    f2 = _trunc(r1)
    r2 = r1 - f2
    return f1, f2, _trunc(r2)


def _terms(x):
    return tuple(t.astype(np.float64) for t in split3(x))


def fma32(a, s, t):
    """fmaf on fp32 arrays with its single rounding: exact product, TwoSum, round-to-odd in float64, then to fp32"""
    a, s, t = np.broadcast_arrays(np.asarray(a, np.float32), np.asarray(s, np.float32), np.asarray(t, np.float32))
    p = a.astype(np.float64) * s.astype(np.float64)
    t = t.astype(np.float64)
    z = p + t
    bb = z - p
    err = (p - (z - bb)) + (t - bb)
    fix = (err != 0) & ((z.view(np.int64) & 1) == 0)
    z = np.where(fix, np.nextafter(z, np.where(err > 0, np.inf, -np.inf)), z)
    return z.astype(np.float32)


class _Act:
    """an activation tensor of the model: fp32 values, bound against a correct kernel, bound against the exact block"""

    def __init__(self, v, b=None, a=None):
        self.v = np.ascontiguousarray(v, np.float32)
        self.b = np.zeros(self.v.shape) if b is None else b
        self.a = np.zeros(self.v.shape) if a is None else a


class _Ctl:
    def __init__(self, drop, at, extra):
        self.drop = tuple(drop) if drop is not None else None
        self.at = at
        self.extra = extra

    def dropped(self, stage, chunk, ij):
        if self.drop is None or ij != self.drop:
            return False
        if self.at is None:
            return True
        return self.at[0] == stage and (self.at[1] is None or self.at[1] == chunk)


def _gemm(act, w, chunks, act_is_a, ctl, stage):
    """act: _Act flattened to [M, K]; w [K, Nc] fp32; chunks: [(chunk id, k indices, column indices or None)] in the kernel's
    order.  act_is_a: the activation is the A operand of mfma6 (else the kernel is).  -> _Act [M, Nc]"""
    m, nc = act.v.shape[0], w.shape[1]
    if ctl.extra is not None and "operands" in ctl.extra:  # the CPU tests look at what met what
        ctl.extra["operands"].append((stage, act.v.copy(), np.array(w, np.float32), chunks))
    xt, wt = _terms(act.v), _terms(w)
    order = SIX if act_is_a else tuple((i, j) for (j, i) in SIX)
    acc = np.zeros((m, nc))
    run = np.zeros((m, nc))
    charge = np.zeros((m, nc))
    lost = np.zeros((m, nc))
    lin_b = np.zeros((m, nc))
    lin_a = np.zeros((m, nc))
    exact = (act.b @ np.abs(w).astype(np.float64)) == 0  # the kernel's accumulator still holds the model's exact partial sum
    for cid, ks, cols in chunks:
        cs = slice(None) if cols is None else cols
        wk = [t[ks][:, cs] for t in wt]
        if not any(t.any() for t in wk):
            continue  # a chunk of zero kernel terms: exact zero products, nothing moves
        xk = [t[:, ks] for t in xt]
        absw = np.abs(w[ks][:, cs]).astype(np.float64)
        lin_b[:, cs] += act.b[:, ks] @ absw
        lin_a[:, cs] += act.a[:, ks] @ absw
        for i, j in order:
            if ctl.dropped(stage, cid, (i, j)):
                continue
            acc[:, cs] += xk[i - 1] @ wk[j - 1]
            a_ij = np.abs(xk[i - 1]) @ np.abs(wk[j - 1])
            nnz = (xk[i - 1] != 0).astype(np.float64) @ (wk[j - 1] != 0).astype(np.float64)
            run[:, cs] += a_ij
            # one non-zero product added to an exact accumulator, the sum an fp32 number: that one addition cannot round
            part = acc[:, cs]
            exact[:, cs] &= (nnz == 0) | ((nnz == 1) & (part.astype(np.float32).astype(np.float64) == part))
            charge[:, cs] += np.where((nnz > 0) & ~exact[:, cs], np.minimum(R_MFMA, nnz + 1), 0) * U * run[:, cs]
        lost[:, cs] += np.abs(xk[1]) @ np.abs(wk[2]) + np.abs(xk[2]) @ np.abs(wk[1]) + np.abs(xk[2]) @ np.abs(wk[2])
    v = (acc + 0.0).astype(np.float32)  # the accumulator starts at +0: a sum of zeros is +0
    return _Act(v, lin_b + charge, lin_a + charge + lost)


def _affine(x, s, t):
    v = fma32(x.v, s, t)
    rnd = U * np.abs(v.astype(np.float64))
    sl = np.abs(np.asarray(s, np.float64))
    return _Act(v, sl * x.b + np.where(x.b > 0, rnd, 0.0), sl * x.a + rnd)


def _add(x, res):
    v = (x.v.astype(np.float64) + np.asarray(res.v, np.float64)).astype(np.float32)
    rnd = U * np.abs(v.astype(np.float64))
    b = x.b + res.b
    return _Act(v, b + np.where(b > 0, rnd, 0.0), x.a + res.a + rnd)


def _prelu(x, alpha):
    alpha = np.broadcast_to(np.asarray(alpha, np.float32), x.v.shape)
    neg = (alpha.astype(np.float64) * x.v.astype(np.float64)).astype(np.float32)
    v = np.where(x.v >= 0, x.v, neg)
    sl = np.maximum(1.0, np.abs(alpha.astype(np.float64)))
    rnd = U * np.abs(v.astype(np.float64))
    may_mul = (x.v < 0) | (np.abs(x.v.astype(np.float64)) <= x.b)
    return _Act(v, sl * x.b + np.where((x.b > 0) & may_mul, rnd, 0.0), sl * x.a + np.where(x.v < 0, rnd, 0.0))


def _bn(P, prefix):
    return orc.bn_fold(P[prefix + "mean"], P[prefix + "variance"], P[prefix + "gamma"], P[prefix + "beta"])


def _flat(x):
    return _Act(x.v.reshape(-1, x.v.shape[-1]), x.b.reshape(-1, x.b.shape[-1]), x.a.reshape(-1, x.a.shape[-1]))


def _unflat(x, shape):
    shape = tuple(shape) + (x.v.shape[-1],)
    return _Act(x.v.reshape(shape), x.b.reshape(shape), x.a.reshape(shape))


def _shift(arr, dy, dx):
    """out[n, y, x] = arr[n, y + dy, x + dx], zero outside (SAME padding of an already projected tensor)"""
    n, h, w, c = arr.shape
    out = np.zeros_like(arr)
    y0, y1 = max(0, -dy), min(h, h - dy)
    x0, x1 = max(0, -dx), min(w, w - dx)
    if y0 < y1 and x0 < x1:
        out[:, y0:y1, x0:x1] = arr[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def _im2col(x, offsets):
    """[N, H, W, C] -> [N H W, taps * C], tap-major"""
    return _Act(*(np.concatenate([_shift(arr, dy, dx) for dy, dx in offsets], axis=-1).reshape(-1, len(offsets) * arr.shape[-1])
                  for arr in (x.v, x.b, x.a)))


def _k16(first_chunk, base, n):
    """n consecutive K = 16 chunks whose k indices start at base; ids first_chunk, first_chunk + 1, ..."""
    return [(first_chunk + c, np.arange(base + 16 * c, base + 16 * c + 16), None) for c in range(n)]


def _expansion(q, we, ctl, act_is_a, kchunks):
    """1x1 expansion, one accumulator per 32-column N-tile nt over kchunks K-chunks: chunk id kchunks * nt + c"""
    chunks = []
    for nt in range(we.shape[1] // 32):
        cols = np.arange(32 * nt, 32 * nt + 32)
        chunks += [(kchunks * nt + c, np.arange(16 * c, 16 * c + 16), cols) for c in range(kchunks)]
    return _gemm(q, we, chunks, act_is_a, ctl, "expansion")


def _finish(ctl, out):
    if ctl.extra is not None:
        ctl.extra["anchor"] = out.a
    return out.v, out.b


def bottleneck(P, name, x, dil=1, asym=False, drop=None, at=None, extra=None):
    """k_bottleneck_bf16x3 / k_bottleneck_asym_bf16x3: x [N, H, W, 128] -> (value fp32, bound float64)"""
    ctl = _Ctl(drop, at, extra)
    x = _Act(x)
    n, h, w, _ = x.v.shape
    s, t = _bn(P, name + ".proj_")
    p = _gemm(_flat(x), P[name + ".proj_kernel"].reshape(128, 32), _k16(0, 0, 8), False, ctl, "projection")
    p = _unflat(_prelu(_affine(p, s, t), P[name + ".proj_alpha"]), (n, h, w))
    if asym:
        col = _im2col(p, [(kh - 2, 0) for kh in range(5)])
        r = _gemm(col, P[name + ".conv_kernel.0"].reshape(160, 32), _k16(0, 0, 10), False, ctl, "convolution")
        col = _im2col(_unflat(r, (n, h, w)), [(0, kw - 2) for kw in range(5)])
        c = _gemm(col, P[name + ".conv_kernel.1"].reshape(160, 32), _k16(10, 0, 10), False, ctl, "convolution")
    else:
        col = _im2col(p, [((kh - 1) * dil, (kw - 1) * dil) for kh in range(3) for kw in range(3)])
        c = _gemm(col, P[name + ".conv_kernel"].reshape(288, 32), _k16(0, 0, 18), False, ctl, "convolution")
    s, t = _bn(P, name + ".conv_")
    q = _prelu(_affine(c, s, t), P[name + ".conv_alpha"])
    s, t = _bn(P, name + ".exp_")
    e = _affine(_expansion(q, P[name + ".exp_kernel"].reshape(32, 128), ctl, True, 2), s, t)
    out = _prelu(_add(e, _flat(x)), P[name + ".residual_alpha"])
    return _finish(ctl, _unflat(out, (n, h, w)))


def bottleneck_down(P, name, x, drop=None, at=None, extra=None):
    """k_downsample_bf16x3: x [N, H, W, 64] -> (value [N, H/2, W/2, 128], bound, argmax); the pooled residual and the
    pooling indices are exact fp32 in the kernel: the oracle's"""
    ctl = _Ctl(drop, at, extra)
    x = np.ascontiguousarray(x, np.float32)
    n, h, w, _ = x.shape
    ho, wo = h // 2, w // 2
    # chunk s = 4 cc + t: tap t = dy * 2 + dx, channels 16 cc .. + 15 (pack_down_layer; the k-slot permutation inside a chunk
    # does not change a sum)
    win = _Act(x.reshape(n, ho, 2, wo, 2, 64).transpose(0, 1, 3, 2, 4, 5).reshape(n * ho * wo, 256))
    chunks = [(4 * cc + tp, np.arange(64 * tp + 16 * cc, 64 * tp + 16 * cc + 16), None) for cc in range(4) for tp in range(4)]
    s, t = _bn(P, name + ".proj_")
    p = _gemm(win, P[name + ".proj_kernel"].reshape(256, 32), chunks, False, ctl, "projection")
    p = _unflat(_prelu(_affine(p, s, t), P[name + ".proj_alpha"]), (n, ho, wo))
    col = _im2col(p, [(kh - 1, kw - 1) for kh in range(3) for kw in range(3)])
    c = _gemm(col, P[name + ".conv_kernel"].reshape(288, 32), _k16(0, 0, 18), False, ctl, "convolution")
    s, t = _bn(P, name + ".conv_")
    q = _prelu(_affine(c, s, t), P[name + ".conv_alpha"])
    s, t = _bn(P, name + ".exp_")
    e = _affine(_expansion(q, P[name + ".exp_kernel"].reshape(32, 128), ctl, False, 2), s, t)
    pool, argmax = orc.maxpool2x2_argmax(x)
    res = np.zeros((n * ho * wo, 128), np.float32)
    res[:, :64] = pool.reshape(-1, 64)
    out = _prelu(_add(e, _Act(res)), P[name + ".residual_alpha"])
    v, b = _finish(ctl, _unflat(out, (n, ho, wo)))
    return v, b, argmax


# parity-stacked transposed-conv kernel (ssal_api.hip: stack_convT): slot -> (tap of the first class, of the second), kh*3+kw
_UP_TAPS = ((0, 1), (2, -1), (6, 7), (8, -1), (3, 4), (5, -1))
_UP_SLOT_SHIFT = ((0, 0), (0, -1), (-1, 0), (-1, -1), (0, 0), (0, -1))  # the slot's projected pixel relative to (i, j)


def stack_conv_t(w):
    """[3, 3, 16, 32] (HW-O-I) -> [6 slots, 32 ci, 32 rows = two parity classes x 16 channels]"""
    ws = np.zeros((6, 32, 32), np.float32)
    flat = np.asarray(w, np.float32).reshape(9, 16, 32)
    for sl, taps in enumerate(_UP_TAPS):
        for half, tp in enumerate(taps):
            if tp >= 0:
                ws[sl, :, 16 * half:16 * half + 16] = flat[tp].T
    return ws


def bottleneck_up(P, name, x, argmax, drop=None, at=None, extra=None):
    """k_upsample_bf16x3: x [N, H, W, 128], argmax [N, H, W, 64] -> (value [N, 2H, 2W, 64], bound); unpool_2d is the oracle's"""
    ctl = _Ctl(drop, at, extra)
    x = _Act(x)
    n, h, w, _ = x.v.shape
    s, t = _bn(P, name + ".proj_")
    p = _gemm(_flat(x), P[name + ".proj_kernel"].reshape(128, 32), _k16(0, 0, 8), False, ctl, "projection")
    p = _unflat(_prelu(_affine(p, s, t), P[name + ".proj_alpha"]), (n, h, w))
    # the 1x1 residual convolution: per N-tile nt one accumulator over chunks c = 0..7, chunk id 2 c + nt; no BN
    wr = P[name + ".res_kernel"].reshape(128, 64)
    chunks = [(2 * c + nt, np.arange(16 * c, 16 * c + 16), np.arange(32 * nt, 32 * nt + 32)) for nt in range(2) for c in range(8)]
    res = _unflat(_gemm(_flat(x), wr, chunks, False, ctl, "residual"), (n, h, w))
    # transposed convolution: accumulator A = [ee | eo] over slots 0..3, B = [oe | oo] over slots 4, 5; chunk id 2 slot + c2
    ws = stack_conv_t(P[name + ".conv_kernel"])
    col = _im2col(p, _UP_SLOT_SHIFT)
    wst = ws.reshape(192, 32)
    acc_a = _gemm(col, wst, [ch for sl in range(4) for ch in _k16(2 * sl, 32 * sl, 2)], False, ctl, "convolution")
    acc_b = _gemm(col, wst, [ch for sl in (4, 5) for ch in _k16(2 * sl, 32 * sl, 2)], False, ctl, "convolution")
    cs, ct = _bn(P, name + ".conv_")
    es, et = _bn(P, name + ".exp_")
    we = P[name + ".exp_kernel"].reshape(16, 64)
    exp_chunks = [(nt, np.arange(16), np.arange(32 * nt, 32 * nt + 32)) for nt in range(2)]
    out = _Act(np.zeros((n, 2 * h, 2 * w, 64), np.float32))
    # unpool_2d: value and both bounds of the residual land where the pooling index points (one output per window and channel)
    argmax = np.ascontiguousarray(argmax, np.int64)
    res_up = _Act(orc.unpool2d(res.v, argmax), np.zeros(out.v.shape), np.zeros(out.v.shape))
    yy, xx = argmax // (2 * w * 64), (argmax // 64) % (2 * w)
    nn, _, _, cc = np.indices(argmax.shape)
    res_up.b[nn, yy, xx, cc] = res.b
    res_up.a[nn, yy, xx, cc] = res.a
    for cls in range(4):  # ee, eo, oe, oo: output pixel (2 i + (cls >> 1), 2 j + (cls & 1))
        acc = acc_a if cls < 2 else acc_b
        rows = slice(16 * (cls & 1), 16 * (cls & 1) + 16)
        q = _prelu(_affine(_Act(acc.v[:, rows], acc.b[:, rows], acc.a[:, rows]), cs, ct), P[name + ".conv_alpha"])
        e = _unflat(_affine(_gemm(q, we, exp_chunks, False, ctl, "expansion"), es, et), (n, h, w))
        sel = (slice(None), slice(cls >> 1, None, 2), slice(cls & 1, None, 2))
        o = _prelu(_add(e, _Act(res_up.v[sel], res_up.b[sel], res_up.a[sel])), P[name + ".residual_alpha"])
        out.v[sel], out.b[sel], out.a[sel] = o.v, o.b, o.a
    return _finish(ctl, out)


# ---- the exact blocks in float64 (what the mode approximates): the anchor of the CPU tests -------------------------------
def _exact_block(P, name, kind, x, dil=1, argmax=None):
    f = np.float64

    def bn_prelu(v, prefix, alpha):
        s, t = _bn(P, name + prefix)
        v = v * s.astype(f) + t.astype(f)
        return v if alpha is None else np.where(v >= 0, v, P[name + alpha].astype(f) * v)

    def conv(v, wk, offsets):
        col = np.concatenate([_shift(v, dy, dx) for dy, dx in offsets], axis=-1)
        return col @ wk.astype(f).reshape(-1, wk.shape[-1])

    x = np.asarray(x, f)
    n, h, w, _ = x.shape
    if kind == "down":
        win = x.reshape(n, h // 2, 2, w // 2, 2, 64).transpose(0, 1, 3, 2, 4, 5).reshape(n, h // 2, w // 2, 256)
        p = win @ P[name + ".proj_kernel"].astype(f).reshape(256, 32)
    else:
        p = x @ P[name + ".proj_kernel"].astype(f).reshape(128, 32)
    p = bn_prelu(p, ".proj_", ".proj_alpha")
    if kind == "asym":
        r = conv(p, P[name + ".conv_kernel.0"], [(kh - 2, 0) for kh in range(5)])
        c = conv(r, P[name + ".conv_kernel.1"], [(0, kw - 2) for kw in range(5)])
    elif kind == "up":
        ws = stack_conv_t(P[name + ".conv_kernel"]).astype(f).reshape(192, 32)
        col = np.concatenate([_shift(p, dy, dx) for dy, dx in _UP_SLOT_SHIFT], axis=-1)
        acc = np.concatenate([col[..., :128] @ ws[:128], col[..., 128:] @ ws[128:]], axis=-1)  # ee | eo | oe | oo
        c = np.zeros((n, 2 * h, 2 * w, 16))
        for cls in range(4):
            c[:, cls >> 1::2, cls & 1::2] = acc[..., 16 * cls:16 * cls + 16]
    else:
        c = conv(p, P[name + ".conv_kernel"], [((kh - 1) * dil, (kw - 1) * dil) for kh in range(3) for kw in range(3)])
    q = bn_prelu(c, ".conv_", ".conv_alpha")
    wexp = P[name + ".exp_kernel"].astype(f)
    e = bn_prelu(q @ wexp.reshape(-1, wexp.shape[-1]), ".exp_", None)
    if kind == "down":
        pool = x.reshape(n, h // 2, 2, w // 2, 2, 64).max(axis=(2, 4))
        res = np.concatenate([pool, np.zeros_like(pool)], axis=-1)
    elif kind == "up":
        r = x @ P[name + ".res_kernel"].astype(f).reshape(128, 64)
        res = np.zeros((n, 2 * h, 2 * w, 64))
        yy, xx = argmax // (2 * w * 64), (argmax // 64) % (2 * w)
        nn, _, _, cc = np.indices(argmax.shape)
        res[nn, yy, xx, cc] = r
    else:
        res = x
    v = e + res
    return np.where(v >= 0, v, P[name + ".residual_alpha"].astype(f) * v)


def exact_bottleneck(P, name, x, dil=1, asym=False):
    return _exact_block(P, name, "asym" if asym else "regular", x, dil=dil)


def exact_bottleneck_down(P, name, x):
    return _exact_block(P, name, "down", x)


def exact_bottleneck_up(P, name, x, argmax):
    return _exact_block(P, name, "up", x, argmax=np.asarray(argmax, np.int64))
