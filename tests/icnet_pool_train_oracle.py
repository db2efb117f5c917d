"""TEST INFRASTRUCTURE ONLY -- never imported by the product.

Float64 restatement of the training step of ICNet through its pyramid pooling, from ``conv5_3_3x3``,
``conv5_2``, ``conv3_1`` and ``conv3_sub1`` to the loss:
  * ``conv5_3 = relu(BN(conv5_3_3x3 @ kernel) + conv5_2)``: the increase layer of the last bottleneck, 1 x 1, 256 -> 1024,
    under inference batch-norm, with the identity shortcut;
  * ``conv5_3_sum = conv5_3 + sum_b resize(bin averages of level b)``, b in (1, 2, 3, 6): the pyramid pooling, written here
    with slices, means and index gathers (``ppm_forward``);
  * the pyramid head on it: ``icnet_pyramid_train_oracle``'s restatement.
Autograd supplies the gradients (``relu'(0) = 0``); ``pool_backward`` restates the new backward pass term by term, the way the
kernels compute it -- the pooling adjoint from explicit per-level matrices (``level_matrices``), written independently of
``ppm_forward`` -- and can leave one step out or get it wrong (the discrimination test).  The twenty variables are packed as the
product packs them: the increase layer's three, then ``icnet_pyramid_train_oracle``'s seventeen.
"""
import numpy as np
import torch
import torch.nn.functional as F

import final_train_oracle as fto
import icnet_cascade_train_oracle as ico
import icnet_fusion_train_oracle as ifo
import icnet_head_train_oracle as iho
import icnet_pyramid_train_oracle as ipo

LAYER = "conv5_3_1x1_increase"
BLOCK = (LAYER + ".kernel", LAYER + ".gamma", LAYER + ".beta")
NAMES = BLOCK + ipo.NAMES
KERNELS = (BLOCK[0],) + ipo.KERNELS  # what the l1_l2 regulariser reaches
BLOCK_FLOATS = 256 * 1024 + 2 * 1024
STATS_OWN = 2 * 1024
LEVELS = (1, 2, 3, 6)
PIXEL_TILE = ipo.PIXEL_TILE  # pixels of conv5_3 per split-K tile of k_icnet_pyramid_wgrad<256, 1024>
MAX_WG = ipo.MAX_WG          # split-K groups of that launch
K1_CHAIN = 256               # products k_icnet_pool_dx adds one after the other on one accumulator
EPS = ifo.EPS
# one step of the backward pass left out or done the wrong way
WRONG = ("no_relu_mask", "identity_only", "pooled_only", "floor_bins", "no_count", "half_pixel", "no_s1")
# mistakes of the weight-gradient, fold and gamma kernels themselves (icnet_pyramid_train_oracle.WRONG_LOCAL's)
WRONG_LOCAL = ("drop_last_pixel", "drop_last_group", "no_mean_term", "kernel_10_percent")


def shapes(k):
    return ((1, 1, 256, 1024), (1024,), (1024,)) + ipo.shapes(k)


def offsets(k):
    out, lo = {}, 0
    for name, shp in zip(NAMES, shapes(k)):
        out[name] = (lo, lo + int(np.prod(shp)))
        lo = out[name][1]
    return out


def floats(k):
    return BLOCK_FLOATS + ipo.floats(k)


def classes_of(packed):
    return ipo.classes_of(np.asarray(packed)[BLOCK_FLOATS:])


def unpack(packed, k=None):
    packed = np.asarray(packed)
    k = classes_of(packed) if k is None else k
    off = offsets(k)
    return {n: packed[off[n][0]:off[n][1]].reshape(s) for n, s in zip(NAMES, shapes(k))}


def pack(d):
    return np.concatenate([np.asarray(d[n]).reshape(-1) for n in NAMES])


def split_stats(stats):
    """[2 * 1024 + ...] -> mean, variance of the increase layer (float64 torch) and the pyramid trainer's rows (numpy)"""
    stats = np.asarray(stats, dtype=np.float64)
    return torch.as_tensor(stats[:1024]), torch.as_tensor(stats[1024:2048]), stats[2048:]


def draw_stats(seed):
    """moving statistics for the gradient cases: the increase layer's two rows of 1024, then the pyramid trainer's"""
    rng = np.random.default_rng(seed + 1000)
    own = [rng.uniform(-0.3, 0.3, 1024), rng.uniform(0.5, 2.0, 1024)]
    return np.concatenate(own + [ipo.draw_stats(seed)]).astype(np.float32)


def case(seed, n, h, w, k):
    """the arrays of one gradient case: ``conv5_3_3x3`` and ``conv5_2`` >= 0 (ReLU outputs) and an increase kernel of both signs
    sized so that conv5_3's pre-activation has both signs over the shortcut; the rest as the pyramid test draws it"""
    _, c31, c3, d17, labels, mask = ipo.case(seed, n, h, w, k)
    rng = np.random.default_rng(seed + 77)
    a = np.abs(rng.standard_normal((n, h, w, 256)) * 0.7).astype(np.float32)
    c52 = np.abs(rng.standard_normal((n, h, w, 1024)) * 0.3).astype(np.float32)
    d = {BLOCK[0]: rng.uniform(-0.08, 0.08, (1, 1, 256, 1024)).astype(np.float32),
         BLOCK[1]: rng.uniform(0.5, 1.5, 1024).astype(np.float32), BLOCK[2]: rng.uniform(-0.5, 0.1, 1024).astype(np.float32)}
    d.update(d17)
    return a, c52, c31, c3, d, labels, mask


# ---- the pyramid pooling, forward (slices, means, gathers) ----
def _legacy_taps(size, bins):
    """(t0, t1, l) of the legacy mapping of ``size`` pixels onto ``bins`` values, the source position formed in fp32 as the
    forward kernel forms it: src = o * (bins / size), t0 = floor, t1 = min(t0 + 1, bins - 1), l = src - t0"""
    src = np.arange(size, dtype=np.float32) * (np.float32(bins) / np.float32(size))
    t0 = np.floor(src).astype(np.int64)
    t1 = np.minimum(t0 + 1, bins - 1)
    return t0, t1, (src - t0.astype(np.float32)).astype(np.float64)


def ppm_forward(x):
    """x [N, h, w, C] (torch float64) -> conv5_3_sum: x + the four resized bin-average maps, in tf.add_n order"""
    _, h, w, _ = x.shape
    out = x
    for b in LEVELS:
        rows = []
        for i in range(b):
            y0, y1 = (i * h) // b, -(-(i + 1) * h // b)
            rows.append(torch.stack([x[:, y0:y1, (j * w) // b:-(-(j + 1) * w // b)].mean((1, 2)) for j in range(b)], 1))
        v = torch.stack(rows, 1)  # [N, b, b, C]
        ya, yb, ly = _legacy_taps(h, b)
        xa, xb, lx = _legacy_taps(w, b)
        lx_t, ly_t = torch.as_tensor(lx)[None, None, :, None], torch.as_tensor(ly)[None, :, None, None]
        hor = v[:, :, xa] + (v[:, :, xb] - v[:, :, xa]) * lx_t
        out = out + (hor[:, ya] + (hor[:, yb] - hor[:, ya]) * ly_t)
    return out


# ---- the pyramid pooling, as matrices (the adjoint's side; independent of ppm_forward) ----
def _resize_matrix(size, bins, half_pixel=False):
    """[size, bins]: row o holds what pixel o reads of each bin value"""
    if half_pixel:
        eye = torch.eye(bins, dtype=torch.float64)[None]  # [1, bins (channel), bins (length)]
        if bins == 1:
            return np.ones((size, 1))
        return F.interpolate(eye, size=size, mode="linear", align_corners=False)[0].numpy().T.copy()
    m = np.zeros((size, bins))
    for o in range(size):
        src = np.float32(o) * (np.float32(bins) / np.float32(size))
        t0 = int(np.floor(src))
        t1 = min(t0 + 1, bins - 1)
        l = float(src - np.float32(t0))
        if t0 == t1:
            m[o, t0] = 1.0
        else:
            m[o, t0], m[o, t1] = 1.0 - l, l
    return m


def _member_matrix(size, bins, floor_bins=False):
    """[bins, size] of 0 / 1: bin i holds pixels [floor(i size / bins), ceil((i + 1) size / bins))"""
    m = np.zeros((bins, size))
    for i in range(bins):
        lo = (i * size) // bins
        hi = ((i + 1) * size) // bins if floor_bins else -(-(i + 1) * size // bins)
        m[i, lo:hi] = 1.0
    return m


def level_matrices(b, h, w, wrong=None):
    """(R [h w, b b], A [b b, h w]) of one level: conv5_3_sum's term of the level is R (A x)"""
    R = np.kron(_resize_matrix(h, b, wrong == "half_pixel"), _resize_matrix(w, b, wrong == "half_pixel"))
    M = np.kron(_member_matrix(h, b, wrong == "floor_bins"), _member_matrix(w, b, wrong == "floor_bins"))
    cnt = M.sum(1, keepdims=True)
    A = M if wrong == "no_count" else M / np.maximum(cnt, 1.0)
    return R, A


def ppm_adjoint(dsum, wrong=None):
    """dL/dconv5_3 (in front of the ReLU mask) from dL/dconv5_3_sum [N, h, w, C] numpy float64"""
    n, h, w, c = dsum.shape
    flat = dsum.reshape(n, h * w, c)
    out = np.zeros_like(flat) if wrong == "pooled_only" else flat.copy()
    if wrong != "identity_only":
        for b in LEVELS:
            R, A = level_matrices(b, h, w, wrong)
            gb = np.einsum("pq,npc->nqc", R, flat)       # the bin gradients: the adjoint of the resize
            out = out + np.einsum("qp,nqc->npc", A, gb)  # spread over each bin's pixels
    return out.reshape(n, h, w, c)


def bins_per_pixel(h, w):
    """the most bins of all four levels that one pixel lies in: the adds of k_icnet_ppm_adj_sum behind the identity term"""
    tot = np.zeros((h, w))
    for b in LEVELS:
        tot += np.outer(_member_matrix(h, b).sum(0), _member_matrix(w, b).sum(0))
    return int(tot.max())


# ---- forward and loss ----
def _tensors(a, c52, c31, c3, packed, grad=True):
    W = {n: torch.as_tensor(np.asarray(v, dtype=np.float64).copy()).requires_grad_(grad) for n, v in unpack(packed).items()}
    t = lambda x: torch.as_tensor(np.asarray(x, dtype=np.float64))
    return t(a), t(c52), t(c31), t(c3), W


def _pre53(xa, x52, W, m, v):
    s = W[BLOCK[1]] / torch.sqrt(v + EPS)
    return (xa @ W[BLOCK[0]].reshape(256, 1024)) * s + (W[BLOCK[2]] - m * s) + x52


def pool_forward(a, c52, c31, c3, packed, stats):
    """-> (conv5_3, conv5_3_sum, conv5_4_k1, sub24_sum, sub12_sum, full-resolution logits) float64 numpy"""
    xa, x52, _, _, W = _tensors(a, c52, c31, c3, packed, grad=False)
    m, v, pstats = split_stats(stats)
    c53 = torch.relu(_pre53(xa, x52, W, m, v))
    s53 = ppm_forward(c53).numpy()
    return (c53.numpy(), s53) + ipo.pyramid_forward(s53, c31, c3, np.asarray(packed)[BLOCK_FLOATS:], pstats)


def _loss(xa, x52, x31, x3, W, stats, labels, mask, weight, label_smoothing, acts=None, keep=None):
    """the float64 loss as a torch scalar.  ``acts``: (conv5_3, conv5_3_sum, conv5_4_k1, sub24_sum, sub12_sum, logits) in fp32 --
    the ReLUs, the pooling sum and the loss are evaluated at those values, the point the GPU evaluates.  ``keep``: a dict that
    receives conv5_4_k1 and conv5_3_sum (gradients retained) and the float64 conv5_3"""
    acts = (None,) * 6 if acts is None else acts
    m, v, pstats = split_stats(stats)
    c53 = ico._pinned_relu(_pre53(xa, x52, W, m, v), acts[0])
    s53 = ppm_forward(c53)
    if acts[1] is not None:
        s53 = s53 + (torch.as_tensor(np.asarray(acts[1], dtype=np.float64)) - s53).detach()
    inner = {} if keep is not None else None
    loss = ipo._loss(s53, x31, x3, W, pstats, labels, mask, weight, label_smoothing, acts[2], acts[3], acts[4], acts[5], inner)
    if keep is not None:
        s53.retain_grad()
        inner["f1"].retain_grad()
        keep["c53"], keep["s53"], keep["f1"] = c53, s53, inner["f1"]
    return loss


def loss_and_grad(a, c52, c31, c3, packed, stats, labels, mask, weight, label_smoothing, acts=None):
    """float64 (loss, packed gradient)"""
    xa, x52, x31, x3, W = _tensors(a, c52, c31, c3, packed)
    loss = _loss(xa, x52, x31, x3, W, stats, labels, mask, weight, label_smoothing, acts)
    loss.backward()
    return float(loss.detach()), pack({n: W[n].grad.numpy() for n in NAMES})


def pool_backward(a, c52, c31, c3, packed, stats, labels, mask, weight, label_smoothing, acts=None, wrong=None):
    """the increase layer's three gradients restated the way the kernels compute them, from autograd's dL/dconv5_4_k1:
    g32 = relu'(conv5_4_k1) dL/dconv5_4_k1; dsum = (s1 g32) K1^T; d53 = dsum + the pooling adjoint by ``level_matrices``;
    g53 = relu'(conv5_3) d53; dK = s a^T g53, dBeta = sum_p g53, dGamma contracted from the folded weight gradient.
    ``wrong``: one of ``WRONG`` or ``WRONG_LOCAL``.  -> {name: float64 array} for ``BLOCK``"""
    assert wrong is None or wrong in WRONG + WRONG_LOCAL
    xa, x52, x31, x3, W = _tensors(a, c52, c31, c3, packed)
    keep = {}
    _loss(xa, x52, x31, x3, W, stats, labels, mask, weight, label_smoothing, acts, keep).backward()
    f1 = keep["f1"].detach().numpy()
    g32 = keep["f1"].grad.numpy() * (f1 > 0)
    Wn = {n: v.detach().numpy() for n, v in W.items()}
    stats = np.asarray(stats, dtype=np.float64)
    m, v = stats[:1024], stats[1024:2048]
    v1 = stats[STATS_OWN + 256:STATS_OWN + 512]
    s1 = Wn["conv5_4_k1.gamma"] / np.sqrt(v1 + EPS)
    gs = g32 if wrong == "no_s1" else g32 * s1
    dsum = gs @ Wn["conv5_4_k1.kernel"].reshape(1024, 256).T
    d53 = ppm_adjoint(dsum, wrong)
    c53 = keep["c53"].detach().numpy()
    g53 = d53 if wrong == "no_relu_mask" else d53 * (c53 > 0)
    x = np.asarray(a, dtype=np.float64).reshape(-1, 256)
    g = g53.reshape(-1, 1024)
    if wrong == "drop_last_pixel":
        x, g = x[:-1], g[:-1]
    if wrong == "drop_last_group":
        x, g = x[:64], g[:64]
    rstd = 1.0 / np.sqrt(v + EPS)
    K = Wn[BLOCK[0]].reshape(256, 1024)
    raw = x.T @ g
    if wrong == "kernel_10_percent":
        raw = 1.1 * raw
    mean = 0.0 if wrong == "no_mean_term" else m
    return {BLOCK[0]: (raw * (Wn[BLOCK[1]] * rstd)).reshape(1, 1, 256, 1024),
            BLOCK[1]: ((K * raw).sum(0) - mean * g.sum(0)) * rstd, BLOCK[2]: g.sum(0)}


def grad_and_bound(a, c52, c31, c3, packed, stats, labels, mask, weight, label_smoothing, acts):
    """(g64, C, loss64), packed: the float64 gradient at the fp32 activations, and the same contraction over absolute values.
    ``icnet_pyramid_train_oracle.grad_and_bound``'s, with |conv5_3_sum| (fp32) as the pyramid head's input and one more term
    under conv5_4_k1's alive units: its |K1| pull-back through the pyramid pooling (whose weights are all >= 0: it is its own
    magnitude) onto the alive units of conv5_3, contracted there with
      kernel   |s| sum_p |a| gabs53     beta   sum_p gabs53     gamma   rstd sum_p gabs53 (|a| @ |K| + |mean|)."""
    c53_32, s53_32, f1_32, sub24_32, sub12_32, logits32 = acts
    k = classes_of(packed)
    loss, g = loss_and_grad(a, c52, c31, c3, packed, stats, labels, mask, weight, label_smoothing, acts)
    ab = ifo.pixel_bound(logits32, labels, mask, k, weight, label_smoothing)
    xa, _, x31, x3, W = _tensors(np.abs(a), np.abs(c52), np.abs(c31), np.abs(c3), np.abs(np.asarray(packed)), grad=False)
    V = {n: torch.zeros(s, dtype=torch.float64, requires_grad=True) for n, s in zip(NAMES, shapes(k))}
    m0, v0, pstats = split_stats(stats)
    m1, v1, cstats = ipo.split_stats(pstats)
    mc, vc, md, vd, fstats = ico.split_stats(cstats)
    ma, va, mb, vb = ifo.split_stats(fstats)
    r0, r1, rc, rd, ra, rb = (1.0 / torch.sqrt(v + EPS) for v in (v0, v1, vc, vd, va, vb))
    P, B, N = ipo.BLOCK, ico.BLOCK, ifo.NAMES
    absf = lambda t: torch.as_tensor(np.abs(np.asarray(t, dtype=np.float64)))
    alive = lambda t: torch.as_tensor((np.asarray(t) > 0).astype(np.float64))
    lin53 = ((xa @ V[BLOCK[0]].reshape(256, 1024)) * (W[BLOCK[1]] * r0)
             + V[BLOCK[1]] * r0 * (xa @ W[BLOCK[0]].reshape(256, 1024) + m0.abs()) + V[BLOCK[2]])
    x53 = absf(s53_32)
    lin32 = ((ppm_forward(alive(c53_32) * lin53) @ W[P[0]].reshape(1024, 256)) * (W[P[1]] * r1)
             + (x53 @ V[P[0]].reshape(1024, 256)) * (W[P[1]] * r1)
             + V[P[1]] * r1 * (x53 @ W[P[0]].reshape(1024, 256) + m1.abs()) + V[P[2]])
    u1 = iho.resize_legacy(absf(f1_32), 2)
    lin24 = (ifo.conv_dilated(iho.resize_legacy(alive(f1_32) * lin32, 2), W[B[0]]) * (W[B[1]] * rc)
             + ifo.conv_dilated(u1, V[B[0]]) * (W[B[1]] * rc)
             + V[B[1]] * rc * (ifo.conv_dilated(u1, W[B[0]]) + mc.abs()) + V[B[2]]
             + (x31 @ V[B[3]].reshape(256, 128)) * (W[B[4]] * rd)
             + V[B[4]] * rd * (x31 @ W[B[3]].reshape(256, 128) + md.abs()) + V[B[5]])
    u = iho.resize_legacy(absf(sub24_32), 2)
    lin12 = (ifo.conv_dilated(iho.resize_legacy(alive(sub24_32) * lin24, 2), W[N[0]]) * (W[N[1]] * ra)
             + ifo.conv_dilated(u, V[N[0]]) * (W[N[1]] * ra) + V[N[1]] * ra * (ifo.conv_dilated(u, W[N[0]]) + ma.abs())
             + V[N[2]]
             + (x3 @ V[N[3]].reshape(64, 128)) * (W[N[4]] * rb)
             + V[N[4]] * rb * (x3 @ W[N[3]].reshape(64, 128) + mb.abs()) + V[N[5]])
    lq = (iho.resize_legacy(alive(sub12_32) * lin12, 2) @ W[N[6]].reshape(128, k)
          + iho.resize_legacy(absf(sub12_32), 2) @ V[N[6]].reshape(128, k) + V[N[7]])
    (iho.resize_legacy(lq, 4) * ab).sum().backward()
    return g, pack({n: V[n].grad.numpy() for n in NAMES}), loss


def workgroups(n, h32, w32, max_workgroups=0):
    """(pixel tiles, split-K groups) of the increase layer's weight gradient: the pyramid trainer's plan"""
    return ipo.workgroups(n, h32, w32, max_workgroups)


def kappa(name, n, h32, w32, k, weight, max_workgroups=0):
    """the error-bound factor of the gradient test.  The pyramid trainer's seventeen tensors keep section
    39's (their bits are its bits on the same conv5_3_sum).  The increase layer's three share the chain behind one value of g53 =
    dL/dconv5_3:
      section 39's chain behind one value of g32   (icnet_pyramid_train_oracle.kappa's kg32)
      3 + 1                                        s1 = gamma / sqrt(var + eps); the product s1 g32, rounded once when staged
      256                                          k_icnet_pool_dx: one accumulator adds its products in ascending co
      2 * 3                                        a resize weight per axis: the fp32 ratio b / size, the source position, 1 - l
                                                   (the oracle forms the position in fp32 too; the subtraction and the two
                                                   products are not shared)
      w32 + h32                                    the fmaf chains of the column and the row stage of the bin gradients
      1                                            the division by the bin's pixel count
      bins_per_pixel(h32, w32)                     the adds of the bin gradients onto the identity term
    then, per tensor,
      32 ceil(tiles / G) + G                       the matrix-core chain over the group's pixels (conv5_3_3x3 is an input: no
                                                   rounding of its own) and the fold
      3 + 2                                        s (kernel); the two final products
      256 + 2 + 3 + 1                              gamma: the ci chain, - mean dBeta, rstd, the scale"""
    if name in ipo.NAMES:
        return ipo.kappa(name, n, h32, w32, k, weight, max_workgroups)
    tiles, groups = workgroups(n, h32, w32, max_workgroups)
    w32f = float(np.float32(weight))
    cond = 1.0 / np.log(w32f) if w32f > 1.0 else 0.0
    kg24 = 16 * (k + 8) * (1.0 + cond) + 64 + 3 + 16 + 4 + k + 3 + 1 + ico.DX_CHAIN + 9
    kg32 = kg24 + 3 + 1 + ipo.DX_CHAIN + 9
    kg53 = kg32 + 3 + 1 + K1_CHAIN + 2 * 3 + w32 + h32 + 1 + bins_per_pixel(h32, w32)
    chain = kg53 + PIXEL_TILE * -(-tiles // groups) + groups
    if name == BLOCK[0]:
        return chain + 3 + 2
    if name == BLOCK[2]:
        return chain + 1
    return chain + 256 + 2 + 3 + 1


def coherent_case(seed, n, h, w, k):
    """(conv5_3_3x3, conv5_2, conv3_1, conv3_sub1, {name: weights}, stats, labels, mask) with the signs along the whole backward
    path in agreement (``icnet_pyramid_train_oracle.coherent_case``'s recipe, one layer further down): its arrays above
    conv5_3_sum, a non-negative increase kernel with positive gammas over non-negative inputs, so that dL/dconv5_3_sum, the bin
    gradients and g53 have one sign at every pixel and channel.  conv5_3_3x3 carries a factor per pixel and the increase layer's
    beta puts the 30 % quantile of each channel's pre-activation at 0, so that the ReLU mask varies over the map; conv5_4_k1's
    beta is placed the same way on the conv5_3_sum that results; the head is rescaled to logits within +-1."""
    _, c31, c3, d17, stats17, labels, mask = ipo.coherent_case(seed, n, h, w, k)
    rng = np.random.default_rng(seed + 77)
    a = (np.abs(rng.standard_normal((n, h, w, 256)) * 0.7) * rng.uniform(0.3, 1.7, (n, h, w, 1))).astype(np.float32)
    c52 = np.abs(rng.standard_normal((n, h, w, 1024)) * 0.1).astype(np.float32)
    own = np.concatenate([rng.uniform(-0.3, 0.3, 1024), rng.uniform(0.5, 2.0, 1024)]).astype(np.float32)
    stats = np.concatenate([own, stats17]).astype(np.float32)
    K = rng.uniform(0.0, 0.08, (1, 1, 256, 1024)).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, 1024).astype(np.float32)
    m, v = own[:1024].astype(np.float64), own[1024:].astype(np.float64)
    s = gamma.astype(np.float64) / np.sqrt(v + EPS)
    lin = (a.astype(np.float64).reshape(-1, 256) @ K.astype(np.float64).reshape(256, 1024)) * s + c52.reshape(-1, 1024)
    q = np.quantile(lin, 0.3, axis=0)
    if n * h * w == 1:
        q = q * np.where(np.arange(1024) % 3 == 0, 1.5, 0.5)  # one pixel: a third of the channels dead
    d = dict(d17)
    d[BLOCK[0]], d[BLOCK[1]], d[BLOCK[2]] = K, gamma, (m * s - q).astype(np.float32)
    d = {name: np.asarray(d[name]).astype(np.float32) for name in NAMES}
    # conv5_4_k1's beta on this conv5_3_sum, as the pyramid recipe places it
    s53 = pool_forward(a, c52, c31, c3, pack(d), stats)[1]
    k1 = d["conv5_4_k1.kernel"].astype(np.float64).reshape(1024, 256)
    m1, v1 = stats17[:256].astype(np.float64), stats17[256:512].astype(np.float64)
    s1 = d["conv5_4_k1.gamma"].astype(np.float64) / np.sqrt(v1 + EPS)
    q1 = np.quantile(s53.reshape(-1, 1024) @ k1, 0.3, axis=0)
    if n * h * w == 1:
        q1 = q1 * np.where(np.arange(256) % 3 == 0, 1.5, 0.5)
    d["conv5_4_k1.beta"] = (m1 * s1 - s1 * q1).astype(np.float32)
    top = np.abs(pool_forward(a, c52, c31, c3, pack(d), stats)[5]).max()
    d["conv6_cls.kernel"] = (d["conv6_cls.kernel"] / np.float32(max(top, 1e-6))).astype(np.float32)
    return a, c52, c31, c3, d, stats, labels, mask


def adam_pool(w, m, v, g, k, lr, beta1, beta2, eps, b1p, b2p, l1=0.0, l2=0.0):
    """numpy float32 ApplyAdam on the packed vector: the l1_l2 regulariser goes to the seven kernels only"""
    out = [np.array(x, dtype=np.float32) for x in (w, m, v)]
    for name, (lo, hi) in offsets(k).items():
        reg = dict(l1=l1, l2=l2) if name in KERNELS else {}
        res = fto.adam_step(w[lo:hi], m[lo:hi], v[lo:hi], g[lo:hi], lr, beta1, beta2, eps, b1p, b2p, **reg)
        for o, r in zip(out, res):
            o[lo:hi] = r
    return tuple(out)


def train_float64(a, c52, c31, c3, packed0, stats, labels, mask, k, steps, lr, beta1, beta2, eps, weight, label_smoothing, l2):
    """``steps`` Adam steps in float64 (the regulariser on the kernels only) -> the losses before each step"""
    w = np.asarray(packed0, dtype=np.float64).copy()
    m, v = np.zeros_like(w), np.zeros_like(w)
    reg = np.zeros_like(w)
    for name in KERNELS:
        lo, hi = offsets(k)[name]
        reg[lo:hi] = 1.0
    out = []
    for t in range(1, steps + 1):
        loss, g = loss_and_grad(a, c52, c31, c3, w, stats, labels, mask, weight, label_smoothing)
        out.append(loss)
        g = g + reg * (2.0 * l2) * w
        alpha = lr * np.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)
        m += (g - m) * (1.0 - beta1)
        v += (g * g - v) * (1.0 - beta2)
        w -= m * alpha / (np.sqrt(v) + eps)
    return out
