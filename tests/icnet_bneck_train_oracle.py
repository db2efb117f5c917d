"""TEST INFRASTRUCTURE ONLY -- never imported by the product.

Float64 restatement of the training step of ICNet's last backbone bottleneck, from ``conv5_2``,
``conv3_1`` and ``conv3_sub1`` to the loss:
  * ``conv5_3_1x1_reduce = relu(BN(conv5_2 @ kernel))``: 1 x 1, 1024 -> 256, under inference batch-norm;
  * ``conv5_3_3x3 = relu(BN(3 x 3 conv at dilation 4 of it))``: 256 -> 256, SAME = four zero pixels on every side, written here
    as nine shifted slices of the padded map, each times its tap (``conv3``);
  * everything above: ``icnet_pool_train_oracle``'s restatement, with ``conv5_2`` as the increase layer's identity shortcut.
Autograd supplies the gradients (``relu'(0) = 0``); ``bneck_backward`` restates the new backward pass term by term, the way the
kernels compute it, from autograd's dL/dconv5_3, and can leave one step out or get it wrong (the discrimination test).  The 26
variables are packed as the product packs them: the reduce layer's three, the 3 x 3's three, then ``icnet_pool_train_oracle``'s
twenty.
"""
import numpy as np
import torch
import torch.nn.functional as F

import final_train_oracle as fto
import icnet_cascade_train_oracle as ico
import icnet_fusion_train_oracle as ifo
import icnet_head_train_oracle as iho
import icnet_pool_train_oracle as po
import icnet_pyramid_train_oracle as ipo

REDUCE, CONV3 = "conv5_3_1x1_reduce", "conv5_3_3x3"
BLOCK_R = (REDUCE + ".kernel", REDUCE + ".gamma", REDUCE + ".beta")
BLOCK_3 = (CONV3 + ".kernel", CONV3 + ".gamma", CONV3 + ".beta")
BLOCK = BLOCK_R + BLOCK_3
NAMES = BLOCK + po.NAMES
KERNELS = (BLOCK_R[0], BLOCK_3[0]) + po.KERNELS  # what the l1_l2 regulariser reaches
BLOCK_FLOATS = 1024 * 256 + 2 * 256 + 9 * 256 * 256 + 2 * 256
STATS_OWN = 4 * 256
DIL = 4
PIXEL_TILE = 32   # pixels per split-K tile of k_icnet_bneck_wgrad3 and of k_icnet_pyramid_wgrad<1024, 256>
MAX_WG = 16       # split-K groups of either launch
INC_CHAIN = 1024      # products k_icnet_bneck_dx_inc adds one after the other on one accumulator
DX3_CHAIN = 9 * 256   # and k_icnet_bneck_dx_3x3
EPS = ifo.EPS
# one step of the backward pass left out or done the wrong way
WRONG = ("dilation_2", "taps_not_mirrored", "edge_clamp", "no_mask_a", "no_mask_r", "no_s3", "no_si")
# mistakes of the weight-gradient, fold and gamma kernels themselves
WRONG_LOCAL = ("drop_last_pixel", "drop_last_group", "no_mean_term", "kernel_10_percent")
# what each wrong pass corrupts.  The dilation and the padding enter the 3 x 3 weight gradient (its kernel and, through the
# folded gradient, its gamma; not its beta) and the data gradient (the reduce layer's three); the mirroring, conv5_3_1x1_reduce's
# mask and s_3 only the data gradient; conv5_3_3x3's mask and s_i change g3, so all six
CORRUPTS = {"dilation_2": (BLOCK_3[0], BLOCK_3[1]) + BLOCK_R, "edge_clamp": (BLOCK_3[0], BLOCK_3[1]) + BLOCK_R,
            "taps_not_mirrored": BLOCK_R, "no_mask_r": BLOCK_R, "no_s3": BLOCK_R, "no_mask_a": BLOCK, "no_si": BLOCK,
            "drop_last_pixel": BLOCK, "drop_last_group": BLOCK, "no_mean_term": (BLOCK_R[1], BLOCK_3[1]),
            "kernel_10_percent": (BLOCK_R[0], BLOCK_R[1], BLOCK_3[0], BLOCK_3[1])}


def shapes(k):
    return ((1, 1, 1024, 256), (256,), (256,), (3, 3, 256, 256), (256,), (256,)) + po.shapes(k)


def offsets(k):
    out, lo = {}, 0
    for name, shp in zip(NAMES, shapes(k)):
        out[name] = (lo, lo + int(np.prod(shp)))
        lo = out[name][1]
    return out


def floats(k):
    return BLOCK_FLOATS + po.floats(k)


def classes_of(packed):
    return po.classes_of(np.asarray(packed)[BLOCK_FLOATS:])


def unpack(packed, k=None):
    packed = np.asarray(packed)
    k = classes_of(packed) if k is None else k
    off = offsets(k)
    return {n: packed[off[n][0]:off[n][1]].reshape(s) for n, s in zip(NAMES, shapes(k))}


def pack(d):
    return np.concatenate([np.asarray(d[n]).reshape(-1) for n in NAMES])


def split_stats(stats):
    """[4 * 256 + ...] -> mean, variance of the reduce layer, of the 3 x 3 (float64 torch) and the pooling trainer's rows (numpy)"""
    stats = np.asarray(stats, dtype=np.float64)
    return tuple(torch.as_tensor(stats[256 * i:256 * (i + 1)]) for i in range(4)) + (stats[STATS_OWN:],)


def draw_stats(seed):
    """moving statistics for the gradient cases: the two layers' four rows of 256, then the pooling trainer's"""
    rng = np.random.default_rng(seed + 2000)
    own = [rng.uniform(-0.3, 0.3, 256), rng.uniform(0.5, 2.0, 256), rng.uniform(-0.3, 0.3, 256), rng.uniform(0.5, 2.0, 256)]
    return np.concatenate(own + [po.draw_stats(seed)]).astype(np.float32)


def case(seed, n, h, w, k):
    """the arrays of one gradient case: ``conv5_2`` >= 0 (a ReLU output) and two kernels of both signs sized so that both
    pre-activations have both signs; the rest as the pooling test draws it"""
    _, _, c31, c3, d20, labels, mask = po.case(seed, n, h, w, k)
    rng = np.random.default_rng(seed + 177)
    x = np.abs(rng.standard_normal((n, h, w, 1024)) * 0.3).astype(np.float32)
    d = {BLOCK_R[0]: rng.uniform(-0.08, 0.08, (1, 1, 1024, 256)), BLOCK_R[1]: rng.uniform(0.5, 1.5, 256),
         BLOCK_R[2]: rng.uniform(-0.2, 0.4, 256), BLOCK_3[0]: rng.uniform(-0.08, 0.08, (3, 3, 256, 256)),
         BLOCK_3[1]: rng.uniform(0.5, 1.5, 256), BLOCK_3[2]: rng.uniform(-0.2, 0.4, 256)}
    d = {name: v.astype(np.float32) for name, v in d.items()}
    d.update(d20)
    return x, c31, c3, d, labels, mask


# ---- the dilated 3 x 3 ----
def conv3(x, K, dil=DIL):
    """x [N, h, w, ci] (torch), K [3, 3, ci, co]: out[y, x] = sum_tap x[y + dil (ky - 1), x + dil (kx - 1)] @ K[ky, kx], zero
    outside the map"""
    _, h, w, _ = x.shape
    xp = F.pad(x, (0, 0, dil, dil, dil, dil))
    out = 0.0
    for ky in range(3):
        for kx in range(3):
            out = out + xp[:, ky * dil:ky * dil + h, kx * dil:kx * dil + w] @ K[ky, kx]
    return out


def shift(z, dy, dx, clamp=False):
    """numpy [N, h, w, c]: out[y, x] = z[y + dy, x + dx], zero outside the map (``clamp``: the nearest pixel inside)"""
    n, h, w, _ = z.shape
    ys, xs = np.arange(h) + dy, np.arange(w) + dx
    if clamp:
        return z[:, np.clip(ys, 0, h - 1)][:, :, np.clip(xs, 0, w - 1)]
    out = np.zeros_like(z)
    vy, vx = (ys >= 0) & (ys < h), (xs >= 0) & (xs < w)
    if vy.any() and vx.any():
        out[np.ix_(np.arange(n), np.where(vy)[0], np.where(vx)[0])] = z[np.ix_(np.arange(n), ys[vy], xs[vx])]
    return out


# ---- forward and loss ----
def _tensors(x, c31, c3, packed, grad=True):
    W = {n: torch.as_tensor(np.asarray(v, dtype=np.float64).copy()).requires_grad_(grad) for n, v in unpack(packed).items()}
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))
    return t(x), t(c31), t(c3), W


def _pre_r(x, W, m, v):
    s = W[BLOCK_R[1]] / torch.sqrt(v + EPS)
    return (x @ W[BLOCK_R[0]].reshape(1024, 256)) * s + (W[BLOCK_R[2]] - m * s)


def _pre_3(r, W, m, v):
    s = W[BLOCK_3[1]] / torch.sqrt(v + EPS)
    return conv3(r, W[BLOCK_3[0]]) * s + (W[BLOCK_3[2]] - m * s)


def bneck_forward(x, c31, c3, packed, stats):
    """-> (conv5_3_1x1_reduce, conv5_3_3x3, conv5_3, conv5_3_sum, conv5_4_k1, sub24_sum, sub12_sum, full-resolution logits)
    float64 numpy"""
    xt, _, _, W = _tensors(x, c31, c3, packed, grad=False)
    mr, vr, m3, v3, pstats = split_stats(stats)
    r = torch.relu(_pre_r(xt, W, mr, vr))
    a = torch.relu(_pre_3(r, W, m3, v3))
    return (r.numpy(), a.numpy()) + po.pool_forward(a.numpy(), x, c31, c3, np.asarray(packed)[BLOCK_FLOATS:], pstats)


def _loss(xt, x31, x3, W, stats, labels, mask, weight, label_smoothing, acts=None, keep=None):
    """the float64 loss as a torch scalar.  ``acts``: ``bneck_forward``'s eight in fp32 -- the ReLUs, the pooling sum and the loss
    are evaluated at those values, the point the GPU evaluates.  ``keep``: a dict that receives conv5_3 (gradient retained) and the
    float64 conv5_3_1x1_reduce and conv5_3_3x3"""
    acts = (None,) * 8 if acts is None else acts
    mr, vr, m3, v3, pstats = split_stats(stats)
    r = ico._pinned_relu(_pre_r(xt, W, mr, vr), acts[0])
    a = ico._pinned_relu(_pre_3(r, W, m3, v3), acts[1])
    inner = {} if keep is not None else None
    loss = po._loss(a, xt, x31, x3, W, pstats, labels, mask, weight, label_smoothing, tuple(acts[2:]), inner)
    if keep is not None:
        inner["c53"].retain_grad()
        keep["r"], keep["a"], keep["c53"] = r, a, inner["c53"]
    return loss


def loss_and_grad(x, c31, c3, packed, stats, labels, mask, weight, label_smoothing, acts=None):
    """float64 (loss, packed gradient)"""
    xt, x31, x3, W = _tensors(x, c31, c3, packed)
    loss = _loss(xt, x31, x3, W, stats, labels, mask, weight, label_smoothing, acts)
    loss.backward()
    return float(loss.detach()), pack({n: W[n].grad.numpy() for n in NAMES})


def bneck_backward(x, c31, c3, packed, stats, labels, mask, weight, label_smoothing, acts=None, wrong=None, max_workgroups=0):
    """the six new gradients restated the way the kernels compute them, from autograd's dL/dconv5_3:
    g53 = relu'(conv5_3) dL/dconv5_3; g3 = relu'(a) ((s_i g53) K_i^T); dr[p] = sum_tap (s_3 g3)[p - 4 (tap - 1)] K_3[tap]^T;
    gr = relu'(r) dr; dK_3[tap] = s_3 r[p + 4 (tap - 1)]^T g3, dK_r = s_r x^T gr; dBeta = sum_p g; dGamma contracted from the
    folded weight gradients.  ``wrong``: one of ``WRONG`` or ``WRONG_LOCAL``; ``drop_last_group`` leaves out the pixel tiles of
    the last split-K group of the grid ``max_workgroups`` gives (``workgroups``: tile t belongs to group t mod G).
    -> {name: float64 array} for ``BLOCK``"""
    assert wrong is None or wrong in WRONG + WRONG_LOCAL
    xt, x31, x3, W = _tensors(x, c31, c3, packed)
    keep = {}
    _loss(xt, x31, x3, W, stats, labels, mask, weight, label_smoothing, acts, keep).backward()
    c53 = keep["c53"].detach().numpy()
    g53 = keep["c53"].grad.numpy() * (c53 > 0)
    r, a = keep["r"].detach().numpy(), keep["a"].detach().numpy()
    Wn = {n: v.detach().numpy() for n, v in W.items()}
    st = np.asarray(stats, dtype=np.float64)
    mr, vr, m3, v3 = (st[256 * i:256 * (i + 1)] for i in range(4))
    vi = st[STATS_OWN + 1024:STATS_OWN + 2048]
    s_i = Wn[po.BLOCK[1]] / np.sqrt(vi + EPS)
    rstd_r, rstd_3 = 1.0 / np.sqrt(vr + EPS), 1.0 / np.sqrt(v3 + EPS)
    s_r, s_3 = Wn[BLOCK_R[1]] * rstd_r, Wn[BLOCK_3[1]] * rstd_3
    K3 = Wn[BLOCK_3[0]]
    d3 = (g53 if wrong == "no_si" else g53 * s_i) @ Wn[po.BLOCK[0]].reshape(256, 1024).T
    g3 = d3 if wrong == "no_mask_a" else d3 * (a > 0)
    dil = 2 if wrong == "dilation_2" else DIL
    clamp = wrong == "edge_clamp"
    sign = 1 if wrong == "taps_not_mirrored" else -1
    gs3 = g3 if wrong == "no_s3" else g3 * s_3
    dr = np.zeros_like(r)
    for ky in range(3):
        for kx in range(3):
            dr += shift(gs3, sign * dil * (ky - 1), sign * dil * (kx - 1), clamp) @ K3[ky, kx].T
    gr = dr if wrong == "no_mask_r" else dr * (r > 0)
    g3f, grf = g3.reshape(-1, 256).copy(), gr.reshape(-1, 256).copy()
    if wrong == "drop_last_pixel":
        g3f[-1:], grf[-1:] = 0.0, 0.0
    if wrong == "drop_last_group":
        n, h, w, _ = r.shape
        _, groups = workgroups(n, h, w, max_workgroups)
        last = (np.arange(n * h * w) // PIXEL_TILE) % groups == groups - 1
        g3f[last], grf[last] = 0.0, 0.0
    scale = 1.1 if wrong == "kernel_10_percent" else 1.0
    raw3 = np.stack([np.stack([shift(r, dil * (ky - 1), dil * (kx - 1), clamp).reshape(-1, 256).T @ g3f for kx in range(3)])
                     for ky in range(3)]) * scale
    rawr = (np.asarray(x, dtype=np.float64).reshape(-1, 1024).T @ grf) * scale
    mean_r, mean_3 = (0.0, 0.0) if wrong == "no_mean_term" else (mr, m3)
    Kr = Wn[BLOCK_R[0]].reshape(1024, 256)
    return {BLOCK_R[0]: (rawr * s_r).reshape(1, 1, 1024, 256),
            BLOCK_R[1]: ((Kr * rawr).sum(0) - mean_r * grf.sum(0)) * rstd_r, BLOCK_R[2]: grf.sum(0),
            BLOCK_3[0]: raw3 * s_3, BLOCK_3[1]: ((K3 * raw3).sum((0, 1, 2)) - mean_3 * g3f.sum(0)) * rstd_3,
            BLOCK_3[2]: g3f.sum(0)}


def grad_and_bound(x, c31, c3, packed, stats, labels, mask, weight, label_smoothing, acts):
    """(g64, C, loss64), packed: the float64 gradient at the fp32 activations, and the same contraction over absolute values.
    ``icnet_pool_train_oracle.grad_and_bound``'s chain with two more layers under conv5_3's alive units: the increase layer's
    |K_i| pull-back onto the alive units of conv5_3_3x3, the 3 x 3's |K_3| pull-back onto the alive units of conv5_3_1x1_reduce,
    contracted there with
      kernel   |s| sum_p |input| gabs     beta   sum_p gabs     gamma   rstd sum_p gabs (|input| * |K| + |mean|)."""
    r32, a32, c53_32, s53_32, f1_32, sub24_32, sub12_32, logits32 = acts
    k = classes_of(packed)
    loss, g = loss_and_grad(x, c31, c3, packed, stats, labels, mask, weight, label_smoothing, acts)
    ab = ifo.pixel_bound(logits32, labels, mask, k, weight, label_smoothing)
    xt, x31, x3, W = _tensors(np.abs(x), np.abs(c31), np.abs(c3), np.abs(np.asarray(packed)), grad=False)
    V = {n: torch.zeros(s, dtype=torch.float64, requires_grad=True) for n, s in zip(NAMES, shapes(k))}
    mr, vr, m3, v3, pstats = split_stats(stats)
    m0, v0, ystats = po.split_stats(pstats)
    m1, v1, cstats = ipo.split_stats(ystats)
    mc, vc, md, vd, fstats = ico.split_stats(cstats)
    ma, va, mb, vb = ifo.split_stats(fstats)
    rr, r3, r0, r1, rc, rd, ra, rb = (1.0 / torch.sqrt(v + EPS) for v in (vr, v3, v0, v1, vc, vd, va, vb))
    Q, P, B, N = po.BLOCK, ipo.BLOCK, ico.BLOCK, ifo.NAMES
    absf = lambda t: torch.as_tensor(np.abs(np.asarray(t, dtype=np.float64)))
    alive = lambda t: torch.as_tensor((np.asarray(t) > 0).astype(np.float64))
    Kr, Ki = W[BLOCK_R[0]].reshape(1024, 256), W[Q[0]].reshape(256, 1024)
    linr = ((xt @ V[BLOCK_R[0]].reshape(1024, 256)) * (W[BLOCK_R[1]] * rr)
            + V[BLOCK_R[1]] * rr * (xt @ Kr + mr.abs()) + V[BLOCK_R[2]])
    xr = absf(r32)
    lin3 = (conv3(alive(r32) * linr, W[BLOCK_3[0]]) * (W[BLOCK_3[1]] * r3)
            + conv3(xr, V[BLOCK_3[0]]) * (W[BLOCK_3[1]] * r3)
            + V[BLOCK_3[1]] * r3 * (conv3(xr, W[BLOCK_3[0]]) + m3.abs()) + V[BLOCK_3[2]])
    xa = absf(a32)
    lin53 = (((alive(a32) * lin3) @ Ki) * (W[Q[1]] * r0)
             + (xa @ V[Q[0]].reshape(256, 1024)) * (W[Q[1]] * r0)
             + V[Q[1]] * r0 * (xa @ Ki + m0.abs()) + V[Q[2]])
    x53 = absf(s53_32)
    lin32 = ((po.ppm_forward(alive(c53_32) * lin53) @ W[P[0]].reshape(1024, 256)) * (W[P[1]] * r1)
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
    """(pixel tiles, split-K groups) of either new weight gradient: 32-pixel tiles strided over at most 16 groups"""
    return ipo.workgroups(n, h32, w32, max_workgroups)


def kappa(name, n, h32, w32, k, weight, max_workgroups=0):
    """the error-bound factor of the gradient test.  The pooling trainer's twenty tensors keep section
    41's (their bits are its bits on the same conv5_3_3x3).  The 3 x 3's three share the chain behind one value of g3 =
    dL/dconv5_3_3x3:
      section 41's chain behind one value of g53   (icnet_pool_train_oracle.kappa's kg53)
      3 + 1                                        s_i = gamma / sqrt(var + eps); the product s_i g53, rounded once when staged
      1024                                         k_icnet_bneck_dx_inc: one accumulator adds its products in ascending co
    the reduce layer's three the chain behind one value of gr = dL/dconv5_3_1x1_reduce:
      the chain behind g3
      3 + 1                                        s_3; the product s_3 g3, rounded once when staged
      9 * 256                                      k_icnet_bneck_dx_3x3: one accumulator adds all its products one after the
                                                   other (chunk of co, tap, co within the chunk)
    then, per tensor,
      32 ceil(tiles / G) + G                       the matrix-core chain over the group's pixels (the layer's input is a forward
                                                   value: no rounding of its own) and the fold
      3 + 2                                        s (kernel); the two final products
      ci + 2 + 3 + 1                               gamma: the ci chain (1024; 9 * 256 and the 9 tap sums), - mean dBeta, rstd, the
                                                   scale"""
    if name in po.NAMES:
        return po.kappa(name, n, h32, w32, k, weight, max_workgroups)
    tiles, groups = workgroups(n, h32, w32, max_workgroups)
    # section 41's chain behind g53 is what its kappa of the increase layer's beta holds in front of that layer's own pixel
    # chain, fold and final product: taken from there, so that the two derivations cannot drift apart
    kg53 = po.kappa(po.BLOCK[2], n, h32, w32, k, weight, max_workgroups) - (po.PIXEL_TILE * -(-tiles // groups) + groups) - 1
    kg3 = kg53 + 3 + 1 + INC_CHAIN
    kgr = kg3 + 3 + 1 + DX3_CHAIN
    three = name in BLOCK_3
    chain = (kg3 if three else kgr) + PIXEL_TILE * -(-tiles // groups) + groups
    if name in (BLOCK_R[0], BLOCK_3[0]):
        return chain + 3 + 2
    if name in (BLOCK_R[2], BLOCK_3[2]):
        return chain + 1
    return chain + (9 * 256 + 9 if three else 1024) + 2 + 3 + 1


def coherent_case(seed, n, h, w, k):
    """(conv5_2, conv3_1, conv3_sub1, {name: weights}, stats, labels, mask) with the signs along the whole backward path in
    agreement (``icnet_pool_train_oracle.coherent_case``'s recipe, one layer further down): its arrays above conv5_3_3x3,
    non-negative reduce and 3 x 3 kernels with positive gammas over a non-negative conv5_2, so that g53, g3 and gr have one sign
    at every pixel and channel.  conv5_2 carries a factor per pixel (the last pixel the largest one, so that it is alive) and the
    3 x 3's centre tap is four times the others, so that the factor reaches conv5_3_3x3; each of the two layers' betas puts the
    30 % quantile of every channel's pre-activation at 0, so that both ReLU masks vary over the map; the increase layer's and
    conv5_4_k1's betas are placed the same way on the maps that result; the head is rescaled to logits within +-1."""
    _, _, c31, c3, d20, stats20, labels, mask = po.coherent_case(seed, n, h, w, k)
    rng = np.random.default_rng(seed + 177)
    f = rng.uniform(0.3, 1.7, (n, h, w, 1))
    f[-1, -1, -1] = 1.7
    x = (np.abs(rng.standard_normal((n, h, w, 1024)) * 0.3) * f).astype(np.float32)
    own = np.concatenate([rng.uniform(-0.3, 0.3, 256), rng.uniform(0.5, 2.0, 256), rng.uniform(-0.3, 0.3, 256),
                          rng.uniform(0.5, 2.0, 256)]).astype(np.float32)
    stats = np.concatenate([own, stats20]).astype(np.float32)
    d = dict(d20)
    d[BLOCK_R[0]] = rng.uniform(0.0, 0.004, (1, 1, 1024, 256)).astype(np.float32)
    K3 = rng.uniform(0.0, 0.003, (3, 3, 256, 256))
    K3[1, 1] *= 4.0
    d[BLOCK_3[0]] = K3.astype(np.float32)
    d[BLOCK_R[1]], d[BLOCK_3[1]] = (rng.uniform(0.5, 1.5, 256).astype(np.float32) for _ in range(2))
    own64 = own.astype(np.float64)
    x64 = x.astype(np.float64)
    # the reduce layer: pre = s (x K - mean) + beta = s (x K - q) with beta = s (mean - q)
    s_r = d[BLOCK_R[1]].astype(np.float64) / np.sqrt(own64[256:512] + EPS)
    lin_r = x64.reshape(-1, 1024) @ d[BLOCK_R[0]].astype(np.float64).reshape(1024, 256)
    d[BLOCK_R[2]] = (s_r * (own64[:256] - np.quantile(lin_r, 0.3, axis=0))).astype(np.float32)
    r = np.maximum(lin_r * s_r + (d[BLOCK_R[2]].astype(np.float64) - own64[:256] * s_r), 0.0).reshape(n, h, w, 256)
    s_3 = d[BLOCK_3[1]].astype(np.float64) / np.sqrt(own64[768:] + EPS)
    lin_3 = conv3(torch.as_tensor(r), torch.as_tensor(d[BLOCK_3[0]].astype(np.float64))).numpy().reshape(-1, 256)
    d[BLOCK_3[2]] = (s_3 * (own64[512:768] - np.quantile(lin_3, 0.3, axis=0))).astype(np.float32)
    d[po.BLOCK[2]] = np.zeros(1024, np.float32)
    d = {name: np.asarray(d[name]).astype(np.float32) for name in NAMES}
    # the increase layer's beta on this conv5_3_3x3, conv5_4_k1's on the conv5_3_sum that results, as the pooling recipe places them
    a = bneck_forward(x, c31, c3, pack(d), stats)[1]
    mi, vi = stats20[:1024].astype(np.float64), stats20[1024:2048].astype(np.float64)
    s_i = d[po.BLOCK[1]].astype(np.float64) / np.sqrt(vi + EPS)
    lin = (a.reshape(-1, 256) @ d[po.BLOCK[0]].astype(np.float64).reshape(256, 1024)) * s_i + x64.reshape(-1, 1024)
    d[po.BLOCK[2]] = (mi * s_i - np.quantile(lin, 0.3, axis=0)).astype(np.float32)
    s53 = bneck_forward(x, c31, c3, pack(d), stats)[3]
    k1 = d["conv5_4_k1.kernel"].astype(np.float64).reshape(1024, 256)
    m1, v1 = stats20[2048:2304].astype(np.float64), stats20[2304:2560].astype(np.float64)
    s1 = d["conv5_4_k1.gamma"].astype(np.float64) / np.sqrt(v1 + EPS)
    d["conv5_4_k1.beta"] = (m1 * s1 - s1 * np.quantile(s53.reshape(-1, 1024) @ k1, 0.3, axis=0)).astype(np.float32)
    top = np.abs(bneck_forward(x, c31, c3, pack(d), stats)[7]).max()
    d["conv6_cls.kernel"] = (d["conv6_cls.kernel"] / np.float32(max(top, 1e-6))).astype(np.float32)
    return x, c31, c3, d, stats, labels, mask


def adam_bneck(w, m, v, g, k, lr, beta1, beta2, eps, b1p, b2p, l1=0.0, l2=0.0):
    """numpy float32 ApplyAdam on the packed vector: the l1_l2 regulariser goes to the nine kernels only"""
    out = [np.array(x, dtype=np.float32) for x in (w, m, v)]
    for name, (lo, hi) in offsets(k).items():
        reg = dict(l1=l1, l2=l2) if name in KERNELS else {}
        res = fto.adam_step(w[lo:hi], m[lo:hi], v[lo:hi], g[lo:hi], lr, beta1, beta2, eps, b1p, b2p, **reg)
        for o, r in zip(out, res):
            o[lo:hi] = r
    return tuple(out)
