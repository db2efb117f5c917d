"""TEST INFRASTRUCTURE ONLY -- never imported by the product.

Float64 restatement of the training step of ICNet through ``conv5_2``, from ``conv5_1``, ``conv3_1`` and
``conv3_sub1`` to the loss:
  * ``conv5_2_1x1_reduce = relu(BN(conv5_1 @ kernel))``: 1 x 1, 1024 -> 256, under inference batch-norm;
  * ``conv5_2_3x3 = relu(BN(3 x 3 conv at dilation 4 of it))``: 256 -> 256 (``icnet_bneck_train_oracle.conv3``);
  * ``conv5_2 = relu(BN(conv5_2_3x3 @ kernel) + conv5_1)``: 1 x 1, 256 -> 1024, the identity shortcut;
  * everything above: ``icnet_bneck_train_oracle``'s restatement, with ``conv5_2`` as conv5_3's input and identity shortcut.
Autograd supplies the gradients (``relu'(0) = 0``); ``bneck2_backward`` restates the new backward pass term by term, the way the
kernels compute it, from autograd's dL/dconv5_3, and can leave one step out or get it wrong (the discrimination test).  The 35
variables are packed as the product packs them: conv5_2's reduce layer's three, its 3 x 3's three, its increase layer's three,
then ``icnet_bneck_train_oracle``'s 26.
"""
import numpy as np
import torch

import final_train_oracle as fto
import icnet_bneck_train_oracle as bo
import icnet_cascade_train_oracle as ico
import icnet_fusion_train_oracle as ifo
import icnet_head_train_oracle as iho
import icnet_pool_train_oracle as po
import icnet_pyramid_train_oracle as ipo
from icnet_bneck_train_oracle import conv3, shift

REDUCE, CONV3, INCREASE = "conv5_2_1x1_reduce", "conv5_2_3x3", "conv5_2_1x1_increase"
BLOCK_R = (REDUCE + ".kernel", REDUCE + ".gamma", REDUCE + ".beta")
BLOCK_3 = (CONV3 + ".kernel", CONV3 + ".gamma", CONV3 + ".beta")
BLOCK_I = (INCREASE + ".kernel", INCREASE + ".gamma", INCREASE + ".beta")
BLOCK = BLOCK_R + BLOCK_3 + BLOCK_I
NAMES = BLOCK + bo.NAMES
KERNELS = (BLOCK_R[0], BLOCK_3[0], BLOCK_I[0]) + bo.KERNELS  # what the l1_l2 regulariser reaches
BLOCK_FLOATS = 1024 * 256 + 2 * 256 + 9 * 256 * 256 + 2 * 256 + 256 * 1024 + 2 * 1024
STATS_OWN = 4 * 256 + 2 * 1024
DIL = bo.DIL
PIXEL_TILE, MAX_WG = bo.PIXEL_TILE, bo.MAX_WG  # the split-K plan of all five weight gradients of the two blocks
RED_CHAIN = 256  # products k_icnet_bneck2_dx_red adds one after the other on one accumulator
EPS = ifo.EPS
# one step of the new backward pass left out or done the wrong way
WRONG = ("no_shortcut", "no_reduce_path", "no_mask_52", "mask_from_53", "no_sr", "kr_wrong_axis", "dilation_2")
# mistakes of the weight-gradient, fold and gamma kernels themselves
WRONG_LOCAL = ("drop_last_pixel", "drop_last_group", "no_mean_term")
# what each wrong pass corrupts.  Everything that changes g52 = dL/dconv5_2 changes all nine; the dilation enters conv5_2's 3 x 3
# weight gradient (its kernel and, through the folded gradient, its gamma; not its beta) and the data gradient (the reduce
# layer's three), not the increase layer's three, which stand in front of it
CORRUPTS = {"no_shortcut": BLOCK, "no_reduce_path": BLOCK, "no_mask_52": BLOCK, "mask_from_53": BLOCK, "no_sr": BLOCK,
            "kr_wrong_axis": BLOCK, "dilation_2": (BLOCK_3[0], BLOCK_3[1]) + BLOCK_R, "drop_last_pixel": BLOCK,
            "drop_last_group": BLOCK, "no_mean_term": (BLOCK_R[1], BLOCK_3[1], BLOCK_I[1])}


def shapes(k):
    return ((1, 1, 1024, 256), (256,), (256,), (3, 3, 256, 256), (256,), (256,), (1, 1, 256, 1024), (1024,), (1024,)) + bo.shapes(k)


def offsets(k):
    out, lo = {}, 0
    for name, shp in zip(NAMES, shapes(k)):
        out[name] = (lo, lo + int(np.prod(shp)))
        lo = out[name][1]
    return out


def floats(k):
    return BLOCK_FLOATS + bo.floats(k)


def classes_of(packed):
    return bo.classes_of(np.asarray(packed)[BLOCK_FLOATS:])


def unpack(packed, k=None):
    packed = np.asarray(packed)
    k = classes_of(packed) if k is None else k
    off = offsets(k)
    return {n: packed[off[n][0]:off[n][1]].reshape(s) for n, s in zip(NAMES, shapes(k))}


def pack(d):
    return np.concatenate([np.asarray(d[n]).reshape(-1) for n in NAMES])


def split_stats(stats):
    """-> mean, variance of conv5_2's reduce layer, of its 3 x 3, of its increase layer (float64 torch) and the bottleneck
    trainer's rows (numpy)"""
    stats = np.asarray(stats, dtype=np.float64)
    rows = [stats[256 * i:256 * (i + 1)] for i in range(4)] + [stats[1024:2048], stats[2048:3072]]
    return tuple(torch.as_tensor(r) for r in rows) + (stats[STATS_OWN:],)


def _own_stats(rng):
    return [rng.uniform(-0.3, 0.3, 256), rng.uniform(0.5, 2.0, 256), rng.uniform(-0.3, 0.3, 256), rng.uniform(0.5, 2.0, 256),
            rng.uniform(-0.3, 0.3, 1024), rng.uniform(0.5, 2.0, 1024)]


def draw_stats(seed):
    """moving statistics for the gradient cases: conv5_2's six rows, then the bottleneck trainer's"""
    return np.concatenate(_own_stats(np.random.default_rng(seed + 3000)) + [bo.draw_stats(seed)]).astype(np.float32)


def case(seed, n, h, w, k):
    """the arrays of one gradient case: ``conv5_1`` >= 0 (a ReLU output) and three kernels of both signs sized so that the three
    pre-activations have both signs; the rest as the bottleneck test draws it"""
    _, c31, c3, d26, labels, mask = bo.case(seed, n, h, w, k)
    rng = np.random.default_rng(seed + 277)
    x = np.abs(rng.standard_normal((n, h, w, 1024)) * 0.3).astype(np.float32)
    d = {BLOCK_R[0]: rng.uniform(-0.08, 0.08, (1, 1, 1024, 256)), BLOCK_R[1]: rng.uniform(0.5, 1.5, 256),
         BLOCK_R[2]: rng.uniform(-0.2, 0.4, 256), BLOCK_3[0]: rng.uniform(-0.08, 0.08, (3, 3, 256, 256)),
         BLOCK_3[1]: rng.uniform(0.5, 1.5, 256), BLOCK_3[2]: rng.uniform(-0.2, 0.4, 256),
         BLOCK_I[0]: rng.uniform(-0.08, 0.08, (1, 1, 256, 1024)), BLOCK_I[1]: rng.uniform(0.5, 1.5, 1024),
         BLOCK_I[2]: rng.uniform(-0.6, 0.1, 1024)}
    d = {name: v.astype(np.float32) for name, v in d.items()}
    d.update(d26)
    return x, c31, c3, d, labels, mask


# ---- forward and loss ----
def _tensors(x, c31, c3, packed, grad=True):
    W = {n: torch.as_tensor(np.asarray(v, dtype=np.float64).copy()).requires_grad_(grad) for n, v in unpack(packed).items()}
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))
    return t(x), t(c31), t(c3), W


def _pre_r(x, W, m, v):
    s = W[BLOCK_R[1]] / torch.sqrt(v + EPS)
    return (x @ W[BLOCK_R[0]].reshape(1024, 256)) * s + (W[BLOCK_R[2]] - m * s)


def _pre_3(r, W, m, v, dil=DIL):
    s = W[BLOCK_3[1]] / torch.sqrt(v + EPS)
    return conv3(r, W[BLOCK_3[0]], dil) * s + (W[BLOCK_3[2]] - m * s)


def _pre_i(a, x, W, m, v):
    s = W[BLOCK_I[1]] / torch.sqrt(v + EPS)
    return (a @ W[BLOCK_I[0]].reshape(256, 1024)) * s + (W[BLOCK_I[2]] - m * s) + x


def block_forward(x, packed, stats):
    """-> (conv5_2_1x1_reduce, conv5_2_3x3, conv5_2) float64 numpy"""
    xt, _, _, W = _tensors(x, x[..., :1], x[..., :1], packed, grad=False)
    mr, vr, m3, v3, mi, vi, _ = split_stats(stats)
    r = torch.relu(_pre_r(xt, W, mr, vr))
    a = torch.relu(_pre_3(r, W, m3, v3))
    return r.numpy(), a.numpy(), torch.relu(_pre_i(a, xt, W, mi, vi)).numpy()


def bneck2_forward(x, c31, c3, packed, stats):
    """-> (conv5_2_1x1_reduce, conv5_2_3x3, conv5_2) + ``icnet_bneck_train_oracle.bneck_forward``'s eight, float64 numpy"""
    own = block_forward(x, packed, stats)
    return own + bo.bneck_forward(own[2], c31, c3, np.asarray(packed)[BLOCK_FLOATS:], np.asarray(stats)[STATS_OWN:])


def _loss(xt, x31, x3, W, stats, labels, mask, weight, label_smoothing, acts=None, keep=None):
    """the float64 loss as a torch scalar.  ``acts``: ``bneck2_forward``'s eleven in fp32 -- the ReLUs, the pooling sum and the loss
    are evaluated at those values, the point the GPU evaluates.  ``keep``: a dict that receives what the bottleneck oracle keeps
    (conv5_3 with its gradient, conv5_3's reduce and 3 x 3) and r2, a2, c52 of this block (c52's gradient retained)"""
    acts = (None,) * 11 if acts is None else acts
    mr, vr, m3, v3, mi, vi, bstats = split_stats(stats)
    r = ico._pinned_relu(_pre_r(xt, W, mr, vr), acts[0])
    a = ico._pinned_relu(_pre_3(r, W, m3, v3), acts[1])
    c52 = ico._pinned_relu(_pre_i(a, xt, W, mi, vi), acts[2])
    loss = bo._loss(c52, x31, x3, W, bstats, labels, mask, weight, label_smoothing, tuple(acts[3:]), keep)
    if keep is not None:
        keep["r2"], keep["a2"], keep["c52"] = r, a, c52
    return loss


def loss_and_grad(x, c31, c3, packed, stats, labels, mask, weight, label_smoothing, acts=None):
    """float64 (loss, packed gradient)"""
    xt, x31, x3, W = _tensors(x, c31, c3, packed)
    loss = _loss(xt, x31, x3, W, stats, labels, mask, weight, label_smoothing, acts)
    loss.backward()
    return float(loss.detach()), pack({n: W[n].grad.numpy() for n in NAMES})


def bneck2_backward(x, c31, c3, packed, stats, labels, mask, weight, label_smoothing, acts=None, wrong=None, max_workgroups=0):
    """the nine new gradients restated the way the kernels compute them, from autograd's dL/dconv5_3: section 42's g53, g3 and gr
    of conv5_3; g52 = relu'(conv5_2) (g53 + (s_r gr) K_r^T); dK_i = s_i a2^T g52; then section 42's link on conv5_2's own layers:
    g3' = relu'(a2) ((s_i g52) K_i^T), gr' = relu'(r2) sum_tap (s_3 g3')[p - 4 (tap - 1)] K_3[tap]^T, dK_3[tap] = s_3 r2[p + 4
    (tap - 1)]^T g3', dK_r = s_r conv5_1^T gr'; dBeta = sum_p g; dGamma contracted from the folded weight gradients.  ``wrong``:
    one of ``WRONG`` or ``WRONG_LOCAL``; ``drop_last_group`` as in ``icnet_bneck_train_oracle.bneck_backward``.
    -> {name: float64 array} for ``BLOCK``"""
    assert wrong is None or wrong in WRONG + WRONG_LOCAL
    xt, x31, x3, W = _tensors(x, c31, c3, packed)
    keep = {}
    _loss(xt, x31, x3, W, stats, labels, mask, weight, label_smoothing, acts, keep).backward()
    c53 = keep["c53"].detach().numpy()
    g53 = keep["c53"].grad.numpy() * (c53 > 0)
    r, a = keep["r"].detach().numpy(), keep["a"].detach().numpy()
    r2, a2, c52 = (keep[n].detach().numpy() for n in ("r2", "a2", "c52"))
    Wn = {n: v.detach().numpy() for n, v in W.items()}
    st = np.asarray(stats, dtype=np.float64)
    rs = lambda lo, c: 1.0 / np.sqrt(st[lo + c:lo + 2 * c] + EPS)
    # conv5_3's own backward down to gr (section 42)
    u = STATS_OWN
    s_i3 = Wn[po.BLOCK[1]] * rs(u + bo.STATS_OWN, 1024)
    s_33, s_r3 = Wn[bo.BLOCK_3[1]] * rs(u + 512, 256), Wn[bo.BLOCK_R[1]] * rs(u, 256)
    g3 = ((g53 * s_i3) @ Wn[po.BLOCK[0]].reshape(256, 1024).T) * (a > 0)
    K33 = Wn[bo.BLOCK_3[0]]
    gr = sum(shift(g3 * s_33, -DIL * (ky - 1), -DIL * (kx - 1)) @ K33[ky, kx].T for ky in range(3) for kx in range(3)) * (r > 0)
    # the new kernel
    Kr3 = Wn[bo.BLOCK_R[0]].reshape(1024, 256)
    gs = gr if wrong == "no_sr" else gr * s_r3
    path = gs @ (Kr3.reshape(-1).reshape(256, 1024) if wrong == "kr_wrong_axis" else Kr3.T)
    total = (0.0 if wrong == "no_shortcut" else g53) + (0.0 if wrong == "no_reduce_path" else path)
    mask52 = 1.0 if wrong == "no_mask_52" else ((c53 if wrong == "mask_from_53" else c52) > 0)
    g52 = total * mask52
    # conv5_2 as a link
    mr, vr, m3, v3, mi, vi = st[:256], st[256:512], st[512:768], st[768:1024], st[1024:2048], st[2048:3072]
    rstd_r, rstd_3, rstd_i = (1.0 / np.sqrt(v + EPS) for v in (vr, v3, vi))
    s_r, s_3, s_i = Wn[BLOCK_R[1]] * rstd_r, Wn[BLOCK_3[1]] * rstd_3, Wn[BLOCK_I[1]] * rstd_i
    Ki, K3, Kr = Wn[BLOCK_I[0]].reshape(256, 1024), Wn[BLOCK_3[0]], Wn[BLOCK_R[0]].reshape(1024, 256)
    g3b = ((g52 * s_i) @ Ki.T) * (a2 > 0)
    dil = 2 if wrong == "dilation_2" else DIL
    grb = sum(shift(g3b * s_3, -dil * (ky - 1), -dil * (kx - 1)) @ K3[ky, kx].T for ky in range(3) for kx in range(3)) * (r2 > 0)
    gif, g3f, grf = g52.reshape(-1, 1024).copy(), g3b.reshape(-1, 256).copy(), grb.reshape(-1, 256).copy()
    if wrong == "drop_last_pixel":
        gif[-1:], g3f[-1:], grf[-1:] = 0.0, 0.0, 0.0
    if wrong == "drop_last_group":
        n, h, w, _ = r2.shape
        _, groups = workgroups(n, h, w, max_workgroups)
        last = (np.arange(n * h * w) // PIXEL_TILE) % groups == groups - 1
        gif[last], g3f[last], grf[last] = 0.0, 0.0, 0.0
    rawi = a2.reshape(-1, 256).T @ gif
    raw3 = np.stack([np.stack([shift(r2, dil * (ky - 1), dil * (kx - 1)).reshape(-1, 256).T @ g3f for kx in range(3)])
                     for ky in range(3)])
    rawr = np.asarray(x, dtype=np.float64).reshape(-1, 1024).T @ grf
    mean_r, mean_3, mean_i = (0.0, 0.0, 0.0) if wrong == "no_mean_term" else (mr, m3, mi)
    return {BLOCK_R[0]: (rawr * s_r).reshape(1, 1, 1024, 256),
            BLOCK_R[1]: ((Kr * rawr).sum(0) - mean_r * grf.sum(0)) * rstd_r, BLOCK_R[2]: grf.sum(0),
            BLOCK_3[0]: raw3 * s_3, BLOCK_3[1]: ((K3 * raw3).sum((0, 1, 2)) - mean_3 * g3f.sum(0)) * rstd_3,
            BLOCK_3[2]: g3f.sum(0),
            BLOCK_I[0]: (rawi * s_i).reshape(1, 1, 256, 1024),
            BLOCK_I[1]: ((Ki * rawi).sum(0) - mean_i * gif.sum(0)) * rstd_i, BLOCK_I[2]: gif.sum(0)}


def grad_and_bound(x, c31, c3, packed, stats, labels, mask, weight, label_smoothing, acts):
    """(g64, C, loss64), packed: the float64 gradient at the fp32 activations, and the same contraction over absolute values.
    The 26 tensors above conv5_2 take ``icnet_bneck_train_oracle.grad_and_bound`` on the fp32 conv5_2 (the input their kernels
    read).  The nine new ones extend its contraction: the |K_r| pull-back of conv5_3's reduce layer onto conv5_2's alive units,
    plus the shortcut (the alive units of conv5_3 straight onto conv5_2), contracted below with section 42's terms
      kernel   |s| sum_p |input| gabs     beta   sum_p gabs     gamma   rstd sum_p gabs (|input| * |K| + |mean|)."""
    r2_32, a2_32, c52_32, r32, a32, c53_32, s53_32, f1_32, sub24_32, sub12_32, logits32 = acts
    k = classes_of(packed)
    loss, g = loss_and_grad(x, c31, c3, packed, stats, labels, mask, weight, label_smoothing, acts)
    p26, st26 = np.asarray(packed)[BLOCK_FLOATS:], np.asarray(stats)[STATS_OWN:]
    g26, c26, _ = bo.grad_and_bound(c52_32, c31, c3, p26, st26, labels, mask, weight, label_smoothing, tuple(acts[3:]))
    ab = ifo.pixel_bound(logits32, labels, mask, k, weight, label_smoothing)
    xt, _, _, W = _tensors(np.abs(x), c31, c3, np.abs(np.asarray(packed)), grad=False)
    V = {n: torch.zeros(s, dtype=torch.float64, requires_grad=True) for n, s in zip(BLOCK, shapes(k))}
    mr2, vr2, m32, v32, mi2, vi2, bstats = split_stats(stats)
    mr, vr, m3, v3, pstats = bo.split_stats(bstats)
    m0, v0, ystats = po.split_stats(pstats)
    m1, v1, cstats = ipo.split_stats(ystats)
    mc, vc, md, vd, fstats = ico.split_stats(cstats)
    ma, va, mb, vb = ifo.split_stats(fstats)
    rr2, r32_, ri2, rr, r3, r0, r1, rc, ra = (1.0 / torch.sqrt(v + EPS) for v in (vr2, v32, vi2, vr, v3, v0, v1, vc, va))
    absf = lambda t: torch.as_tensor(np.abs(np.asarray(t, dtype=np.float64)))
    alive = lambda t: torch.as_tensor((np.asarray(t) > 0).astype(np.float64))
    Kr2, Ki2 = W[BLOCK_R[0]].reshape(1024, 256), W[BLOCK_I[0]].reshape(256, 1024)
    lin_r2 = ((xt @ V[BLOCK_R[0]].reshape(1024, 256)) * (W[BLOCK_R[1]] * rr2)
              + V[BLOCK_R[1]] * rr2 * (xt @ Kr2 + mr2.abs()) + V[BLOCK_R[2]])
    xr = absf(r2_32)
    lin_32 = (conv3(alive(r2_32) * lin_r2, W[BLOCK_3[0]]) * (W[BLOCK_3[1]] * r32_)
              + conv3(xr, V[BLOCK_3[0]]) * (W[BLOCK_3[1]] * r32_)
              + V[BLOCK_3[1]] * r32_ * (conv3(xr, W[BLOCK_3[0]]) + m32.abs()) + V[BLOCK_3[2]])
    xa = absf(a2_32)
    lin52 = (((alive(a2_32) * lin_32) @ Ki2) * (W[BLOCK_I[1]] * ri2)
             + (xa @ V[BLOCK_I[0]].reshape(256, 1024)) * (W[BLOCK_I[1]] * ri2)
             + V[BLOCK_I[1]] * ri2 * (xa @ Ki2 + mi2.abs()) + V[BLOCK_I[2]])
    u = alive(c52_32) * lin52
    # above conv5_2 only the pull-backs remain: the tensors there have their own contraction
    Q, P, B, N = po.BLOCK, ipo.BLOCK, ico.BLOCK, ifo.NAMES
    linr = (u @ W[bo.BLOCK_R[0]].reshape(1024, 256)) * (W[bo.BLOCK_R[1]] * rr)
    lin3 = conv3(alive(r32) * linr, W[bo.BLOCK_3[0]]) * (W[bo.BLOCK_3[1]] * r3)
    lin53 = ((alive(a32) * lin3) @ W[Q[0]].reshape(256, 1024)) * (W[Q[1]] * r0) + u
    lin32 = (po.ppm_forward(alive(c53_32) * lin53) @ W[P[0]].reshape(1024, 256)) * (W[P[1]] * r1)
    lin24 = ifo.conv_dilated(iho.resize_legacy(alive(f1_32) * lin32, 2), W[B[0]]) * (W[B[1]] * rc)
    lin12 = ifo.conv_dilated(iho.resize_legacy(alive(sub24_32) * lin24, 2), W[N[0]]) * (W[N[1]] * ra)
    lq = iho.resize_legacy(alive(sub12_32) * lin12, 2) @ W[N[6]].reshape(128, k)
    (iho.resize_legacy(lq, 4) * ab).sum().backward()
    c9 = np.concatenate([V[n].grad.numpy().reshape(-1) for n in BLOCK])
    # above conv5_2 this oracle's gradient is the bottleneck oracle's on the fp32 conv5_2
    assert np.abs(g[BLOCK_FLOATS:] - g26).max() <= 1e-9 * max(np.abs(g26).max(), 1e-300)
    return g, np.concatenate([c9, c26]), loss


def workgroups(n, h32, w32, max_workgroups=0):
    """(pixel tiles, split-K groups) of every weight gradient of the link: 32-pixel tiles strided over at most 16 groups"""
    return bo.workgroups(n, h32, w32, max_workgroups)


def kappa(name, n, h32, w32, k, weight, max_workgroups=0):
    """the error-bound factor of the gradient test.  The bottleneck trainer's 26 tensors keep section 42's
    (their bits are its bits on the same conv5_2).  The nine new tensors stand behind one value of g52 = dL/dconv5_2:
      section 42's chain behind one value of gr    (icnet_bneck_train_oracle.kappa's kgr; g53's chain is shorter)
      3 + 1                                        s_r = gamma / sqrt(var + eps); the product s_r gr, rounded once when staged
      256                                          k_icnet_bneck2_dx_red: one accumulator adds its products in ascending co
      1                                            the add of g53
    conv5_2's increase layer's three stand right behind it (section 41's terms); its 3 x 3's three behind g3' (3 + 1 + 1024 more)
    and its reduce layer's three behind gr' (3 + 1 + 9 * 256 more), exactly as section 42 states them for conv5_3; then, per
    tensor,
      32 ceil(tiles / G) + G                       the matrix-core chain over the group's pixels and the fold
      3 + 2                                        s (kernel); the two final products
      ci + 2 + 3 + 1                               gamma: the ci chain (256; 9 * 256 and the 9 tap sums; 1024), - mean dBeta,
                                                   rstd, the scale"""
    if name in bo.NAMES:
        return bo.kappa(name, n, h32, w32, k, weight, max_workgroups)
    tiles, groups = workgroups(n, h32, w32, max_workgroups)
    pixel = PIXEL_TILE * -(-tiles // groups) + groups
    # section 42's chain behind gr is what its kappa of the reduce layer's beta holds in front of that layer's own pixel chain,
    # fold and final product: taken from there, so that the two derivations cannot drift apart
    kgr = bo.kappa(bo.BLOCK_R[2], n, h32, w32, k, weight, max_workgroups) - pixel - 1
    kg52 = kgr + 3 + 1 + RED_CHAIN + 1
    kg3 = kg52 + 3 + 1 + bo.INC_CHAIN
    kgr2 = kg3 + 3 + 1 + bo.DX3_CHAIN
    behind, ci = {BLOCK_I: (kg52, 256), BLOCK_3: (kg3, 9 * 256 + 9), BLOCK_R: (kgr2, 1024)}[
        BLOCK_I if name in BLOCK_I else BLOCK_3 if name in BLOCK_3 else BLOCK_R]
    chain = behind + pixel
    if name.endswith(".kernel"):
        return chain + 3 + 2
    if name.endswith(".beta"):
        return chain + 1
    return chain + ci + 2 + 3 + 1


def coherent_case(seed, n, h, w, k):
    """(conv5_1, conv3_1, conv3_sub1, {name: weights}, stats, labels, mask) with the signs along the whole backward path in
    agreement (``icnet_bneck_train_oracle.coherent_case``'s recipe, one block further down): its arrays above conv5_2,
    non-negative kernels with positive gammas in conv5_2's three layers over a non-negative conv5_1, so that g53, gr, g52 and the
    link's g3' and gr' have one sign at every pixel and channel.  conv5_1 carries a factor per pixel (the last pixel the largest
    one, so that it is alive) -- within 0.8 .. 1.2, narrower than section 42's, so that the units' own variation and not the pixel
    decides the masks: conv5_2's dead units then are not conv5_3's, and leaving conv5_2's mask out, or taking conv5_3's for it,
    lets g53 through where it must not pass -- and the 3 x 3's centre tap is four times the others; conv5_3's reduce kernel gets a
    factor per input channel (0.2 .. 1.8), so that reading it along the wrong axis changes the pull-back; each of the three layers' betas puts the 30 %
    quantile of every channel's pre-activation (the increase layer's with its shortcut) at 0, so that the three new ReLU masks
    vary over the map.  The betas of conv5_3's three layers and of conv5_4_k1 are then placed the same way on the maps that
    result from THIS conv5_2, and the head is rescaled to logits within +-1."""
    _, c31, c3, d26, stats26, labels, mask = bo.coherent_case(seed, n, h, w, k)
    rng = np.random.default_rng(seed + 277)
    f = rng.uniform(0.8, 1.2, (n, h, w, 1))
    f[-1, -1, -1] = 1.2
    x = (np.abs(rng.standard_normal((n, h, w, 1024)) * 0.3) * f).astype(np.float32)
    own = np.concatenate(_own_stats(rng)).astype(np.float32)
    stats = np.concatenate([own, stats26]).astype(np.float32)
    d = dict(d26)
    d[BLOCK_R[0]] = rng.uniform(0.0, 0.004, (1, 1, 1024, 256)).astype(np.float32)
    K3 = rng.uniform(0.0, 0.003, (3, 3, 256, 256))
    K3[1, 1] *= 4.0
    d[BLOCK_3[0]] = K3.astype(np.float32)
    d[BLOCK_I[0]] = rng.uniform(0.0, 0.08, (1, 1, 256, 1024)).astype(np.float32)
    d[BLOCK_R[1]], d[BLOCK_3[1]] = (rng.uniform(0.5, 1.5, 256).astype(np.float32) for _ in range(2))
    # conv5_3's reduce kernel, drawn iid above, gets a factor per INPUT channel: the kernel read along the wrong axis then pulls gr
    # back onto other channels of conv5_2 than the right one does
    d[bo.BLOCK_R[0]] = (d[bo.BLOCK_R[0]] * rng.uniform(0.2, 1.8, (1, 1, 1024, 1))).astype(np.float32)
    d[BLOCK_I[1]] = rng.uniform(0.5, 1.5, 1024).astype(np.float32)
    o64, x64 = own.astype(np.float64), x.astype(np.float64)
    f64 = lambda name: d[name].astype(np.float64)

    def place(lin, gamma, mean, var):
        """beta and the layer's output for pre = s (lin - mean) + beta with the 30 % quantile of every channel at 0"""
        s = gamma.astype(np.float64) / np.sqrt(var + EPS)
        beta = (s * (mean - np.quantile(lin, 0.3, axis=0))).astype(np.float32)
        return beta, np.maximum(lin * s + (beta.astype(np.float64) - mean * s), 0.0)

    def block(x_in, R, T, I, mr, vr, m3, v3, mi, vi):
        """the three betas of one Bneck(256, 1024, 1, 4) on ``x_in`` [pixels as n, h, w, 1024] -> its output"""
        d[R[2]], r = place(x_in.reshape(-1, 1024) @ f64(R[0]).reshape(1024, 256), d[R[1]], mr, vr)
        lin3 = conv3(torch.as_tensor(r.reshape(n, h, w, 256)), torch.as_tensor(f64(T[0]))).numpy().reshape(-1, 256)
        d[T[2]], a = place(lin3, d[T[1]], m3, v3)
        s_i = f64(I[1]) / np.sqrt(vi + EPS)
        lin = (a @ f64(I[0]).reshape(256, 1024)) * s_i + x_in.reshape(-1, 1024)
        d[I[2]] = (mi * s_i - np.quantile(lin, 0.3, axis=0)).astype(np.float32)
        return np.maximum(lin + (d[I[2]].astype(np.float64) - mi * s_i), 0.0).reshape(n, h, w, 1024)

    c52 = block(x64, BLOCK_R, BLOCK_3, BLOCK_I, o64[:256], o64[256:512], o64[512:768], o64[768:1024], o64[1024:2048], o64[2048:])
    s26 = stats26.astype(np.float64)
    block(c52, bo.BLOCK_R, bo.BLOCK_3, po.BLOCK, s26[:256], s26[256:512], s26[512:768], s26[768:1024],
          s26[bo.STATS_OWN:bo.STATS_OWN + 1024], s26[bo.STATS_OWN + 1024:bo.STATS_OWN + 2048])
    d = {name: np.asarray(d[name]).astype(np.float32) for name in NAMES}
    # conv5_4_k1's beta on the conv5_3_sum that results, as the pooling recipe places it; then the head's scale
    s53 = bneck2_forward(x, c31, c3, pack(d), stats)[6]
    k1 = d["conv5_4_k1.kernel"].astype(np.float64).reshape(1024, 256)
    lo = bo.STATS_OWN + po.STATS_OWN
    m1, v1 = s26[lo:lo + 256], s26[lo + 256:lo + 512]
    s1 = d["conv5_4_k1.gamma"].astype(np.float64) / np.sqrt(v1 + EPS)
    d["conv5_4_k1.beta"] = (m1 * s1 - s1 * np.quantile(s53.reshape(-1, 1024) @ k1, 0.3, axis=0)).astype(np.float32)
    top = np.abs(bneck2_forward(x, c31, c3, pack(d), stats)[10]).max()
    d["conv6_cls.kernel"] = (d["conv6_cls.kernel"] / np.float32(max(top, 1e-6))).astype(np.float32)
    return x, c31, c3, d, stats, labels, mask


def adam_bneck2(w, m, v, g, k, lr, beta1, beta2, eps, b1p, b2p, l1=0.0, l2=0.0):
    """numpy float32 ApplyAdam on the packed vector: the l1_l2 regulariser goes to the twelve kernels only"""
    out = [np.array(x, dtype=np.float32) for x in (w, m, v)]
    for name, (lo, hi) in offsets(k).items():
        reg = dict(l1=l1, l2=l2) if name in KERNELS else {}
        res = fto.adam_step(w[lo:hi], m[lo:hi], v[lo:hi], g[lo:hi], lr, beta1, beta2, eps, b1p, b2p, **reg)
        for o, r in zip(out, res):
            o[lo:hi] = r
    return tuple(out)
