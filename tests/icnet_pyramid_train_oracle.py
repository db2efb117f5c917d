"""TEST INFRASTRUCTURE ONLY -- never imported by the product.

Float64 restatement of the training step of ICNet's pyramid head, from ``conv5_3_sum``, ``conv3_1`` and
``conv3_sub1`` to the loss:
  * ``conv5_4_k1 = relu(BN(conv5_3_sum @ kernel))``: a 1 x 1 convolution, 1024 -> 256, under inference batch-norm;
  * the cascade head on it: ``icnet_cascade_train_oracle``'s restatement (both fusion blocks, the head, the 4x resize, the loss).
Autograd supplies the gradients (``relu'(0) = 0``); ``k1_backward`` restates the new layer's backward pass term by term, the
way the kernels compute it, and can leave one step out or get it wrong (the discrimination test).  The seventeen variables are
packed as the product packs them: ``conv5_4_k1``'s three, then ``icnet_cascade_train_oracle``'s fourteen.
"""
import numpy as np
import torch
import torch.nn.functional as F

import final_train_oracle as fto
import icnet_cascade_train_oracle as ico
import icnet_fusion_train_oracle as ifo
import icnet_head_train_oracle as iho

BLOCK = ("conv5_4_k1.kernel", "conv5_4_k1.gamma", "conv5_4_k1.beta")
NAMES = BLOCK + ico.NAMES
KERNELS = (BLOCK[0],) + ico.KERNELS  # what the l1_l2 regulariser reaches
BLOCK_FLOATS = 1024 * 256 + 2 * 256
PIXEL_TILE = 32    # pixels of conv5_4_k1 per split-K tile of k_icnet_pyramid_wgrad
MAX_WG = 16        # split-K groups of that launch
DX_CHAIN = 9 * 128  # products k_icnet_cascade_dx<256> adds one after the other on one accumulator
EPS = ifo.EPS
WRONG = ("no_relu_mask", "half_pixel", "no_scale", "dilation_1", "pad_after")
# mistakes of the weight-gradient, fold and gamma kernels themselves: the last pixel of the map left out of the contraction (a
# ragged pixel tile cut short), every pixel of index >= 64 left out (a split-K group dropped at the 32-pixel tiles of the
# ragged shape), dGamma without its - mean dBeta term, a kernel gradient 10 % off
WRONG_LOCAL = ("drop_last_pixel", "drop_last_group", "no_mean_term", "kernel_10_percent")


def shapes(k):
    return ((1, 1, 1024, 256), (256,), (256,)) + ico.shapes(k)


def offsets(k):
    out, lo = {}, 0
    for name, shp in zip(NAMES, shapes(k)):
        out[name] = (lo, lo + int(np.prod(shp)))
        lo = out[name][1]
    return out


def floats(k):
    return BLOCK_FLOATS + ico.floats(k)


def classes_of(packed):
    return ico.classes_of(np.asarray(packed)[BLOCK_FLOATS:])


def unpack(packed, k=None):
    packed = np.asarray(packed)
    k = classes_of(packed) if k is None else k
    off = offsets(k)
    return {n: packed[off[n][0]:off[n][1]].reshape(s) for n, s in zip(NAMES, shapes(k))}


def pack(d):
    return np.concatenate([np.asarray(d[n]).reshape(-1) for n in NAMES])


def split_stats(stats):
    """[2 * 256 + 8 * 128] -> mean, variance of conv5_4_k1 (float64 torch) and the cascade trainer's [8 * 128] (numpy)"""
    stats = np.asarray(stats, dtype=np.float64)
    return torch.as_tensor(stats[:256]), torch.as_tensor(stats[256:512]), stats[512:]


def case(seed, n, h, w, k):
    """the arrays of one gradient case: ``conv5_3_sum`` >= 0 (a sum of ReLU outputs and their averages) and a kernel of both
    signs sized so that conv5_4_k1's pre-activation has both signs; the rest as the cascade test draws it"""
    rng = np.random.default_rng(seed)
    c53 = np.abs(rng.standard_normal((n, h, w, 1024)) * 0.7).astype(np.float32)
    c31 = (rng.standard_normal((n, 2 * h, 2 * w, 256)) * 0.7).astype(np.float32)
    c3 = (rng.standard_normal((n, 4 * h, 4 * w, 64)) * 0.7).astype(np.float32)
    d = {"conv5_4_k1.kernel": rng.uniform(-0.05, 0.05, (1, 1, 1024, 256)), "conv5_4_k1.gamma": rng.uniform(0.5, 1.5, 256),
         "conv5_4_k1.beta": rng.uniform(-0.3, 0.3, 256),
         "conv_sub4.kernel": rng.uniform(-0.03, 0.03, (3, 3, 256, 128)), "conv_sub4.gamma": rng.uniform(0.5, 1.5, 128),
         "conv_sub4.beta": rng.uniform(-0.3, 0.3, 128), "conv3_1_sub2_proj.kernel": rng.uniform(-0.08, 0.08, (1, 1, 256, 128)),
         "conv3_1_sub2_proj.gamma": rng.uniform(-1.5, 1.5, 128), "conv3_1_sub2_proj.beta": rng.uniform(-0.3, 0.3, 128),
         "conv_sub2.kernel": rng.uniform(-0.04, 0.04, (3, 3, 128, 128)), "conv_sub2.gamma": rng.uniform(0.5, 1.5, 128),
         "conv_sub2.beta": rng.uniform(-0.3, 0.3, 128), "conv3_sub1_proj.kernel": rng.uniform(-0.15, 0.15, (1, 1, 64, 128)),
         "conv3_sub1_proj.gamma": rng.uniform(-1.5, 1.5, 128), "conv3_sub1_proj.beta": rng.uniform(-0.3, 0.3, 128),
         "conv6_cls.kernel": rng.uniform(-0.3, 0.3, (1, 1, 128, k)), "conv6_cls.bias": rng.uniform(-0.5, 0.5, k)}
    d = {name: v.astype(np.float32) for name, v in d.items()}
    labels = rng.integers(0, k, (n, 32 * h, 32 * w)).astype(np.uint8)
    mask = (rng.uniform(size=labels.shape) > 0.25).astype(np.float32)
    labels[(rng.uniform(size=labels.shape) < 0.3) & (mask == 0)] = 255  # ignored pixels: label 255 under mask 0
    labels[0, 0, 0], mask[0, 0, 0] = k, 1.0                             # a label >= K under mask 1: the all-off row
    labels[-1, -1, -1], mask[-1, -1, -1] = 0, 1.0
    return c53, c31, c3, d, labels, mask


def draw_stats(seed):
    """moving statistics for the gradient cases: conv5_4_k1's two rows of 256, then the cascade trainer's eight of 128"""
    rng = np.random.default_rng(seed)
    rows = [rng.uniform(-0.3, 0.3, 256), rng.uniform(0.5, 2.0, 256)]
    rows += [rng.uniform(0.5, 2.0, 128) if i % 2 else rng.uniform(-0.3, 0.3, 128) for i in range(8)]
    return np.concatenate(rows).astype(np.float32)


def coherent_case(seed, n, h, w, k):
    """(conv5_3_sum, conv3_1, conv3_sub1, {name: weights}, stats, labels, mask) with the signs along the whole backward path in
    agreement, so that the contraction over magnitudes C_j stays within a small factor of |g_j| for conv5_4_k1's three tensors
    and the bound kappa 2^-24 C_j bites (icnet_highres_train_oracle.case(coherent=True)'s recipe, one branch further down):
    non-negative inputs, non-negative kernels and positive gammas in conv5_4_k1, both fusion blocks' convolutions and their
    projections, one label (class 0) everywhere under a head whose class-0 column is positive and dominates, logits within
    +-1 of the zero bias.  Then dL/dsub12_sum, g24, du16 and g32 have one sign at every pixel and channel.  conv5_3_sum carries
    a factor per pixel and conv5_4_k1's beta puts the 30 % quantile of each channel's pre-activation at 0, so that its ReLU
    mask varies over the map; its moving mean stays, of both signs, a few per cent of the accumulator."""
    rng = np.random.default_rng(seed)
    c53 = (np.abs(rng.standard_normal((n, h, w, 1024)) * 0.7) * rng.uniform(0.3, 1.7, (n, h, w, 1))).astype(np.float32)
    c31 = np.abs(rng.standard_normal((n, 2 * h, 2 * w, 256)) * 0.7).astype(np.float32)
    c3 = np.abs(rng.standard_normal((n, 4 * h, 4 * w, 64)) * 0.7).astype(np.float32)
    stats = draw_stats(seed + 1)
    d = {"conv5_4_k1.kernel": rng.uniform(0.0, 0.05, (1, 1, 1024, 256)), "conv5_4_k1.gamma": rng.uniform(0.5, 1.5, 256),
         "conv_sub4.kernel": rng.uniform(0.0, 0.01, (3, 3, 256, 128)), "conv_sub4.gamma": rng.uniform(0.5, 1.5, 128),
         "conv_sub4.beta": rng.uniform(0.5, 1.0, 128), "conv3_1_sub2_proj.kernel": rng.uniform(0.0, 0.02, (1, 1, 256, 128)),
         "conv3_1_sub2_proj.gamma": rng.uniform(0.5, 1.5, 128), "conv3_1_sub2_proj.beta": rng.uniform(0.5, 1.0, 128),
         "conv_sub2.kernel": rng.uniform(0.0, 0.01, (3, 3, 128, 128)), "conv_sub2.gamma": rng.uniform(0.5, 1.5, 128),
         "conv_sub2.beta": rng.uniform(0.5, 1.0, 128), "conv3_sub1_proj.kernel": rng.uniform(0.0, 0.05, (1, 1, 64, 128)),
         "conv3_sub1_proj.gamma": rng.uniform(0.5, 1.5, 128), "conv3_sub1_proj.beta": rng.uniform(0.5, 1.0, 128)}
    k1 = d["conv5_4_k1.kernel"].astype(np.float32).astype(np.float64).reshape(1024, 256)
    m1, v1 = stats[:256].astype(np.float64), stats[256:512].astype(np.float64)
    s1 = d["conv5_4_k1.gamma"].astype(np.float32).astype(np.float64) / np.sqrt(v1 + EPS)
    q = np.quantile(c53.astype(np.float64).reshape(-1, 1024) @ k1, 0.3, axis=0)
    if n * h * w == 1:
        q = q * np.where(np.arange(256) % 3 == 0, 1.5, 0.5)  # one pixel: a third of the channels dead
    d["conv5_4_k1.beta"] = m1 * s1 - s1 * q
    head = rng.uniform(-0.05, 0.05, (1, 1, 128, k))
    head[..., 0] = rng.uniform(0.5, 1.0, (1, 1, 128))
    d["conv6_cls.kernel"], d["conv6_cls.bias"] = head, np.zeros(k)
    d = {name: np.asarray(d[name]).astype(np.float32) for name in NAMES}
    top = np.abs(pyramid_forward(c53, c31, c3, pack(d), stats)[3]).max()
    d["conv6_cls.kernel"] = (d["conv6_cls.kernel"] / np.float32(max(top, 1e-6))).astype(np.float32)
    labels = np.zeros((n, 32 * h, 32 * w), np.uint8)
    mask = (rng.uniform(size=labels.shape) > 0.25).astype(np.float32)
    return c53, c31, c3, d, stats, labels, mask


def _tensors(c53, c31, c3, packed, grad=True):
    W = {n: torch.as_tensor(np.asarray(v, dtype=np.float64).copy()).requires_grad_(grad) for n, v in unpack(packed).items()}
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))
    return t(c53), t(c31), t(c3), W


def _pre32(x53, W, m1, v1):
    s1 = W[BLOCK[1]] / torch.sqrt(v1 + EPS)
    return (x53 @ W[BLOCK[0]].reshape(1024, 256)) * s1 + (W[BLOCK[2]] - m1 * s1)


def pyramid_forward(c53, c31, c3, packed, stats):
    """-> (conv5_4_k1, sub24_sum, sub12_sum, full-resolution logits) float64 numpy"""
    x53, _, _, W = _tensors(c53, c31, c3, packed, grad=False)
    m1, v1, cstats = split_stats(stats)
    f1 = torch.relu(_pre32(x53, W, m1, v1)).numpy()
    return (f1,) + ico.cascade_forward(f1, c31, c3, np.asarray(packed)[BLOCK_FLOATS:], cstats)


def _loss(x53, x31, x3, W, stats, labels, mask, weight, label_smoothing, f1_32, sub24_32, sub12_32, logits32, keep=None):
    """the float64 loss as a torch scalar; ``keep``: a dict that receives the pre-activation of sub24_sum (gradient retained)
    and the float64 conv5_4_k1"""
    k = int(W[NAMES[-1]].numel())
    on, off, w32, c_w = fto.xent_constants(k, weight, label_smoothing)
    s = fto.mask_scale(mask)
    m1, v1, cstats = split_stats(stats)
    mc, vc, md, vd, fstats = ico.split_stats(cstats)
    f1 = ico._pinned_relu(_pre32(x53, W, m1, v1), f1_32)
    pre24 = ico._pre24(f1, x31, W, mc, vc, md, vd)
    if keep is not None:
        pre24.retain_grad()
        keep["pre24"], keep["f1"] = pre24, f1
    s24 = ico._pinned_relu(pre24, sub24_32)
    ma, va, mb, vb = ifo.split_stats(fstats)
    N = ifo.NAMES
    acc_a = ifo.conv_dilated(iho.resize_legacy(s24, 2), W[N[0]])
    acc_b = x3 @ W[N[3]].reshape(64, 128)
    sa, sb = W[N[1]] / torch.sqrt(va + EPS), W[N[4]] / torch.sqrt(vb + EPS)
    s12 = ico._pinned_relu(acc_a * sa + (W[N[2]] - ma * sa) + acc_b * sb + (W[N[5]] - mb * sb), sub12_32)
    _, lg = iho.head_logits(s12, W[N[6]].reshape(128, k), W[N[7]])
    if logits32 is not None:
        lg = lg + (torch.as_tensor(np.asarray(logits32, dtype=np.float64)) - lg).detach()
    y = fto.one_hot(labels, k, on, off)
    mk = torch.as_tensor(np.asarray(mask, dtype=np.float64))
    return fto.pixel_loss(lg, y, mk, w32, c_w, True).sum() * s


def loss_and_grad(c53, c31, c3, packed, stats, labels, mask, weight, label_smoothing, f1_32=None, sub24_32=None, sub12_32=None,
                  logits32=None):
    """float64 (loss, packed gradient).  With ``f1_32`` / ``sub24_32`` / ``sub12_32`` / ``logits32`` the three ReLUs and the loss
    are evaluated at those (fp32) values -- the point the GPU evaluates."""
    x53, x31, x3, W = _tensors(c53, c31, c3, packed)
    loss = _loss(x53, x31, x3, W, stats, labels, mask, weight, label_smoothing, f1_32, sub24_32, sub12_32, logits32)
    loss.backward()
    return float(loss.detach()), pack({n: W[n].grad.numpy() for n in NAMES})


def _adjoint_half_pixel(y):
    """the adjoint of the half-pixel-centre 2x bilinear resize (NOT the forward path's): the wrong resize adjoint"""
    y = torch.as_tensor(np.asarray(y, dtype=np.float64)).permute(0, 3, 1, 2)
    x = torch.zeros(y.shape[0], y.shape[1], y.shape[2] // 2, y.shape[3] // 2, dtype=torch.float64, requires_grad=True)
    F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False).backward(y)
    return x.grad.permute(0, 2, 3, 1).numpy()


def k1_backward(c53, c31, c3, packed, stats, labels, mask, weight, label_smoothing, f1_32=None, sub24_32=None, sub12_32=None,
                logits32=None, wrong=None):
    """conv5_4_k1's three gradients restated the way the kernels compute them, from autograd's dL/d(pre-activation of sub24_sum):
    gs = s_c g24; du16 = the transposed dilated convolution through conv_sub4; g32 = relu'(conv5_4_k1) adjoint_2x(du16);
    dK = s x^T g32, dBeta = sum_p g32, dGamma = sum_p g32 (acc - mean) rstd.  ``wrong``: one of ``WRONG`` -- that step is left
    out or done the wrong way; or one of ``WRONG_LOCAL``.  -> {name: float64 array} for ``BLOCK``"""
    assert wrong is None or wrong in WRONG + WRONG_LOCAL
    x53, x31, x3, W = _tensors(c53, c31, c3, packed)
    keep = {}
    _loss(x53, x31, x3, W, stats, labels, mask, weight, label_smoothing, f1_32, sub24_32, sub12_32, logits32, keep).backward()
    g24 = keep["pre24"].grad.numpy()  # behind sub24_sum's ReLU, normalised
    Wn = {n: v.detach().numpy() for n, v in W.items()}
    stats = np.asarray(stats, dtype=np.float64)
    m1, v1, vc = stats[:256], stats[256:512], stats[512 + 128:512 + 256]
    sc = Wn["conv_sub4.gamma"] / np.sqrt(vc + EPS)
    gs = g24 if wrong == "no_scale" else g24 * sc
    Kc = Wn["conv_sub4.kernel"]
    d = 1 if wrong == "dilation_1" else 2
    pb = 0 if wrong == "pad_after" else d  # forward: y[p] = sum_k K[k] u[p + d k - pb]
    n, h16, w16, _ = gs.shape
    du = np.zeros((n, h16, w16, 256))
    for kh in range(3):
        for kw in range(3):
            oy, ox = d * kh - pb, d * kw - pb  # u[q] feeds y[q - o]: du[q] += gs[q - o] K[k]^T
            ys, xs = max(oy, 0), max(ox, 0)
            ye, xe = min(h16 + oy, h16), min(w16 + ox, w16)
            if ys >= ye or xs >= xe:
                continue  # a padding tap contributes nothing
            du[:, ys:ye, xs:xe] += gs[:, ys - oy:ye - oy, xs - ox:xe - ox] @ Kc[kh, kw].T
    g32 = _adjoint_half_pixel(du) if wrong == "half_pixel" else ico.adjoint_2x(du)
    f1 = keep["f1"].detach().numpy()
    if wrong != "no_relu_mask":
        g32 = g32 * (f1 > 0)
    x = np.asarray(c53, dtype=np.float64).reshape(-1, 1024)
    g = g32.reshape(-1, 256)
    if wrong == "drop_last_pixel":
        x, g = x[:-1], g[:-1]
    if wrong == "drop_last_group":
        x, g = x[:64], g[:64]
    rstd = 1.0 / np.sqrt(v1 + EPS)
    K1 = Wn[BLOCK[0]].reshape(1024, 256)
    raw = x.T @ g
    if wrong == "kernel_10_percent":
        raw = 1.1 * raw
    mean = 0.0 if wrong == "no_mean_term" else m1
    # dGamma as the device forms it: contracted from the folded (here: possibly wrong) weight gradient
    return {BLOCK[0]: (raw * (Wn[BLOCK[1]] * rstd)).reshape(1, 1, 1024, 256),
            BLOCK[1]: ((K1 * raw).sum(0) - mean * g.sum(0)) * rstd, BLOCK[2]: g.sum(0)}


def grad_and_bound(c53, c31, c3, packed, stats, labels, mask, weight, label_smoothing, f1_32, sub24_32, sub12_32, logits32):
    """(g64, C, loss64), packed: the float64 gradient at the fp32 activations, and the same contraction over absolute values.
    ``icnet_cascade_train_oracle.grad_and_bound``'s, with |conv5_4_k1| (fp32) as the cascade's low-resolution input and one more
    term under sub24_sum's alive units: its |conv_sub4| pull-back onto the alive units of conv5_4_k1, contracted there with
      kernel   |s| sum_p |x| gabs32     beta   sum_p gabs32     gamma   rstd sum_p gabs32 (|x| @ |K| + |mean|)."""
    k = classes_of(packed)
    loss, g = loss_and_grad(c53, c31, c3, packed, stats, labels, mask, weight, label_smoothing, f1_32, sub24_32, sub12_32,
                            logits32)
    a = ifo.pixel_bound(logits32, labels, mask, k, weight, label_smoothing)
    x53, x31, x3, W = _tensors(np.abs(c53), np.abs(c31), np.abs(c3), np.abs(np.asarray(packed)), grad=False)
    V = {n: torch.zeros(s, dtype=torch.float64, requires_grad=True) for n, s in zip(NAMES, shapes(k))}
    m1, v1, cstats = split_stats(stats)
    mc, vc, md, vd, fstats = ico.split_stats(cstats)
    ma, va, mb, vb = ifo.split_stats(fstats)
    r1, rc, rd, ra, rb = (1.0 / torch.sqrt(v + EPS) for v in (v1, vc, vd, va, vb))
    B, N = ico.BLOCK, ifo.NAMES
    absf = lambda t: torch.as_tensor(np.abs(np.asarray(t, dtype=np.float64)))
    alive = lambda t: torch.as_tensor((np.asarray(t) > 0).astype(np.float64))
    lin32 = ((x53 @ V[BLOCK[0]].reshape(1024, 256)) * (W[BLOCK[1]] * r1)
             + V[BLOCK[1]] * r1 * (x53 @ W[BLOCK[0]].reshape(1024, 256) + m1.abs()) + V[BLOCK[2]])
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
    (iho.resize_legacy(lq, 4) * a).sum().backward()
    return g, pack({n: V[n].grad.numpy() for n in NAMES}), loss


def workgroups(n, h32, w32, max_workgroups=0):
    """(pixel tiles, split-K groups) of k_icnet_pyramid_wgrad"""
    tiles = -(-n * h32 * w32 // PIXEL_TILE)
    g = min(tiles, MAX_WG)
    return tiles, (min(g, max_workgroups) if max_workgroups > 0 else g)


def kappa(name, n, h32, w32, k, weight, max_workgroups=0):
    """the error-bound factor of the gradient test.  The cascade trainer's fourteen tensors keep section
    29's (their bits are its bits on the same conv5_4_k1).  conv5_4_k1's three share the chain behind one value of g32 =
    dL/dconv5_4_k1:
      section 29's chain behind one value of g24   16 (K + 8) (1 + cond) + 64 + 3 + 16 + 4 + K + 3 + 1 + 9 * 128 + 9
      3 + 1                                        s_c = gamma / sqrt(var + eps); the product s_c g24, rounded once when staged
      9 * 128                                      k_icnet_cascade_dx<256>: one accumulator adds all its products one after the
                                                   other (quarter of co, tap, co within the quarter)
      9                                            the resize adjoint's at most 3 x 3 fmaf terms
    then, per tensor,
      32 ceil(tiles / G) + G                       the matrix-core chain over the group's pixels (conv5_3_sum is an input: no
                                                   rounding of its own) and the fold
      3 + 2                                        s (kernel); the two final products
      1024 + 2 + 3 + 1                             gamma: the ci chain, - mean dBeta, rstd, the scale"""
    if name in ico.NAMES:
        return ico.kappa(name, n, h32, w32, k, weight, max_workgroups)
    tiles, groups = workgroups(n, h32, w32, max_workgroups)
    w32f = float(np.float32(weight))
    cond = 1.0 / np.log(w32f) if w32f > 1.0 else 0.0
    kg24 = 16 * (k + 8) * (1.0 + cond) + 64 + 3 + 16 + 4 + k + 3 + 1 + ico.DX_CHAIN + 9
    kg32 = kg24 + 3 + 1 + DX_CHAIN + 9
    chain = kg32 + PIXEL_TILE * -(-tiles // groups) + groups
    if name == BLOCK[0]:
        return chain + 3 + 2
    if name == BLOCK[2]:
        return chain + 1
    return chain + 1024 + 2 + 3 + 1


def adam_pyramid(w, m, v, g, k, lr, beta1, beta2, eps, b1p, b2p, l1=0.0, l2=0.0):
    """numpy float32 ApplyAdam on the packed vector: the l1_l2 regulariser goes to the six kernels only"""
    out = [np.array(a, dtype=np.float32) for a in (w, m, v)]
    for name, (lo, hi) in offsets(k).items():
        reg = dict(l1=l1, l2=l2) if name in KERNELS else {}
        res = fto.adam_step(w[lo:hi], m[lo:hi], v[lo:hi], g[lo:hi], lr, beta1, beta2, eps, b1p, b2p, **reg)
        for o, r in zip(out, res):
            o[lo:hi] = r
    return tuple(out)


def train_float64(c53, c31, c3, packed0, stats, labels, mask, k, steps, lr, beta1, beta2, eps, weight, label_smoothing, l2):
    """``steps`` Adam steps in float64 (the regulariser on the kernels only) -> the losses before each step"""
    w = np.asarray(packed0, dtype=np.float64).copy()
    m, v = np.zeros_like(w), np.zeros_like(w)
    reg = np.zeros_like(w)
    for name in KERNELS:
        lo, hi = offsets(k)[name]
        reg[lo:hi] = 1.0
    out = []
    for t in range(1, steps + 1):
        loss, g = loss_and_grad(c53, c31, c3, w, stats, labels, mask, weight, label_smoothing)
        out.append(loss)
        g = g + reg * (2.0 * l2) * w
        alpha = lr * np.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)
        m += (g - m) * (1.0 - beta1)
        v += (g * g - v) * (1.0 - beta2)
        w -= m * alpha / (np.sqrt(v) + eps)
    return out
