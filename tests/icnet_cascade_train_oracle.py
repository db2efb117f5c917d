"""TEST INFRASTRUCTURE ONLY -- never imported by the product.

Float64 restatement of the training step of ICNet's whole cascade head, from ``conv5_4_k1``, ``conv3_1``
and ``conv3_sub1`` to the loss:
  * ``sub24_sum = relu(BN(conv_sub4(resize_2x(conv5_4_k1))) + BN(conv3_1_sub2_proj(conv3_1)))``: 3 x 3, dilation 2, TF ``SAME``
    on the legacy 2x resize, and a 1 x 1 convolution, both under inference batch-norm;
  * the last fusion block, the head, the 4x resize and the loss: ``icnet_fusion_train_oracle`` / ``icnet_head_train_oracle`` /
    ``final_train_oracle``.
Autograd supplies the gradients (``relu'(0) = 0``).  The fourteen variables are packed as the product packs them: the new
block's six, then ``icnet_fusion_train_oracle``'s eight.
"""
import numpy as np
import torch

import final_train_oracle as fto
import icnet_fusion_train_oracle as ifo
import icnet_head_train_oracle as iho

BLOCK = ("conv_sub4.kernel", "conv_sub4.gamma", "conv_sub4.beta", "conv3_1_sub2_proj.kernel", "conv3_1_sub2_proj.gamma",
         "conv3_1_sub2_proj.beta")
NAMES = BLOCK + ifo.NAMES
KERNELS = (BLOCK[0], BLOCK[3]) + ifo.KERNELS  # what the l1_l2 regulariser reaches
BLOCK_FLOATS = 328192
MAX_WG = 64        # split-K groups of the 256-channel weight-gradient launch (tiles of 4 x 8 pixels of sub24_sum)
DX_CHAIN = 9 * 128  # products k_icnet_cascade_dx adds one after the other on one accumulator
EPS = ifo.EPS


def shapes(k):
    return ((3, 3, 256, 128), (128,), (128,), (1, 1, 256, 128), (128,), (128,)) + ifo.shapes(k)


def offsets(k):
    out, lo = {}, 0
    for name, shp in zip(NAMES, shapes(k)):
        out[name] = (lo, lo + int(np.prod(shp)))
        lo = out[name][1]
    return out


def floats(k):
    return BLOCK_FLOATS + ifo.floats(k)


def classes_of(packed):
    return ifo.classes_of(np.asarray(packed)[BLOCK_FLOATS:])


def unpack(packed, k=None):
    packed = np.asarray(packed)
    k = classes_of(packed) if k is None else k
    off = offsets(k)
    return {n: packed[off[n][0]:off[n][1]].reshape(s) for n, s in zip(NAMES, shapes(k))}


def pack(d):
    return np.concatenate([np.asarray(d[n]).reshape(-1) for n in NAMES])


def split_stats(stats):
    """[8 * 128] -> mean_c, var_c, mean_d, var_d (float64 torch) and the fusion block's [4 * 128] (numpy)"""
    stats = np.asarray(stats, dtype=np.float64)
    return tuple(torch.as_tensor(stats[i * 128:(i + 1) * 128]) for i in range(4)) + (stats[512:],)


def adjoint_2x(y):
    """the adjoint of ``resize_legacy(., 2)`` restated from its weights, numpy float64 [N, 2h, 2w, C] -> [N, h, w, C]: even rows
    / columns copy, odd ones average with the +1 tap clamped to the map -- the last one collects its clamped tap twice"""
    y = np.asarray(y, dtype=np.float64)
    for axis in (1, 2):
        h = y.shape[axis] // 2
        ev, od = np.take(y, range(0, 2 * h, 2), axis), np.take(y, range(1, 2 * h, 2), axis)
        out = ev + 0.5 * od                               # tap i of u[2 i] and of u[2 i + 1]
        sl = [slice(None)] * y.ndim
        sl[axis] = slice(1, None)
        out[tuple(sl)] += 0.5 * np.take(od, range(0, h - 1), axis)   # tap i + 1 of u[2 i + 1]
        sl[axis] = slice(h - 1, h)
        out[tuple(sl)] += 0.5 * np.take(od, [h - 1], axis)           # clamped: i + 1 = h -> h - 1
        y = out
    return y


def _tensors(c54, c31, c3, packed, grad=True):
    W = {n: torch.as_tensor(np.asarray(v, dtype=np.float64).copy()).requires_grad_(grad) for n, v in unpack(packed).items()}
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))
    return t(c54), t(c31), t(c3), W


def _pre24(x54, x31, W, mc, vc, md, vd):
    acc_c = ifo.conv_dilated(iho.resize_legacy(x54, 2), W[BLOCK[0]])
    acc_d = x31 @ W[BLOCK[3]].reshape(256, 128)
    sc, sd = W[BLOCK[1]] / torch.sqrt(vc + EPS), W[BLOCK[4]] / torch.sqrt(vd + EPS)
    return acc_c * sc + (W[BLOCK[2]] - mc * sc) + acc_d * sd + (W[BLOCK[5]] - md * sd)


def _pinned_relu(pre, at32):
    """relu(pre); with ``at32`` the value is the fp32 one wherever the unit is alive there, and the unit is dead exactly where
    fp32 says so (differentiated through the float64 chain)"""
    if at32 is None:
        return torch.relu(pre)
    s32 = torch.as_tensor(np.asarray(at32, dtype=np.float64))
    return torch.where(s32 > 0, pre + (s32 - pre).detach(), torch.zeros_like(pre))


def cascade_forward(c54, c31, c3, packed, stats):
    """-> (sub24_sum, sub12_sum, full-resolution logits) float64 numpy"""
    k = classes_of(packed)
    x54, x31, x3, W = _tensors(c54, c31, c3, packed, grad=False)
    mc, vc, md, vd, fstats = split_stats(stats)
    s24 = torch.relu(_pre24(x54, x31, W, mc, vc, md, vd))
    s12, _, _ = ifo.fusion_forward(s24, x3, W, fstats)
    _, lg = iho.head_logits(s12, W[NAMES[12]].reshape(128, k), W[NAMES[13]])
    return s24.numpy(), s12.numpy(), lg.numpy()


def loss_and_grad(c54, c31, c3, packed, stats, labels, mask, weight, label_smoothing, sub24_32=None, sub12_32=None,
                  logits32=None):
    """float64 (loss, packed gradient).  With ``sub24_32`` / ``sub12_32`` / ``logits32`` both ReLUs and the loss are evaluated at
    those (fp32) values -- the point the GPU evaluates."""
    k = classes_of(packed)
    on, off, w32, c_w = fto.xent_constants(k, weight, label_smoothing)
    s = fto.mask_scale(mask)
    x54, x31, x3, W = _tensors(c54, c31, c3, packed)
    mc, vc, md, vd, fstats = split_stats(stats)
    s24 = _pinned_relu(_pre24(x54, x31, W, mc, vc, md, vd), sub24_32)
    ma, va, mb, vb = ifo.split_stats(fstats)
    F = ifo.NAMES
    acc_a = ifo.conv_dilated(iho.resize_legacy(s24, 2), W[F[0]])
    acc_b = x3 @ W[F[3]].reshape(64, 128)
    sa, sb = W[F[1]] / torch.sqrt(va + EPS), W[F[4]] / torch.sqrt(vb + EPS)
    s12 = _pinned_relu(acc_a * sa + (W[F[2]] - ma * sa) + acc_b * sb + (W[F[5]] - mb * sb), sub12_32)
    _, lg = iho.head_logits(s12, W[F[6]].reshape(128, k), W[F[7]])
    if logits32 is not None:
        lg = lg + (torch.as_tensor(np.asarray(logits32, dtype=np.float64)) - lg).detach()
    y = fto.one_hot(labels, k, on, off)
    mk = torch.as_tensor(np.asarray(mask, dtype=np.float64))
    loss = fto.pixel_loss(lg, y, mk, w32, c_w, True).sum() * s
    loss.backward()
    return float(loss.detach()), pack({n: W[n].grad.numpy() for n in NAMES})


def grad_and_bound(c54, c31, c3, packed, stats, labels, mask, weight, label_smoothing, sub24_32, sub12_32, logits32):
    """(g64, C, loss64), packed: the float64 gradient at the fp32 activations, and the same contraction over absolute values.
    ``icnet_fusion_train_oracle.grad_and_bound``'s, with |sub24_sum| (fp32) as the last block's input and one more term under
    sub12_sum's alive units: its |conv_sub2| pull-back onto the alive units of sub24_sum, contracted there with
      kernels   |s| sum_q |input| gabs24     beta   sum_q gabs24     gamma   rstd sum_q gabs24 (conv(|input|, |K|) + |mean|)."""
    k = classes_of(packed)
    loss, g = loss_and_grad(c54, c31, c3, packed, stats, labels, mask, weight, label_smoothing, sub24_32, sub12_32, logits32)
    a = ifo.pixel_bound(logits32, labels, mask, k, weight, label_smoothing)
    x54, x31, x3, W = _tensors(np.abs(c54), np.abs(c31), np.abs(c3), np.abs(np.asarray(packed)), grad=False)
    V = {n: torch.zeros(s, dtype=torch.float64, requires_grad=True) for n, s in zip(NAMES, shapes(k))}
    mc, vc, md, vd, fstats = split_stats(stats)
    ma, va, mb, vb = ifo.split_stats(fstats)
    rc, rd, ra, rb = (1.0 / torch.sqrt(v + EPS) for v in (vc, vd, va, vb))
    F = ifo.NAMES
    u1 = iho.resize_legacy(x54, 2)
    alive24 = torch.as_tensor((np.asarray(sub24_32) > 0).astype(np.float64))
    lin24 = (ifo.conv_dilated(u1, V[BLOCK[0]]) * (W[BLOCK[1]] * rc)
             + V[BLOCK[1]] * rc * (ifo.conv_dilated(u1, W[BLOCK[0]]) + mc.abs()) + V[BLOCK[2]]
             + (x31 @ V[BLOCK[3]].reshape(256, 128)) * (W[BLOCK[4]] * rd)
             + V[BLOCK[4]] * rd * (x31 @ W[BLOCK[3]].reshape(256, 128) + md.abs()) + V[BLOCK[5]])
    u = iho.resize_legacy(torch.as_tensor(np.abs(np.asarray(sub24_32, dtype=np.float64))), 2)
    alive12 = torch.as_tensor((np.asarray(sub12_32) > 0).astype(np.float64))
    lin12 = (ifo.conv_dilated(iho.resize_legacy(alive24 * lin24, 2), W[F[0]]) * (W[F[1]] * ra)
             + ifo.conv_dilated(u, V[F[0]]) * (W[F[1]] * ra) + V[F[1]] * ra * (ifo.conv_dilated(u, W[F[0]]) + ma.abs())
             + V[F[2]]
             + (x3 @ V[F[3]].reshape(64, 128)) * (W[F[4]] * rb)
             + V[F[4]] * rb * (x3 @ W[F[3]].reshape(64, 128) + mb.abs()) + V[F[5]])
    s12 = torch.as_tensor(np.abs(np.asarray(sub12_32, dtype=np.float64)))
    lq = (iho.resize_legacy(alive12 * lin12, 2) @ W[F[6]].reshape(128, k)
          + iho.resize_legacy(s12, 2) @ V[F[6]].reshape(128, k) + V[F[7]])
    (iho.resize_legacy(lq, 4) * a).sum().backward()
    return g, pack({n: V[n].grad.numpy() for n in NAMES}), loss


def workgroups(n, h32, w32, max_workgroups=0):
    tiles = n * -(-2 * h32 // ifo.TILE_H) * -(-2 * w32 // ifo.TILE_W)
    g = min(tiles, MAX_WG)
    return tiles, (min(g, max_workgroups) if max_workgroups > 0 else g)


def kappa(name, n, h32, w32, k, weight, max_workgroups=0):
    """the error-bound factor of the gradient test.  The fusion trainer's eight tensors keep section 28's
    (their bits are its bits, at h16 = 2 h32, w16 = 2 w32).  The new block's share the chain behind one value of g24 =
    dL/dsub24_sum:
      section 28's chain behind one value of g   16 (K + 8) (1 + cond) + 64 + 3 + 16 + 4 + K
      3 + 1                                      s_a = gamma / sqrt(var + eps); the product s_a g, rounded once when staged
      9 * 128                                    k_icnet_cascade_dx: one accumulator adds all its products one after the other
                                                 (quarter of co, tap, co within the quarter)
      9                                          the resize adjoint's at most 3 x 3 fmaf terms
    then, per tensor,
      32 ceil(tiles / G) + G                     the matrix-core chain over the tiles of sub24_sum and the fold
      6                                          u1: three interpolations of two roundings
      3 + 2                                      s (kernels); the two final products
      256 + 9 + 2 + 3 + 1                        gamma: the ci chain, the taps, - mean dBeta, rstd, the scale"""
    if name in ifo.NAMES:
        return ifo.kappa(name, n, 2 * h32, 2 * w32, k, weight, max_workgroups)
    tiles, groups = workgroups(n, h32, w32, max_workgroups)
    w32f = float(np.float32(weight))
    cond = 1.0 / np.log(w32f) if w32f > 1.0 else 0.0
    kg24 = 16 * (k + 8) * (1.0 + cond) + 64 + 3 + 16 + 4 + k + 3 + 1 + DX_CHAIN + 9
    chain = kg24 + 32 * -(-tiles // groups) + groups + 6
    if name in KERNELS:
        return chain + 3 + 2
    if name.endswith("beta"):
        return chain + 1
    return chain + 256 + 9 + 2 + 3 + 1


def adam_cascade(w, m, v, g, k, lr, beta1, beta2, eps, b1p, b2p, l1=0.0, l2=0.0):
    """numpy float32 ApplyAdam on the packed vector: the l1_l2 regulariser goes to the five kernels only"""
    out = [np.array(a, dtype=np.float32) for a in (w, m, v)]
    for name, (lo, hi) in offsets(k).items():
        reg = dict(l1=l1, l2=l2) if name in KERNELS else {}
        res = fto.adam_step(w[lo:hi], m[lo:hi], v[lo:hi], g[lo:hi], lr, beta1, beta2, eps, b1p, b2p, **reg)
        for o, r in zip(out, res):
            o[lo:hi] = r
    return tuple(out)


def train_float64(c54, c31, c3, packed0, stats, labels, mask, k, steps, lr, beta1, beta2, eps, weight, label_smoothing, l2):
    """``steps`` Adam steps in float64 (the regulariser on the kernels only) -> the losses before each step"""
    w = np.asarray(packed0, dtype=np.float64).copy()
    m, v = np.zeros_like(w), np.zeros_like(w)
    reg = np.zeros_like(w)
    for name in KERNELS:
        lo, hi = offsets(k)[name]
        reg[lo:hi] = 1.0
    out = []
    for t in range(1, steps + 1):
        loss, g = loss_and_grad(c54, c31, c3, w, stats, labels, mask, weight, label_smoothing)
        out.append(loss)
        g = g + reg * (2.0 * l2) * w
        alpha = lr * np.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)
        m += (g - m) * (1.0 - beta1)
        v += (g * g - v) * (1.0 - beta2)
        w -= m * alpha / (np.sqrt(v) + eps)
    return out
