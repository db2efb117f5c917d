"""TEST INFRASTRUCTURE ONLY -- never imported by the product.

Float64 restatement of the training step of ICNet's last fusion stage, from ``sub24_sum`` and
``conv3_sub1`` to the loss:
  * ``u = resize_2x(sub24_sum)``: the legacy mapping of ``icnet_head_train_oracle.resize_legacy``;
  * ``conv_sub2``: 3 x 3, dilation 2, TF ``SAME`` (two zero rows / columns on every side), no bias; ``conv3_sub1_proj``: 1 x 1;
  * inference batch-norm: ``s = gamma / sqrt(var + 1e-3)``, ``a s + (beta - mean s)``; ``sub12_sum = relu(a + b)``;
  * the head, the 4x resize and the loss: ``icnet_head_train_oracle`` / ``final_train_oracle``.
Autograd supplies the gradients (``relu'(0) = 0``).  The eight variables are packed as the product packs them.
"""
import numpy as np
import torch
import torch.nn.functional as F

import final_train_oracle as fto
import icnet_head_train_oracle as iho

NAMES = ("conv_sub2.kernel", "conv_sub2.gamma", "conv_sub2.beta", "conv3_sub1_proj.kernel", "conv3_sub1_proj.gamma",
         "conv3_sub1_proj.beta", "conv6_cls.kernel", "conv6_cls.bias")
KERNELS = (NAMES[0], NAMES[3], NAMES[6])  # what the l1_l2 regulariser reaches
TILE_H, TILE_W, MAX_WG = 4, 8, 96         # k_icnet_fusion_wgrad: pixels of sub12_sum per tile, split-K groups
EPS = 1e-3


def shapes(k):
    return ((3, 3, 128, 128), (128,), (128,), (1, 1, 64, 128), (128,), (128,), (1, 1, 128, k), (k,))


def offsets(k):
    out, lo = {}, 0
    for name, shp in zip(NAMES, shapes(k)):
        out[name] = (lo, lo + int(np.prod(shp)))
        lo = out[name][1]
    return out


def floats(k):
    return 156160 + 129 * k


def classes_of(packed):
    return (np.asarray(packed).size - 156160) // 129


def unpack(packed, k=None):
    packed = np.asarray(packed)
    k = classes_of(packed) if k is None else k
    off = offsets(k)
    return {n: packed[off[n][0]:off[n][1]].reshape(s) for n, s in zip(NAMES, shapes(k))}


def pack(d):
    return np.concatenate([np.asarray(d[n]).reshape(-1) for n in NAMES])


def split_stats(stats):
    """[4 * 128] -> mean_a, var_a, mean_b, var_b (float64 torch)"""
    return tuple(torch.as_tensor(np.asarray(stats, dtype=np.float64)[i * 128:(i + 1) * 128]) for i in range(4))


def conv_dilated(u, kern):
    """u [N, H, W, 128], kern [3, 3, 128, C] (HWIO) -> [N, H, W, C]: dilation 2, SAME"""
    return F.conv2d(u.permute(0, 3, 1, 2), kern.permute(3, 2, 0, 1), padding=2, dilation=2).permute(0, 2, 3, 1)


def fusion_forward(s24, c3, W, stats):
    """-> (sub12_sum, acc_a, acc_b) float64 torch; W: the eight tensors (torch float64)"""
    ma, va, mb, vb = split_stats(stats)
    acc_a = conv_dilated(iho.resize_legacy(s24, 2), W[NAMES[0]])
    acc_b = c3 @ W[NAMES[3]].reshape(64, 128)
    sa, sb = W[NAMES[1]] / torch.sqrt(va + EPS), W[NAMES[4]] / torch.sqrt(vb + EPS)
    a = acc_a * sa + (W[NAMES[2]] - ma * sa)
    b = acc_b * sb + (W[NAMES[5]] - mb * sb)
    return torch.relu(a + b), acc_a, acc_b


def _tensors(s24, c3, packed, grad=True):
    W = {n: torch.as_tensor(np.asarray(v, dtype=np.float64).copy()).requires_grad_(grad) for n, v in unpack(packed).items()}
    return (torch.as_tensor(np.asarray(s24, dtype=np.float64)), torch.as_tensor(np.asarray(c3, dtype=np.float64)), W)


def loss_and_grad(s24, c3, packed, stats, labels, mask, weight, label_smoothing, sub12_32=None, logits32=None, wmask=None):
    """float64 (loss, packed gradient).  With ``sub12_32`` / ``logits32`` the ReLU and the loss are evaluated at those (fp32)
    values -- the point the GPU evaluates -- and differentiated through the float64 chain.  ``wmask`` [N, 2h, 2w, 1]: a weight
    per pixel of sub12_sum on g = dL/dsub12_sum inside the contraction of the block's six parameter gradients only (0: the
    pixel is left out of the split-K sum, 2: counted twice) -- the deliberately wrong sums of the grid tests."""
    k = classes_of(packed)
    on, off, w32, c_w = fto.xent_constants(k, weight, label_smoothing)
    s = fto.mask_scale(mask)
    x24, x3, W = _tensors(s24, c3, packed)
    ma, va, mb, vb = split_stats(stats)
    acc_a = conv_dilated(iho.resize_legacy(x24, 2), W[NAMES[0]])
    acc_b = x3 @ W[NAMES[3]].reshape(64, 128)
    sa, sb = W[NAMES[1]] / torch.sqrt(va + EPS), W[NAMES[4]] / torch.sqrt(vb + EPS)
    pre = acc_a * sa + (W[NAMES[2]] - ma * sa) + acc_b * sb + (W[NAMES[5]] - mb * sb)
    if wmask is not None:  # (the block's inputs are constants here: only the parameters see pre's gradient)
        pre = pre.detach() + torch.as_tensor(np.asarray(wmask, dtype=np.float64)) * (pre - pre.detach())
    if sub12_32 is not None:
        # the value is the fp32 one wherever the unit is alive there, and the unit is dead exactly where fp32 says so
        s32 = torch.as_tensor(np.asarray(sub12_32, dtype=np.float64))
        sub12 = torch.where(s32 > 0, pre + (s32 - pre).detach(), torch.zeros_like(pre))
    else:
        sub12 = torch.relu(pre)
    _, lg = iho.head_logits(sub12, W[NAMES[6]].reshape(128, k), W[NAMES[7]])
    if logits32 is not None:
        lg = lg + (torch.as_tensor(np.asarray(logits32, dtype=np.float64)) - lg).detach()
    y = fto.one_hot(labels, k, on, off)
    mk = torch.as_tensor(np.asarray(mask, dtype=np.float64))
    loss = fto.pixel_loss(lg, y, mk, w32, c_w, True).sum() * s
    loss.backward()
    return float(loss.detach()), pack({n: W[n].grad.numpy() for n in NAMES})


def pixel_bound(logits32, labels, mask, k, weight, label_smoothing):
    """section 15's per-pixel magnitude bound A_{p,k} (icnet_head_train_oracle.grad_and_bound states it) at the fp32 logits"""
    on, off, w32, c_w = fto.xent_constants(k, weight, label_smoothing)
    s = fto.mask_scale(mask)
    lg = torch.as_tensor(np.asarray(logits32, dtype=np.float64))
    y = fto.one_hot(labels, k, on, off)
    mk = torch.as_tensor(np.asarray(mask, dtype=np.float64))
    sm = torch.softmax(lg, -1)
    p = (sm * y).sum(-1)
    ce0 = (y * (torch.logsumexp(lg, -1)[..., None] - lg)).sum(-1)
    if w32 > 1.0:
        u = w32 + c_w * p
        wc = 1.0 / torch.log(u)
        dw = wc * wc * abs(c_w) / u
    else:
        wc, dw = torch.ones_like(p), torch.zeros_like(p)
    return s * mk[..., None] * (wc[..., None] * (sm + y) + (ce0 * dw)[..., None].abs() * sm * (y + p[..., None]))


def grad_and_bound(s24, c3, packed, stats, labels, mask, weight, label_smoothing, sub12_32, logits32):
    """(g64, C, loss64), packed: the float64 gradient at the fp32 ``sub12_sum`` / logits, and the same contraction over
    absolute values -- every term the kernels add, in absolute value: A pulled back through both resizes and |conv6_cls| onto
    the alive units of sub12_sum (gabs), then
      kernels   |s| sum_p |input| gabs                       beta    sum_p gabs
      gamma     rstd sum_p gabs (conv(|input|, |K|) + |mean|)   (the kernel forms sum K dKraw - mean dBeta)
      conv6_cls section 23's: A pulled back and contracted with |sub12_sum| (kernel) or 1 (bias)."""
    k = classes_of(packed)
    loss, g = loss_and_grad(s24, c3, packed, stats, labels, mask, weight, label_smoothing, sub12_32, logits32)
    a = pixel_bound(logits32, labels, mask, k, weight, label_smoothing)
    x24, x3, W = _tensors(np.abs(s24), np.abs(c3), np.abs(np.asarray(packed)), grad=False)
    V = {n: torch.zeros(s, dtype=torch.float64, requires_grad=True) for n, s in zip(NAMES, shapes(k))}
    ma, va, mb, vb = split_stats(stats)
    ra, rb = 1.0 / torch.sqrt(va + EPS), 1.0 / torch.sqrt(vb + EPS)
    u = iho.resize_legacy(x24, 2)
    alive = torch.as_tensor((np.asarray(sub12_32) > 0).astype(np.float64))
    lin = (conv_dilated(u, V[NAMES[0]]) * (W[NAMES[1]] * ra) + V[NAMES[1]] * ra * (conv_dilated(u, W[NAMES[0]]) + ma.abs())
           + V[NAMES[2]]
           + (x3 @ V[NAMES[3]].reshape(64, 128)) * (W[NAMES[4]] * rb)
           + V[NAMES[4]] * rb * (x3 @ W[NAMES[3]].reshape(64, 128) + mb.abs()) + V[NAMES[5]])
    s12 = torch.as_tensor(np.abs(np.asarray(sub12_32, dtype=np.float64)))
    lq = (iho.resize_legacy(alive * lin, 2) @ W[NAMES[6]].reshape(128, k)
          + iho.resize_legacy(s12, 2) @ V[NAMES[6]].reshape(128, k) + V[NAMES[7]])
    (iho.resize_legacy(lq, 4) * a).sum().backward()
    return g, pack({n: V[n].grad.numpy() for n in NAMES}), loss


def workgroups(n, h16, w16, max_workgroups=0):
    tiles = n * -(-2 * h16 // TILE_H) * -(-2 * w16 // TILE_W)
    g = min(tiles, MAX_WG)
    return tiles, (min(g, max_workgroups) if max_workgroups > 0 else g)


def kappa(name, n, h16, w16, k, weight, max_workgroups=0):
    """the error-bound factor of the gradient test, in roundings of a term's own magnitude along the
    longest sequential fp32 chain behind one entry of the named gradient.
    conv6_cls: section 23's (icnet_head_train_oracle.kappa at h8 = 2 h16, w8 = 2 w16).  The others share the chain behind one
    value of g = dL/dsub12_sum:
      16 (K + 8) (1 + cond) + 64 + 3 + 16   section 23's per-pixel term and its two gathers
      4 + K                                  the gather of at most four tile windows; the K-term fmaf chain hw Wcls^T
    then, per tensor,
      32 ceil(tiles / G) + G                 the matrix-core chain (32 pixels per tile on one accumulator) and the fold
      6                                      u: three interpolations of two roundings (the dilated branch)
      3 + 2                                  s = gamma / sqrt(var + eps) (kernels); the two final products
      128 + 9 + 2 + 3 + 1                    gamma: the ci chain, the taps, - mean dBeta, rstd, the scale"""
    if name in NAMES[6:]:
        return iho.kappa(n, 2 * h16, 2 * w16, k, weight, max_workgroups)
    tiles, groups = workgroups(n, h16, w16, max_workgroups)
    w32 = float(np.float32(weight))
    cond = 1.0 / np.log(w32) if w32 > 1.0 else 0.0
    kg = 16 * (k + 8) * (1.0 + cond) + 64 + 3 + 16 + 4 + k
    chain = kg + 32 * -(-tiles // groups) + groups + 6
    if name in KERNELS:
        return chain + 3 + 2
    if name.endswith("beta"):
        return chain + 1
    return chain + 128 + 9 + 2 + 3 + 1


def adam_fusion(w, m, v, g, k, lr, beta1, beta2, eps, b1p, b2p, l1=0.0, l2=0.0):
    """numpy float32 ApplyAdam on the packed vector: the l1_l2 regulariser goes to the three kernels only"""
    out = [np.array(a, dtype=np.float32) for a in (w, m, v)]
    for name, (lo, hi) in offsets(k).items():
        reg = dict(l1=l1, l2=l2) if name in KERNELS else {}
        res = fto.adam_step(w[lo:hi], m[lo:hi], v[lo:hi], g[lo:hi], lr, beta1, beta2, eps, b1p, b2p, **reg)
        for o, r in zip(out, res):
            o[lo:hi] = r
    return tuple(out)


def train_float64(s24, c3, packed0, stats, labels, mask, k, steps, lr, beta1, beta2, eps, weight, label_smoothing, l2):
    """``steps`` Adam steps in float64 (the regulariser on the kernels only) -> the losses before each step"""
    w = np.asarray(packed0, dtype=np.float64).copy()
    m, v = np.zeros_like(w), np.zeros_like(w)
    reg = np.zeros_like(w)
    for name in KERNELS:
        lo, hi = offsets(k)[name]
        reg[lo:hi] = 1.0
    out = []
    for t in range(1, steps + 1):
        loss, g = loss_and_grad(s24, c3, w, stats, labels, mask, weight, label_smoothing)
        out.append(loss)
        g = g + reg * (2.0 * l2) * w
        alpha = lr * np.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)
        m += (g - m) * (1.0 - beta1)
        v += (g * g - v) * (1.0 - beta2)
        w -= m * alpha / (np.sqrt(v) + eps)
    return out
