"""TEST INFRASTRUCTURE ONLY -- never imported by the product.

Float64 restatement of the training step of ICNet's output layer, from ``sub12_sum`` to the loss:
  * ``sub12_sum_interp``: tf.image.resize_bilinear 2x, TF-1.13 legacy mapping (src = dst / 2, the +1 tap clamped to the last
    row / column), ``top = tl + (tr - tl) xl; bot = ..; out = top + (bot - top) yl``;
  * ``conv6_cls``: 1x1 convolution [128, K] plus bias;  ``conv6_interp``: the same resize, 4x;
  * the loss, its constants and TensorFlow's gradient conventions: ``final_train_oracle`` (tensortools/losses.py:3-74).
Autograd supplies the gradients.  The head is packed as the product packs it: [128 K | K] = kernel ([c][k]), then bias.
"""
import numpy as np
import torch

import final_train_oracle as fto

adam_step = fto.adam_step
TILE = 8  # pixels of lq per tile side of k_icnet_head_grad


def resize_legacy(x, f):
    """x [N, H, W, C] (torch float64) -> [N, f H, f W, C]"""
    _, h, w, _ = x.shape
    ys, xs = torch.arange(f * h), torch.arange(f * w)
    y0, x0 = ys // f, xs // f
    y1, x1 = torch.clamp(y0 + 1, max=h - 1), torch.clamp(x0 + 1, max=w - 1)
    ly = ((ys % f).double() / f)[None, :, None, None]
    lx = ((xs % f).double() / f)[None, None, :, None]
    r0, r1 = x[:, y0], x[:, y1]
    top = r0[:, :, x0] + (r0[:, :, x1] - r0[:, :, x0]) * lx
    bot = r1[:, :, x0] + (r1[:, :, x1] - r1[:, :, x0]) * lx
    return top + (bot - top) * ly


def head_logits(x, kernel, bias):
    """sub12_sum [N, h, w, 128], kernel [128, K], bias [K] (torch float64) -> (lq [N, 2h, 2w, K], logits [N, 8h, 8w, K])"""
    lq = resize_legacy(x, 2) @ kernel + bias
    return lq, resize_legacy(lq, 4)


def split(head, k):
    head = np.asarray(head)
    return head[:128 * k].reshape(128, k), head[128 * k:]


def loss_and_grad(features, head, labels, mask, weight, label_smoothing, logits32=None, p_class_gradient=True):
    """float64 (loss, dL/d(head) [129 K]) for sub12_sum [N, h, w, 128] (fp32 values), the packed head, labels / mask
    [N, 8h, 8w].  With ``logits32`` [N, 8h, 8w, K] the loss is evaluated at those (fp32) logits -- the point the GPU
    evaluates -- and differentiated through the two resizes and the convolution."""
    k = np.asarray(head).size // 129
    on, off, w32, c_w = fto.xent_constants(k, weight, label_smoothing)
    s = fto.mask_scale(mask)
    kern, bias = (torch.as_tensor(np.asarray(a, dtype=np.float64)).requires_grad_(True) for a in split(head, k))
    x = torch.as_tensor(np.asarray(features, dtype=np.float64))
    _, lg = head_logits(x, kern, bias)
    if logits32 is not None:
        lg = lg + (torch.as_tensor(np.asarray(logits32, dtype=np.float64)) - lg).detach()
    y = fto.one_hot(labels, k, on, off)
    mk = torch.as_tensor(np.asarray(mask, dtype=np.float64))
    loss = fto.pixel_loss(lg, y, mk, w32, c_w, p_class_gradient).sum() * s
    loss.backward()
    return float(loss.detach()), np.concatenate([kern.grad.numpy().reshape(-1), bias.grad.numpy()])


def grad_and_bound(features, head, labels, mask, weight, label_smoothing, logits32):
    """(g64 [129 K], C [129 K], loss64): the float64 gradient at the fp32 logits, and the same contraction over absolute
    values: the per-pixel magnitude bound A of section 15,
        A_{p,k} = s mask (w_p (softmax_k + y_k) + |ce_p w'_p| softmax_k (y_k + p_class)),  s = 1 / sum(mask),
    pulled back through the 4x and the 2x resize (whose weights are >= 0) and contracted with |sub12_sum| (kernel) or 1
    (bias) -- every term the kernel adds, in absolute value."""
    k = np.asarray(head).size // 129
    on, off, w32, c_w = fto.xent_constants(k, weight, label_smoothing)
    s = fto.mask_scale(mask)
    loss, g = loss_and_grad(features, head, labels, mask, weight, label_smoothing, logits32)
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
    a = s * mk[..., None] * (wc[..., None] * (sm + y) + (ce0 * dw)[..., None].abs() * sm * (y + p[..., None]))
    kern = torch.zeros((128, k), dtype=torch.float64, requires_grad=True)
    bias = torch.zeros((k,), dtype=torch.float64, requires_grad=True)
    _, la = head_logits(torch.as_tensor(np.abs(np.asarray(features, dtype=np.float64))), kern, bias)
    (la * a).sum().backward()
    return g, np.concatenate([kern.grad.numpy().reshape(-1), bias.grad.numpy()]), loss


def workgroups(h8, w8, max_workgroups=0):
    tiles = -(-2 * h8 // TILE) * -(-2 * w8 // TILE)
    g = min(tiles, 1024)
    return tiles, (min(g, max_workgroups) if max_workgroups > 0 else g)


def kappa(n, h8, w8, k, weight, max_workgroups=0):
    """the error-bound factor of the gradient test, in roundings of a term's own magnitude along the
    longest fp32 chain behind one gradient entry:
      36 n ceil(tiles / G)   the contraction: 36 window pixels of sub12_sum per tile and image, one accumulator per workgroup
      G + 2                  the fold over the workgroups, the final scale
      64 + 3                 the gather through the 4x resize: at most 8 x 8 loss pixels per window pixel and band, the
                             bands' partial sums (a window row is read by at most three of them... two, bounded by 3)
      16                     the gather through the 2x resize: at most 4 x 4 pixels of lq per pixel of sub12_sum
      16 (K + 8) (1 + cond)  section 15's per-pixel error of dL/dlogit relative to A, cond = 1 / log(weight) when weight > 1"""
    tiles, groups = workgroups(h8, w8, max_workgroups)
    w32 = float(np.float32(weight))
    cond = 1.0 / np.log(w32) if w32 > 1.0 else 0.0
    return 36 * n * -(-tiles // groups) + groups + 2 + 64 + 3 + 16 + 16 * (k + 8) * (1.0 + cond)


def adam_head(head, m, v, g, k, lr, beta1, beta2, eps, b1p, b2p, l1=0.0, l2=0.0):
    """numpy float32 ApplyAdam on the packed head: the l1_l2 regulariser goes to the kernel [128 K], not to the bias [K]"""
    s = 128 * k
    wk, mk, vk = fto.adam_step(head[:s], m[:s], v[:s], g[:s], lr, beta1, beta2, eps, b1p, b2p, l1=l1, l2=l2)
    wb, mb, vb = fto.adam_step(head[s:], m[s:], v[s:], g[s:], lr, beta1, beta2, eps, b1p, b2p)
    return np.concatenate([wk, wb]), np.concatenate([mk, mb]), np.concatenate([vk, vb])


def train_float64(features, head0, labels, mask, k, steps, lr, beta1, beta2, eps, weight, label_smoothing, l2):
    """``steps`` Adam steps in float64 (the regulariser on the kernel only) -> the losses before each step"""
    head = np.asarray(head0, dtype=np.float64).copy()
    m, v = np.zeros_like(head), np.zeros_like(head)
    reg = np.concatenate([np.ones(128 * k), np.zeros(k)])
    out = []
    for t in range(1, steps + 1):
        loss, g = loss_and_grad(features, head, labels, mask, weight, label_smoothing)
        out.append(loss)
        g = g + reg * (2.0 * l2) * head
        alpha = lr * np.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)
        m += (g - m) * (1.0 - beta1)
        v += (g * g - v) * (1.0 - beta2)
        head -= m * alpha / (np.sqrt(v) + eps)
    return out
