"""TEST INFRASTRUCTURE ONLY -- never imported by the product.

Float64 restatement of the output-layer training step:
  * ``tensortools/losses.py:3-74`` (masked_softmax_cross_entropy) with the constants of the forward op k_masked_xent:
    fp32 on / off values, fp32 weight and e - 1; a label >= K gives the all-off row (tf.one_hot);
  * TensorFlow's gradient: softmax_cross_entropy_with_logits backpropagates softmax - y (whatever sum(y) is), and the class
    weight 1 / log(weight + (e - 1 - weight) p_class) is differentiated through p_class (no stop_gradient in the
    reference);
  * conv2d_transpose 3x3 / stride 2 / SAME (enet_modules.py:1376-1380): out[2i + kh, 2j + kw] += in[i, j] W[kh, kw];
  * the Keras l1_l2 regulariser gradient and TF-1.13 ApplyAdam restated in numpy float32.
"""
import numpy as np
import torch

E_MINUS_1 = np.float32(1.718281828459045)


def xent_constants(k, weight, label_smoothing):
    """(on, off, weight, c_w) as float64 values of the fp32 numbers the kernels use"""
    ls = np.float32(label_smoothing)
    on = np.float32(np.float32(1.0) - ls)
    off = np.float32(ls / np.float32(np.float32(k) - np.float32(1.0)))
    w32 = np.float32(weight)
    return float(on), float(off), float(w32), float(np.float32(E_MINUS_1 - w32))


def one_hot(labels, k, on, off):
    lab = torch.as_tensor(np.asarray(labels).astype(np.int64))
    y = torch.full(tuple(lab.shape) + (k,), off, dtype=torch.float64)
    ok = lab < k
    y[ok] = y[ok].scatter(-1, lab[ok][:, None], on)
    return y


def conv2d_transpose_3x3_s2(x, w):
    """x [N, h, w, C], w [3, 3, K, C] (float64 torch) -> [N, 2h, 2w, K]"""
    n, h, ww, _ = x.shape
    k = w.shape[2]
    out = torch.zeros((n, 2 * h + 1, 2 * ww + 1, k), dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            out[:, kh:kh + 2 * h:2, kw:kw + 2 * ww:2, :] += torch.einsum("nhwc,kc->nhwk", x, w[kh, kw])
    return out[:, :2 * h, :2 * ww]


def contract(g, x):
    """the transposed convolution's kernel gradient: g [N, 2h, 2w, K] (d / d logits), x [N, h, w, C] -> [3, 3, K, C]"""
    n, h, ww, c = x.shape
    k = g.shape[-1]
    gp = torch.zeros((n, 2 * h + 1, 2 * ww + 1, k), dtype=torch.float64)
    gp[:, :2 * h, :2 * ww] = g
    out = torch.zeros((3, 3, k, c), dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            out[kh, kw] = torch.einsum("nhwk,nhwc->kc", gp[:, kh:kh + 2 * h:2, kw:kw + 2 * ww:2], x)
    return out


def pixel_loss(logits, y, mask, weight, c_w, p_class_gradient=True):
    """per-pixel masked (and weighted) cross entropy [N, H, W] with TensorFlow's gradient"""
    lse = torch.logsumexp(logits, -1)
    ysum = y.sum(-1)
    # value sum_k y_k (lse - x_k); gradient softmax - y (TF's SoftmaxCrossEntropyWithLogits backprop)
    ce0 = lse - (y * logits).sum(-1) + (ysum - 1.0) * lse.detach()
    ce = ce0 * mask
    if weight > 1.0:
        p = (torch.softmax(logits, -1) * y).sum(-1)
        if not p_class_gradient:
            p = p.detach()
        ce = ce * (1.0 / torch.log(weight + c_w * p))
    return ce


def mask_scale(mask):
    """1 / (double)(float)sum(mask), the loss' denominator"""
    return 1.0 / float(np.float32(np.asarray(mask, dtype=np.float64).sum()))


def loss_and_grad(features, kernel, labels, mask, weight, label_smoothing, logits32=None, p_class_gradient=True):
    """float64 (loss, dL/dW [3, 3, K, 16]) for features [N, h, w, 16] (fp32 values), kernel [3, 3, K, 16], labels / mask
    [N, 2h, 2w].  With ``logits32`` [N, 2h, 2w, K] the loss is evaluated at those (fp32) logits -- the point the GPU
    evaluates (its logits are bit-identical to the forward's) -- and differentiated through the transposed convolution."""
    k = kernel.shape[2]
    on, off, w32, c_w = xent_constants(k, weight, label_smoothing)
    s = mask_scale(mask)
    x = torch.as_tensor(np.asarray(features, dtype=np.float64))
    wt = torch.as_tensor(np.asarray(kernel, dtype=np.float64)).requires_grad_(True)
    lg = conv2d_transpose_3x3_s2(x, wt)
    if logits32 is not None:
        lg = lg + (torch.as_tensor(np.asarray(logits32, dtype=np.float64)) - lg).detach()
    y = one_hot(labels, k, on, off)
    mk = torch.as_tensor(np.asarray(mask, dtype=np.float64))
    loss = pixel_loss(lg, y, mk, w32, c_w, p_class_gradient).sum() * s
    loss.backward()
    return float(loss.detach()), wt.grad.numpy()


def grad_and_bound(features, kernel, labels, mask, weight, label_smoothing, logits32):
    """(g64 [3, 3, K, 16], C [3, 3, K, 16], loss64): the float64 gradient at the fp32 logits and the contraction over
    |features| of the per-pixel magnitude bound
        A_{p,k} = s mask (w_p (softmax_k + y_k) + |ce_p w'_p| softmax_k (y_k + p_class)),  s = 1 / sum(mask),
    one image at a time (the gradient is a sum over images)."""
    k = kernel.shape[2]
    on, off, w32, c_w = xent_constants(k, weight, label_smoothing)
    s = mask_scale(mask)
    wt = torch.as_tensor(np.asarray(kernel, dtype=np.float64))
    g = np.zeros(kernel.shape, np.float64)
    c = np.zeros(kernel.shape, np.float64)
    loss = 0.0
    for n in range(features.shape[0]):
        x = torch.as_tensor(np.asarray(features[n:n + 1], dtype=np.float64))
        lg = torch.as_tensor(np.asarray(logits32[n:n + 1], dtype=np.float64)).requires_grad_(True)
        y = one_hot(labels[n:n + 1], k, on, off)
        mk = torch.as_tensor(np.asarray(mask[n:n + 1], dtype=np.float64))
        ln = pixel_loss(lg, y, mk, w32, c_w).sum() * s
        ln.backward()
        loss += float(ln.detach())
        g += contract(lg.grad, x).numpy()
        with torch.no_grad():
            sm = torch.softmax(lg, -1)
            p = (sm * y).sum(-1)
            ce0 = (y * (torch.logsumexp(lg, -1)[..., None] - lg)).sum(-1)
            if w32 > 1.0:
                u = w32 + c_w * p
                wc = 1.0 / torch.log(u)
                dw = wc * wc * abs(c_w) / u
            else:
                wc = torch.ones_like(p)
                dw = torch.zeros_like(p)
            a = s * mk[..., None] * (wc[..., None] * (sm + y) + (ce0 * dw)[..., None].abs() * sm * (y + p[..., None]))
            c += contract(a, x.abs()).numpy()
    return g, c, loss


def kappa(n, h, w, k, weight, max_workgroups=1024, tile=16):
    """the error-bound factor of the gradient test: the longest fp32 chain per accumulator of
    dW (n images x 256 pixels x tiles per workgroup), the fold over the workgroups, the final scale, and the per-pixel
    error of dL/dlogit relative to A: 16 (K + 8) roundings-equivalents, amplified by the condition number 1 / log(weight)
    of the class weight's logarithm when weight > 1"""
    tiles = -(-h // tile) * -(-w // tile)
    groups = min(tiles, max_workgroups)
    chain = n * tile * tile * -(-tiles // groups)
    w32 = float(np.float32(weight))
    cond = 1.0 / np.log(w32) if w32 > 1.0 else 0.0
    return chain + groups + 2 + 16 * (k + 8) * (1.0 + cond)


def adam_step(w, m, v, g, lr, beta1, beta2, eps, beta1_power, beta2_power, l1=0.0, l2=0.0):
    """numpy float32 restatement of the regulariser gradient + TF-1.13 ApplyAdam -> (w, m, v)"""
    f = np.float32
    w, m, v, g = (np.asarray(a, dtype=f) for a in (w, m, v, g))
    alpha = f(f(lr) * np.sqrt(f(1.0) - f(beta2_power))) / (f(1.0) - f(beta1_power))
    g = g + (f(l2) * (f(2.0) * w) + f(l1) * np.sign(w).astype(f))
    m = m + (g - m) * (f(1.0) - f(beta1))
    v = v + (g * g - v) * (f(1.0) - f(beta2))
    w = w - (m * alpha) / (np.sqrt(v) + f(eps))
    return w.astype(f), m.astype(f), v.astype(f)
