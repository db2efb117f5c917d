"""TEST INFRASTRUCTURE ONLY -- never imported by the product.

Torch restatement of the last-block training step: autograd of
    a5_0 -> Bottleneck5_1 (inference mode, enet_modules.py:526-599) -> conv2d_transpose 3x3 / stride 2 / SAME -> masked
    softmax cross entropy (tensortools/losses.py:3-74)
with UNFOLDED batch-norm as TensorFlow computes it, y = gamma (x - mean) / sqrt(var + 1e-3) + beta, and the reference's PReLU
relu(x) - alpha relu(-x) (extra_ops.py:9-26; torch's relu has TensorFlow's derivative 0 at 0).  float64 by default; with
``dtype=torch.float32`` the same restatement runs in the reference's arithmetic.  The loss, one_hot, the transposed convolution
and Adam are those of final_train_oracle.
"""
import numpy as np
import torch
import torch.nn.functional as F

import final_train_oracle as fto

BLOCK = "Bottleneck5_1"
BLOCK_VARS = ("proj_kernel", "proj_gamma", "proj_beta", "proj_alpha", "conv_kernel", "conv_gamma", "conv_beta", "conv_alpha",
              "exp_kernel", "exp_gamma", "exp_beta", "residual_alpha")
STATS = ("proj_mean", "proj_variance", "conv_mean", "conv_variance", "exp_mean", "exp_variance")
NAMES = ("Final.kernel",) + tuple("%s.%s" % (BLOCK, a) for a in BLOCK_VARS)
SHAPES = {"proj_kernel": (1, 1, 16, 4), "proj_gamma": (4,), "proj_beta": (4,), "proj_alpha": (4,),
          "conv_kernel": (3, 3, 4, 4), "conv_gamma": (4,), "conv_beta": (4,), "conv_alpha": (4,),
          "exp_kernel": (1, 1, 4, 16), "exp_gamma": (16,), "exp_beta": (16,), "residual_alpha": (16,),
          "proj_mean": (4,), "proj_variance": (4,), "conv_mean": (4,), "conv_variance": (4,), "exp_mean": (16,),
          "exp_variance": (16,)}
# the variables the reference attaches kernel_regularizer to (enet_modules.py:366-382, 433-449, 477-484, 516-523; Final)
REGULARISED = ("Final.kernel",) + tuple("%s.%s" % (BLOCK, a) for a in
                                        ("proj_kernel", "proj_alpha", "conv_kernel", "conv_alpha", "exp_kernel", "residual_alpha"))


def random_params(seed, k, gain=0.3):
    """(params {name: fp32 array} of the 13 trained variables, stats {name: fp32 array}) with statistics away from 0 / 1"""
    rng = np.random.default_rng(seed)
    p = {"Final.kernel": rng.uniform(-gain, gain, (3, 3, k, 16)).astype(np.float32)}
    for a in BLOCK_VARS:
        shp = SHAPES[a]
        if a.endswith("kernel"):
            v = rng.standard_normal(shp) * (0.5 if a != "conv_kernel" else 0.3)
        elif a.endswith("gamma"):
            v = rng.uniform(0.6, 1.4, shp)
        elif a.endswith("beta"):
            v = rng.uniform(-0.3, 0.3, shp)
        else:
            v = rng.uniform(0.05, 0.4, shp)
        p["%s.%s" % (BLOCK, a)] = v.astype(np.float32)
    s = {a: (rng.uniform(0.5, 1.5, SHAPES[a]) if a.endswith("variance") else rng.uniform(-0.3, 0.3, SHAPES[a])).astype(np.float32)
         for a in STATS}
    return p, s


def prelu(x, alpha):
    return torch.relu(x) - alpha * torch.relu(-x)


def batch_norm(x, gamma, beta, mean, var):
    return gamma * (x - mean) / torch.sqrt(var + 1e-3) + beta


def conv2d_transpose_3x3_s2(x, w):
    if x.dtype == torch.float64:
        return fto.conv2d_transpose_3x3_s2(x, w)
    n, h, ww, _ = x.shape
    out = torch.zeros((n, 2 * h + 1, 2 * ww + 1, w.shape[2]), dtype=x.dtype)
    for kh in range(3):
        for kw in range(3):
            out[:, kh:kh + 2 * h:2, kw:kw + 2 * ww:2, :] += torch.einsum("nhwc,kc->nhwk", x, w[kh, kw])
    return out[:, :2 * h, :2 * ww]


def block_forward(x, t, pre=None):
    """Bottleneck5_1 in inference mode; x [N, h, w, 16], t = {short name: tensor}.  ``pre`` (a list) collects the three
    PReLU inputs."""
    y = torch.einsum("nhwc,cf->nhwf", x, t["proj_kernel"][0, 0])
    y = batch_norm(y, t["proj_gamma"], t["proj_beta"], t["proj_mean"], t["proj_variance"])
    if pre is not None:
        pre.append(y)
    y = prelu(y, t["proj_alpha"])
    y = F.conv2d(y.permute(0, 3, 1, 2), t["conv_kernel"].permute(3, 2, 0, 1), padding=1).permute(0, 2, 3, 1)
    y = batch_norm(y, t["conv_gamma"], t["conv_beta"], t["conv_mean"], t["conv_variance"])
    if pre is not None:
        pre.append(y)
    y = prelu(y, t["conv_alpha"])
    y = torch.einsum("nhwf,fc->nhwc", y, t["exp_kernel"][0, 0])
    y = batch_norm(y, t["exp_gamma"], t["exp_beta"], t["exp_mean"], t["exp_variance"])
    y = y + x
    if pre is not None:
        pre.append(y)
    return prelu(y, t["residual_alpha"])


def loss_and_grads(features5_0, params, stats, labels, mask, weight, label_smoothing, logits32=None, dtype=torch.float64):
    """(loss, {name: gradient as a float64 numpy array}, smallest |PReLU input|) by autograd, one image at a time (the
    loss is a sum over images times 1 / sum(mask) of the whole batch).  With ``logits32`` [N, 2h, 2w, K] the loss is
    evaluated at those (fp32) logits -- the point the GPU evaluates -- and differentiated through the chain."""
    k = params["Final.kernel"].shape[2]
    on, off, w32, c_w = fto.xent_constants(k, weight, label_smoothing)
    s = fto.mask_scale(mask)
    np_dt = np.float64 if dtype == torch.float64 else np.float32
    leaves = {n: torch.as_tensor(np.asarray(params[n], dtype=np_dt)).requires_grad_(True) for n in NAMES}
    t = {a: leaves["%s.%s" % (BLOCK, a)] for a in BLOCK_VARS}
    t.update({a: torch.as_tensor(np.asarray(stats[a], dtype=np_dt)) for a in STATS})
    total, smallest = 0.0, np.inf
    for n in range(features5_0.shape[0]):
        x = torch.as_tensor(np.asarray(features5_0[n:n + 1], dtype=np_dt))
        pre = []
        lg = conv2d_transpose_3x3_s2(block_forward(x, t, pre), leaves["Final.kernel"])
        if logits32 is not None:
            lg = lg + (torch.as_tensor(np.asarray(logits32[n:n + 1], dtype=np_dt)) - lg).detach()
        y = fto.one_hot(labels[n:n + 1], k, on, off).to(dtype)
        mk = torch.as_tensor(np.asarray(mask[n:n + 1], dtype=np_dt))
        ln = fto.pixel_loss(lg, y, mk, w32, c_w).sum() * s
        ln.backward()
        total += float(ln.detach())
        smallest = min([smallest] + [float(p.detach().abs().min()) for p in pre])
    return total, {n: leaves[n].grad.numpy().astype(np.float64) for n in NAMES}, smallest


def tolerance(g32, g64):
    """per tensor: 8 e_ref with e_ref = max |g32 - g64| (the reference arithmetic's own error), floor 2^-22 max |g64|"""
    return {n: max(8.0 * float(np.abs(g32[n] - g64[n]).max()), 2.0 ** -22 * float(np.abs(g64[n]).max())) for n in g64}
