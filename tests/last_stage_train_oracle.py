"""TEST INFRASTRUCTURE ONLY -- never imported by the product.

Torch restatement of the last-stage training step: autograd of
    a4_2, argmax1 -> Bottleneck5_0 (inference mode, enet_modules.py:940-1292) -> Bottleneck5_1 -> conv2d_transpose 3x3 /
    stride 2 / SAME -> masked softmax cross entropy
with UNFOLDED batch-norm and the reference's PReLU, built on last_block_train_oracle (Bottleneck5_1, the transposed
convolution, the tolerance recipe) and final_train_oracle (loss, one_hot, Adam).  The unpool is xops.unpool_2d
(extra_ops.py:28-86): a scatter of the residual convolution's output to the per-image flat positions ``argmax1`` names; its
backward is the gather at those positions.  float64 by default; ``dtype=torch.float32`` runs the reference's arithmetic.
"""
import numpy as np
import torch

import final_train_oracle as fto
import last_block_train_oracle as lbo

STAGE = "Bottleneck5_0"
STAGE_VARS = ("proj_kernel", "proj_gamma", "proj_beta", "proj_alpha", "conv_kernel", "conv_gamma", "conv_beta", "conv_alpha",
              "exp_kernel", "exp_gamma", "exp_beta", "res_kernel", "residual_alpha")
STATS = lbo.STATS
STAGE_NAMES = tuple("%s.%s" % (STAGE, a) for a in STAGE_VARS)
NAMES = lbo.NAMES + STAGE_NAMES
SHAPES = {"proj_kernel": (1, 1, 64, 16), "proj_gamma": (16,), "proj_beta": (16,), "proj_alpha": (16,),
          "conv_kernel": (3, 3, 8, 16), "conv_gamma": (8,), "conv_beta": (8,), "conv_alpha": (8,),
          "exp_kernel": (1, 1, 8, 16), "exp_gamma": (16,), "exp_beta": (16,), "res_kernel": (1, 1, 64, 16),
          "residual_alpha": (16,),
          "proj_mean": (16,), "proj_variance": (16,), "conv_mean": (8,), "conv_variance": (8,), "exp_mean": (16,),
          "exp_variance": (16,)}
# the variables the reference passes a regulariser to (enet_modules.py:1070-1214), next to the last block's
REGULARISED = lbo.REGULARISED + tuple("%s.%s" % (STAGE, a) for a in
                                      ("proj_kernel", "proj_alpha", "conv_kernel", "conv_alpha", "exp_kernel", "res_kernel",
                                       "residual_alpha"))


def random_params(seed, k):
    """(params {name: fp32 array} of the 26 trained variables, stats {block: {name: fp32 array}})"""
    p, s51 = lbo.random_params(seed, k)
    rng = np.random.default_rng(seed + 7)
    for a in STAGE_VARS:
        shp = SHAPES[a]
        if a.endswith("kernel"):
            v = rng.standard_normal(shp) * {"proj_kernel": 0.2, "conv_kernel": 0.2, "exp_kernel": 0.4, "res_kernel": 0.2}[a]
        elif a.endswith("gamma"):
            v = rng.uniform(0.6, 1.4, shp)
        elif a.endswith("beta"):
            v = rng.uniform(-0.3, 0.3, shp)
        else:
            v = rng.uniform(0.05, 0.4, shp)
        p["%s.%s" % (STAGE, a)] = v.astype(np.float32)
    s50 = {a: (rng.uniform(0.5, 1.5, SHAPES[a]) if a.endswith("variance") else rng.uniform(-0.3, 0.3, SHAPES[a])).astype(np.float32)
           for a in STATS}
    return p, {lbo.BLOCK: s51, STAGE: s50}


def random_argmax(rng, n, h, w):
    """int64 [n, h, w, 16]: a position drawn uniformly inside each 2 x 2 window, per-image index (y * 2w + x) * 16 + c"""
    dy, dx = rng.integers(0, 2, (n, h, w, 16)), rng.integers(0, 2, (n, h, w, 16))
    i, j, c = np.arange(h).reshape(1, h, 1, 1), np.arange(w).reshape(1, 1, w, 1), np.arange(16).reshape(1, 1, 1, 16)
    return (((2 * i + dy) * (2 * w) + 2 * j + dx) * 16 + c).astype(np.int64)


def unpool_2d(r, argmax):
    """r [1, h, w, C] scattered to [1, 2h, 2w, C] at the flat per-image positions of argmax [1, h, w, C]"""
    n, h, w, c = r.shape
    out = torch.zeros((n, 4 * h * w * c), dtype=r.dtype)
    return out.scatter(1, argmax.reshape(n, -1), r.reshape(n, -1)).reshape(n, 2 * h, 2 * w, c)


def stage_forward(x, argmax, t, pre=None):
    """Bottleneck5_0 in inference mode; x [1, h, w, 64], argmax int64 [1, h, w, 16], t = {short name: tensor}.  ``pre`` (a
    list) collects the three PReLU inputs."""
    y = torch.einsum("nhwc,cf->nhwf", x, t["proj_kernel"][0, 0])
    y = lbo.batch_norm(y, t["proj_gamma"], t["proj_beta"], t["proj_mean"], t["proj_variance"])
    if pre is not None:
        pre.append(y)
    y = lbo.prelu(y, t["proj_alpha"])
    y = lbo.conv2d_transpose_3x3_s2(y, t["conv_kernel"])
    y = lbo.batch_norm(y, t["conv_gamma"], t["conv_beta"], t["conv_mean"], t["conv_variance"])
    if pre is not None:
        pre.append(y)
    y = lbo.prelu(y, t["conv_alpha"])
    y = torch.einsum("nhwf,fc->nhwc", y, t["exp_kernel"][0, 0])
    y = lbo.batch_norm(y, t["exp_gamma"], t["exp_beta"], t["exp_mean"], t["exp_variance"])
    y = y + unpool_2d(torch.einsum("nhwc,cf->nhwf", x, t["res_kernel"][0, 0]), argmax)
    if pre is not None:
        pre.append(y)
    return lbo.prelu(y, t["residual_alpha"])


def loss_and_grads(features4_2, argmax1, params, stats, labels, mask, weight, label_smoothing, logits32=None,
                   dtype=torch.float64):
    """(loss, {name: gradient as a float64 numpy array}, the six PReLU inputs of every image as one float64 vector) by
    autograd, one image at a time.  With ``logits32`` [N, 4h, 4w, K] the loss is evaluated at those (fp32) logits and
    differentiated through the chain."""
    k = params["Final.kernel"].shape[2]
    on, off, w32, c_w = fto.xent_constants(k, weight, label_smoothing)
    s = fto.mask_scale(mask)
    np_dt = np.float64 if dtype == torch.float64 else np.float32
    leaves = {n: torch.as_tensor(np.asarray(params[n], dtype=np_dt)).requires_grad_(True) for n in NAMES}
    t51 = {a: leaves["%s.%s" % (lbo.BLOCK, a)] for a in lbo.BLOCK_VARS}
    t51.update({a: torch.as_tensor(np.asarray(stats[lbo.BLOCK][a], dtype=np_dt)) for a in STATS})
    t50 = {a: leaves["%s.%s" % (STAGE, a)] for a in STAGE_VARS}
    t50.update({a: torch.as_tensor(np.asarray(stats[STAGE][a], dtype=np_dt)) for a in STATS})
    total, pres = 0.0, []
    for n in range(features4_2.shape[0]):
        x = torch.as_tensor(np.asarray(features4_2[n:n + 1], dtype=np_dt))
        am = torch.as_tensor(np.asarray(argmax1[n:n + 1], dtype=np.int64))
        pre = []
        a5 = stage_forward(x, am, t50, pre)
        lg = lbo.conv2d_transpose_3x3_s2(lbo.block_forward(a5, t51, pre), leaves["Final.kernel"])
        if logits32 is not None:
            lg = lg + (torch.as_tensor(np.asarray(logits32[n:n + 1], dtype=np_dt)) - lg).detach()
        y = fto.one_hot(labels[n:n + 1], k, on, off).to(dtype)
        mk = torch.as_tensor(np.asarray(mask[n:n + 1], dtype=np_dt))
        ln = fto.pixel_loss(lg, y, mk, w32, c_w).sum() * s
        ln.backward()
        total += float(ln.detach())
        pres += [p.detach().numpy().astype(np.float64).reshape(-1) for p in pre]
    return total, {n: leaves[n].grad.numpy().astype(np.float64) for n in NAMES}, np.concatenate(pres)


def prelu_margin(pre64, pre32):
    """smallest |PReLU input| of the float64 forward over the largest |fp32 - float64| deviation at those inputs"""
    return float(np.abs(pre64).min()) / max(float(np.abs(pre32 - pre64).max()), 1e-300)


tolerance = lbo.tolerance
