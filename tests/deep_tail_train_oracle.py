"""TEST INFRASTRUCTURE ONLY -- never imported by the product.

Torch restatement of the deep-tail training step: autograd of
    a4_0, argmax1 -> Bottleneck4_1 -> Bottleneck4_2 (two regular 64 -> 16 -> 16 -> 64 bottlenecks in inference mode,
    enet_modules.py:526-599) -> Bottleneck5_0 -> Bottleneck5_1 -> conv2d_transpose 3x3 / stride 2 / SAME -> masked softmax
    cross entropy
with UNFOLDED batch-norm and the reference's PReLU, built on decoder_tail_train_oracle (Bottleneck4_2's parameters, the 38
names), last_stage_train_oracle (Bottleneck5_0, the unpool), last_block_train_oracle (the regular bottleneck, the transposed
convolution, the tolerance recipe) and final_train_oracle (loss, one_hot, Adam).  float64 by default; ``dtype=torch.float32``
runs the reference's arithmetic.
"""
import numpy as np
import torch

import decoder_tail_train_oracle as dto
import final_train_oracle as fto
import last_block_train_oracle as lbo
import last_stage_train_oracle as lso

DEEP = "Bottleneck4_1"
DEEP_VARS = lbo.BLOCK_VARS  # a regular bottleneck's twelve trained variables
STATS = lbo.STATS
DEEP_NAMES = tuple("%s.%s" % (DEEP, a) for a in DEEP_VARS)
NAMES = dto.NAMES + DEEP_NAMES  # the tail's 38, then Bottleneck4_1's twelve
SHAPES = dto.SHAPES
REGULARISED = dto.REGULARISED + tuple("%s.%s" % (DEEP, a) for a in
                                      ("proj_kernel", "proj_alpha", "conv_kernel", "conv_alpha", "exp_kernel", "residual_alpha"))


def random_params(seed, k):
    """(params {name: fp32 array} of the 50 trained variables, stats {block: {name: fp32 array}}); Bottleneck4_1's are drawn
    with Bottleneck4_2's distributions from their own generator"""
    p, stats = dto.random_params(seed, k)
    rng = np.random.default_rng(seed + 17)
    for a in DEEP_VARS:
        shp = SHAPES[a]
        if a.endswith("kernel"):
            v = rng.standard_normal(shp) * {"proj_kernel": 0.15, "conv_kernel": 0.1, "exp_kernel": 0.25}[a]
        elif a.endswith("gamma"):
            v = rng.uniform(0.6, 1.4, shp)
        elif a.endswith("beta"):
            v = rng.uniform(-0.3, 0.3, shp)
        else:
            v = rng.uniform(0.05, 0.4, shp)
        p["%s.%s" % (DEEP, a)] = v.astype(np.float32)
    stats = dict(stats)
    stats[DEEP] = {a: (rng.uniform(0.5, 1.5, SHAPES[a]) if a.endswith("variance") else rng.uniform(-0.3, 0.3, SHAPES[a])).astype(np.float32)
                   for a in STATS}
    return p, stats


def _blocks(get, stats, np_dt):
    def block(name, variables):
        t = {a: get("%s.%s" % (name, a)) for a in variables}
        t.update({a: torch.as_tensor(np.asarray(stats[name][a], dtype=np_dt)) for a in STATS})
        return t
    return (block(lbo.BLOCK, lbo.BLOCK_VARS), block(lso.STAGE, lso.STAGE_VARS), block(dto.TAIL, dto.TAIL_VARS),
            block(DEEP, DEEP_VARS))


def _forward(x, am, t51, t50, t42, t41, pre):
    """Bottleneck5_1's output for one image; ``pre`` collects the twelve PReLU inputs"""
    a41 = lbo.block_forward(x, t41, pre)
    a42 = lbo.block_forward(a41, t42, pre)
    return lbo.block_forward(lso.stage_forward(a42, am, t50, pre), t51, pre)


def loss_and_grads(features4_0, argmax1, params, stats, labels, mask, weight, label_smoothing, logits32=None,
                   dtype=torch.float64):
    """(loss, {name: gradient as a float64 numpy array}, the twelve PReLU inputs of every image as one float64 vector) by
    autograd, one image at a time.  With ``logits32`` [N, 4h, 4w, K] the loss is evaluated at those (fp32) logits and
    differentiated through the chain."""
    k = params["Final.kernel"].shape[2]
    on, off, w32, c_w = fto.xent_constants(k, weight, label_smoothing)
    s = fto.mask_scale(mask)
    np_dt = np.float64 if dtype == torch.float64 else np.float32
    leaves = {n: torch.as_tensor(np.asarray(params[n], dtype=np_dt)).requires_grad_(True) for n in NAMES}
    t51, t50, t42, t41 = _blocks(leaves.__getitem__, stats, np_dt)
    total, pres = 0.0, []
    for n in range(features4_0.shape[0]):
        x = torch.as_tensor(np.asarray(features4_0[n:n + 1], dtype=np_dt))
        am = torch.as_tensor(np.asarray(argmax1[n:n + 1], dtype=np.int64))
        pre = []
        lg = lbo.conv2d_transpose_3x3_s2(_forward(x, am, t51, t50, t42, t41, pre), leaves["Final.kernel"])
        if logits32 is not None:
            lg = lg + (torch.as_tensor(np.asarray(logits32[n:n + 1], dtype=np_dt)) - lg).detach()
        y = fto.one_hot(labels[n:n + 1], k, on, off).to(dtype)
        mk = torch.as_tensor(np.asarray(mask[n:n + 1], dtype=np_dt))
        ln = fto.pixel_loss(lg, y, mk, w32, c_w).sum() * s
        ln.backward()
        total += float(ln.detach())
        pres += [p.detach().numpy().astype(np.float64).reshape(-1) for p in pre]
    return total, {n: leaves[n].grad.numpy().astype(np.float64) for n in NAMES}, np.concatenate(pres)


def prelu_inputs(features4_0, argmax1, params, stats, dtype=torch.float64):
    """the twelve PReLU inputs of every image as one float64 vector: the forward alone (what the seed search needs)"""
    np_dt = np.float64 if dtype == torch.float64 else np.float32
    t51, t50, t42, t41 = _blocks(lambda nm: torch.as_tensor(np.asarray(params[nm], dtype=np_dt)), stats, np_dt)
    pres = []
    for n in range(features4_0.shape[0]):
        x = torch.as_tensor(np.asarray(features4_0[n:n + 1], dtype=np_dt))
        am = torch.as_tensor(np.asarray(argmax1[n:n + 1], dtype=np.int64))
        pre = []
        _forward(x, am, t51, t50, t42, t41, pre)
        pres += [p.numpy().astype(np.float64).reshape(-1) for p in pre]
    return np.concatenate(pres)


prelu_margin = lso.prelu_margin
tolerance = lbo.tolerance
