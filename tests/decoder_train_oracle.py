"""TEST INFRASTRUCTURE ONLY -- never imported by the product.

Torch restatement of the decoder training step: autograd of
    a3_8, argmax2, argmax1 -> Bottleneck4_0 (the 128 -> 64 upsampling block in inference mode, enet_modules.py:940-1292) ->
    Bottleneck4_1 -> Bottleneck4_2 -> Bottleneck5_0 -> Bottleneck5_1 -> conv2d_transpose 3x3 / stride 2 / SAME -> masked
    softmax cross entropy
with UNFOLDED batch-norm and the reference's PReLU, built on deep_tail_train_oracle (the 50 names, the two regular blocks),
last_stage_train_oracle (the upsampling block's forward and the unpool, which take any channel count: here 128 -> 32 -> 16 ->
64 with 64-channel pooling indices), last_block_train_oracle and final_train_oracle.  float64 by default;
``dtype=torch.float32`` runs the reference's arithmetic.
"""
import numpy as np
import torch

import decoder_tail_train_oracle as dto
import deep_tail_train_oracle as dpo
import final_train_oracle as fto
import last_block_train_oracle as lbo
import last_stage_train_oracle as lso

LOW = "Bottleneck4_0"
LOW_VARS = lso.STAGE_VARS  # an upsampling bottleneck's thirteen trained variables
STATS = lbo.STATS
LOW_NAMES = tuple("%s.%s" % (LOW, a) for a in LOW_VARS)
NAMES = dpo.NAMES + LOW_NAMES  # the deep tail's 50, then Bottleneck4_0's thirteen
LOW_SHAPES = {"proj_kernel": (1, 1, 128, 32), "proj_gamma": (32,), "proj_beta": (32,), "proj_alpha": (32,),
              "conv_kernel": (3, 3, 16, 32), "conv_gamma": (16,), "conv_beta": (16,), "conv_alpha": (16,),
              "exp_kernel": (1, 1, 16, 64), "exp_gamma": (64,), "exp_beta": (64,), "res_kernel": (1, 1, 128, 64),
              "residual_alpha": (64,),
              "proj_mean": (32,), "proj_variance": (32,), "conv_mean": (16,), "conv_variance": (16,), "exp_mean": (64,),
              "exp_variance": (64,)}
# the variables the reference passes a regulariser to in BottleneckUpsample (enet_modules.py:1070-1214), next to the deep tail's
REGULARISED = dpo.REGULARISED + tuple("%s.%s" % (LOW, a) for a in
                                      ("proj_kernel", "proj_alpha", "conv_kernel", "conv_alpha", "exp_kernel", "res_kernel",
                                       "residual_alpha"))
PRELUS = 15  # three per trained block


def random_params(seed, k):
    """(params {name: fp32 array} of the 63 trained variables, stats {block: {name: fp32 array}}); Bottleneck4_0's come from
    their own generator, the kernels scaled so that every layer's output keeps the size of its input"""
    p, stats = dpo.random_params(seed, k)
    rng = np.random.default_rng(seed + 29)
    for a in LOW_VARS:
        shp = LOW_SHAPES[a]
        if a.endswith("kernel"):
            v = rng.standard_normal(shp) * {"proj_kernel": 0.1, "conv_kernel": 0.15, "exp_kernel": 0.25, "res_kernel": 0.1}[a]
        elif a.endswith("gamma"):
            v = rng.uniform(0.6, 1.4, shp)
        elif a.endswith("beta"):
            v = rng.uniform(-0.3, 0.3, shp)
        else:
            v = rng.uniform(0.05, 0.4, shp)
        p["%s.%s" % (LOW, a)] = v.astype(np.float32)
    stats = dict(stats)
    stats[LOW] = {a: (rng.uniform(0.5, 1.5, LOW_SHAPES[a]) if a.endswith("variance")
                      else rng.uniform(-0.3, 0.3, LOW_SHAPES[a])).astype(np.float32) for a in STATS}
    return p, stats


def random_argmax(rng, n, h, w, c):
    """int64 [n, h, w, c]: a position drawn uniformly inside each 2 x 2 window, per-image index (y * 2w + x) * c + channel
    (last_stage_train_oracle.random_argmax for any channel count)"""
    dy, dx = rng.integers(0, 2, (n, h, w, c)), rng.integers(0, 2, (n, h, w, c))
    i, j, ch = np.arange(h).reshape(1, h, 1, 1), np.arange(w).reshape(1, 1, w, 1), np.arange(c).reshape(1, 1, 1, c)
    return (((2 * i + dy) * (2 * w) + 2 * j + dx) * c + ch).astype(np.int64)


def _blocks(get, stats, np_dt):
    def block(name, variables):
        t = {a: get("%s.%s" % (name, a)) for a in variables}
        t.update({a: torch.as_tensor(np.asarray(stats[name][a], dtype=np_dt)) for a in STATS})
        return t
    return (block(lbo.BLOCK, lbo.BLOCK_VARS), block(lso.STAGE, lso.STAGE_VARS), block(dto.TAIL, dto.TAIL_VARS),
            block(dpo.DEEP, dpo.DEEP_VARS), block(LOW, LOW_VARS))


def _forward(x, am2, am1, t51, t50, t42, t41, t40, pre):
    """Bottleneck5_1's output for one image; ``pre`` collects the 15 PReLU inputs"""
    a40 = lso.stage_forward(x, am2, t40, pre)
    a41 = lbo.block_forward(a40, t41, pre)
    a42 = lbo.block_forward(a41, t42, pre)
    return lbo.block_forward(lso.stage_forward(a42, am1, t50, pre), t51, pre)


def loss_and_grads(features3_8, argmax2, argmax1, params, stats, labels, mask, weight, label_smoothing, logits32=None,
                   dtype=torch.float64):
    """(loss, {name: gradient as a float64 numpy array}, the 15 PReLU inputs of every image as one float64 vector) by
    autograd, one image at a time.  With ``logits32`` [N, 8h, 8w, K] the loss is evaluated at those (fp32) logits and
    differentiated through the chain."""
    k = params["Final.kernel"].shape[2]
    on, off, w32, c_w = fto.xent_constants(k, weight, label_smoothing)
    s = fto.mask_scale(mask)
    np_dt = np.float64 if dtype == torch.float64 else np.float32
    leaves = {n: torch.as_tensor(np.asarray(params[n], dtype=np_dt)).requires_grad_(True) for n in NAMES}
    blocks = _blocks(leaves.__getitem__, stats, np_dt)
    total, pres = 0.0, []
    for n in range(features3_8.shape[0]):
        x = torch.as_tensor(np.asarray(features3_8[n:n + 1], dtype=np_dt))
        am2 = torch.as_tensor(np.asarray(argmax2[n:n + 1], dtype=np.int64))
        am1 = torch.as_tensor(np.asarray(argmax1[n:n + 1], dtype=np.int64))
        pre = []
        lg = lbo.conv2d_transpose_3x3_s2(_forward(x, am2, am1, *blocks, pre), leaves["Final.kernel"])
        if logits32 is not None:
            lg = lg + (torch.as_tensor(np.asarray(logits32[n:n + 1], dtype=np_dt)) - lg).detach()
        y = fto.one_hot(labels[n:n + 1], k, on, off).to(dtype)
        mk = torch.as_tensor(np.asarray(mask[n:n + 1], dtype=np_dt))
        ln = fto.pixel_loss(lg, y, mk, w32, c_w).sum() * s
        ln.backward()
        total += float(ln.detach())
        pres += [p.detach().numpy().astype(np.float64).reshape(-1) for p in pre]
    return total, {n: leaves[n].grad.numpy().astype(np.float64) for n in NAMES}, np.concatenate(pres)


def loss_only(features3_8, argmax2, argmax1, params, stats, labels, mask, weight, label_smoothing):
    """the float64 loss of ``loss_and_grads`` from the forward alone (what central differences need)"""
    k = params["Final.kernel"].shape[2]
    on, off, w32, c_w = fto.xent_constants(k, weight, label_smoothing)
    s = fto.mask_scale(mask)
    get = lambda nm: torch.as_tensor(np.asarray(params[nm], dtype=np.float64))
    blocks = _blocks(get, stats, np.float64)
    total = 0.0
    with torch.no_grad():
        for n in range(features3_8.shape[0]):
            x = torch.as_tensor(np.asarray(features3_8[n:n + 1], dtype=np.float64))
            am2 = torch.as_tensor(np.asarray(argmax2[n:n + 1], dtype=np.int64))
            am1 = torch.as_tensor(np.asarray(argmax1[n:n + 1], dtype=np.int64))
            lg = lbo.conv2d_transpose_3x3_s2(_forward(x, am2, am1, *blocks, None), get("Final.kernel"))
            y = fto.one_hot(labels[n:n + 1], k, on, off).to(torch.float64)
            mk = torch.as_tensor(np.asarray(mask[n:n + 1], dtype=np.float64))
            total += float(fto.pixel_loss(lg, y, mk, w32, c_w).sum() * s)
    return total


def prelu_inputs(features3_8, argmax2, argmax1, params, stats, dtype=torch.float64):
    """the 15 PReLU inputs of every image as one float64 vector: the forward alone (what the seed search needs)"""
    np_dt = np.float64 if dtype == torch.float64 else np.float32
    blocks = _blocks(lambda nm: torch.as_tensor(np.asarray(params[nm], dtype=np_dt)), stats, np_dt)
    pres = []
    for n in range(features3_8.shape[0]):
        x = torch.as_tensor(np.asarray(features3_8[n:n + 1], dtype=np_dt))
        am2 = torch.as_tensor(np.asarray(argmax2[n:n + 1], dtype=np.int64))
        am1 = torch.as_tensor(np.asarray(argmax1[n:n + 1], dtype=np.int64))
        pre = []
        _forward(x, am2, am1, *blocks, pre)
        pres += [p.numpy().astype(np.float64).reshape(-1) for p in pre]
    return np.concatenate(pres)


prelu_margin = lso.prelu_margin
tolerance = lbo.tolerance
