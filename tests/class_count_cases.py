"""TEST INFRASTRUCTURE ONLY -- never imported by the product.

The inputs of the class-count sweep (test_gpu_class_counts.py on the MI355X, test_class_counts_cpu.py on the host) and of the
dead-channel tests (test_gpu_train_dead_channels.py, test_train_dead_channels_cpu.py): one place, so that the host checks the
very arrays the GPU tests run.

BLOCK_SEED and DEAD_BLOCK_SEED are chosen by the recipe documented in test_gpu_train_decoder.py: try 300, 301, ... and keep the
first seed whose PReLU margin (last_stage_train_oracle.prelu_margin: the smallest |PReLU input| of the float64 forward over the
largest |fp32 - float64| deviation at those inputs, float64 against float32 torch on the CPU; the GPU plays no part) exceeds 24;
the tests assert > 16, which leaves room for the fp32 deviation of another host's torch kernels.
  BLOCK_SEED = 300       a5_0 2 x 3 x 17, Bottleneck5_1 drawn once for every K: the first seed tried, margin 139.8 on the search host
  DEAD_BLOCK_SEED = 300  a5_0 1 x 12 x 36, projection channel 1 and convolution channel 2 of Bottleneck5_1 dead, the margin taken
                         over the inputs of the other channels: the first seed tried, margin 133.6 on the search host
"""
import numpy as np
import torch

import last_block_train_oracle as lbo
import last_stage_train_oracle as lso

CLASS_COUNTS = tuple(range(2, 33))
MEASURES = ("entropy", "margin", "confidence")
LOSSES = ((0.0, 0.0), (1.02, 0.1))  # (weight, label smoothing)

BLOCK_SEED = 300
BLOCK_SHAPE = (2, 3, 17)  # two images, two 16-wide tiles, the second one ragged, three rows
DEAD_BLOCK_SEED = 300
DEAD_BLOCK_SHAPE = (1, 12, 36)  # Bottleneck5_0's output for a3_8 of 1 x 3 x 9
DEAD_PROJ, DEAD_CONV = 1, 2  # the dead channel of the projection and of the convolution, in every trained block


def sweep_logits(k, n=2, h=3, w=5):
    """logits [n, h, w, k] of the score sweeps; pixel (0, 0, 0) ties over all classes (label 0, margin 0, entropy confidence 0)"""
    lg = (np.random.default_rng(1500 + k).normal(size=(n, h, w, k)) * 4).astype(np.float32)
    lg[0, 0, 0, :] = 1.25
    return lg


def annotation(rng, shape, k):
    """(labels uint8, mask fp32) of ``shape``: a quarter of the mask 0, label 255 under both mask values"""
    labels = rng.integers(0, k, shape).astype(np.uint8)
    mask = (rng.uniform(size=shape) > 0.25).astype(np.float32)
    ign = np.flatnonzero(rng.uniform(size=labels.size) < 0.05)
    labels.reshape(-1)[ign] = 255
    flat_l, flat_m = labels.reshape(-1), mask.reshape(-1)
    flat_l[0], flat_m[0] = 255, 1.0   # label 255 under mask 1 ...
    flat_l[1], flat_m[1] = 255, 0.0   # ... and under mask 0, whatever the draw gave
    return labels, mask


def loss_case(k, n=2, h=6, w=10):
    """(logits [n, h, w, k], labels, mask) of the loss op's sweep: label 255 under both mask values, one label == k under mask 1"""
    rng = np.random.default_rng(2100 + k)
    lg = (rng.normal(size=(n, h, w, k)) * 3).astype(np.float32)
    labels, mask = annotation(rng, (n, h, w), k)
    labels[-1, -1, -1], mask[-1, -1, -1] = k, 1.0  # tf.one_hot's all-off row
    return lg, labels, mask


def final_case(k, gain=0.3):
    """(features [2, 3, 17, 16], Final.kernel [3, 3, k, 16], labels, mask [2, 6, 34]) of the output-layer gradient's sweep"""
    n, h, w = BLOCK_SHAPE
    rng = np.random.default_rng(3100 + k)
    x = (rng.standard_normal((n, h, w, 16)) * 0.7).astype(np.float32)
    kern = rng.uniform(-gain, gain, (3, 3, k, 16)).astype(np.float32)
    labels, mask = annotation(rng, (n, 2 * h, 2 * w), k)
    return x, kern, labels, mask


def block_inputs(seed=BLOCK_SEED, shape=BLOCK_SHAPE):
    """(a5_0 [n, h, w, 16], Bottleneck5_1's twelve variables, its six statistics): no class count enters"""
    n, h, w = shape
    x = (np.random.default_rng(seed).standard_normal((n, h, w, 16)) * 0.7).astype(np.float32)
    params, stats = lbo.random_params(seed + 1000, 2)
    del params["Final.kernel"]  # random_params draws it first, so the class count is pinned (2) to pin the block's draws
    return x, params, stats


def block_case(k, gain=0.3):
    """the block head's sweep: block_inputs() for every K; only Final.kernel, the labels and the mask are drawn per K"""
    x, params, stats = block_inputs()
    n, h, w = BLOCK_SHAPE
    rng = np.random.default_rng(4100 + k)
    params = dict(params)
    params["Final.kernel"] = rng.uniform(-gain, gain, (3, 3, k, 16)).astype(np.float32)
    labels, mask = annotation(rng, (n, 2 * h, 2 * w), k)
    return x, labels, mask, params, stats


def block_prelu_inputs(x, params, stats, dtype=torch.float64):
    """Bottleneck5_1's three PReLU inputs for every image: [proj (.., 4), conv (.., 4), residual (.., 16)] float64 arrays"""
    np_dt = np.float64 if dtype == torch.float64 else np.float32
    t = {a: torch.as_tensor(np.asarray(params["%s.%s" % (lbo.BLOCK, a)], dtype=np_dt)) for a in lbo.BLOCK_VARS}
    t.update({a: torch.as_tensor(np.asarray(stats[a], dtype=np_dt)) for a in lbo.STATS})
    pre = []
    with torch.no_grad():
        lbo.block_forward(torch.as_tensor(np.asarray(x, dtype=np_dt)), t, pre)
    return [p.numpy().astype(np.float64) for p in pre]


def block_margin(x, params, stats, dead=False):
    """lso.prelu_margin of the block's PReLU inputs; ``dead``: without the inputs of DEAD_PROJ / DEAD_CONV, which are exactly 0"""
    p64, p32 = block_prelu_inputs(x, params, stats), block_prelu_inputs(x, params, stats, torch.float32)
    if dead:
        assert not p64[0][..., DEAD_PROJ].any() and not p64[1][..., DEAD_CONV].any(), "the dead channels are not dead"
        keep = (np.arange(4) != DEAD_PROJ, np.arange(4) != DEAD_CONV, np.ones(16, bool))
        p64 = [p[..., m] for p, m in zip(p64, keep)]
        p32 = [p[..., m] for p, m in zip(p32, keep)]
    flat = lambda ps: np.concatenate([p.reshape(-1) for p in ps])
    return lso.prelu_margin(flat(p64), flat(p32))


# ---- dead channels ---------------------------------------------------------------------------------------------------
def kill_channels(params, block):
    """gamma = beta = 0 on DEAD_PROJ of the projection and on DEAD_CONV of the convolution of ``block``: fma(acc, 0, 0) = +0
    at every pixel, whatever the moving statistics are"""
    for a, ch in (("proj_gamma", DEAD_PROJ), ("proj_beta", DEAD_PROJ), ("conv_gamma", DEAD_CONV), ("conv_beta", DEAD_CONV)):
        params["%s.%s" % (block, a)][ch] = 0.0


def dead_entries(block, shapes, upsampling):
    """{variable name: index} of the gradient entries that must be exactly 0 when ``block``'s channels are dead.  ``shapes`` is
    the oracle's shape table of the block.  A convolution kernel is [kh, kw, in, out]; the transposed convolution of an
    upsampling block is [kh, kw, out, in] (conv2d_transpose_3x3_s2: out[.., k] += in[.., c] w[kh, kw, k, c]).  The 1 x 1
    kernels are [1, 1, in, out]."""
    n_proj, n_conv = shapes["proj_gamma"][0], shapes["conv_gamma"][0]
    in_axis = 3 if upsampling else 2
    assert shapes["proj_kernel"][3] == n_proj and shapes["exp_kernel"][2] == n_conv
    assert shapes["conv_kernel"][in_axis] == n_proj and shapes["conv_kernel"][5 - in_axis] == n_conv
    reads = [slice(None)] * 4
    reads[in_axis] = DEAD_PROJ
    makes = [slice(None)] * 4
    makes[5 - in_axis] = DEAD_CONV
    e = {"proj_gamma": [(DEAD_PROJ,)], "proj_beta": [(DEAD_PROJ,)], "proj_alpha": [(DEAD_PROJ,)],
         "proj_kernel": [(slice(None), slice(None), slice(None), DEAD_PROJ)],
         "conv_kernel": [tuple(reads), tuple(makes)],
         "conv_gamma": [(DEAD_CONV,)], "conv_beta": [(DEAD_CONV,)], "conv_alpha": [(DEAD_CONV,)],
         "exp_kernel": [(slice(None), slice(None), DEAD_CONV, slice(None))]}
    return {"%s.%s" % (block, a): idx for a, idx in e.items()}


def assert_dead_entries_zero(who, grads, entries):
    """every listed entry == 0 (either sign); returns how many entries were checked"""
    count = 0
    for nm, idxs in entries.items():
        g = np.asarray(grads[nm])
        for idx in idxs:
            v = np.atleast_1d(g[idx])
            bad = ~(v == 0)
            assert not bad.any(), "%s: %s%s holds %d non-zero of %d entries (largest |g| %.3e)" % (
                who, nm, list(idx), int(bad.sum()), v.size, float(np.nanmax(np.abs(v))) if not np.isnan(v).all() else np.nan)
            count += v.size
    return count


def dead_block_case(k=19):
    """the last block alone with dead channels: (a5_0 [1, 12, 36, 16], labels, mask, params, stats)"""
    x, params, stats = block_inputs(DEAD_BLOCK_SEED, DEAD_BLOCK_SHAPE)
    n, h, w = DEAD_BLOCK_SHAPE
    rng = np.random.default_rng(5100 + k)
    params = {nm: np.array(v) for nm, v in params.items()}
    params["Final.kernel"] = rng.uniform(-0.3, 0.3, (3, 3, k, 16)).astype(np.float32)
    kill_channels(params, lbo.BLOCK)
    labels, mask = annotation(rng, (n, 2 * h, 2 * w), k)
    return x, labels, mask, params, stats


def decoder_blocks():
    """(block, its oracle's shape table, upsampling?) of the five trained blocks, the last block first"""
    import decoder_tail_train_oracle as dto
    import decoder_train_oracle as dco
    import deep_tail_train_oracle as ddo
    return ((lbo.BLOCK, lbo.SHAPES, False), (lso.STAGE, lso.SHAPES, True), (dto.TAIL, dto.SHAPES, False),
            (ddo.DEEP, ddo.SHAPES, False), (dco.LOW, dco.LOW_SHAPES, True))


DEAD_DECODER_SEED = 300  # any seed serves: the exact zeros hold whatever the other PReLU inputs do


def dead_decoder_case(k=19):
    """test_gpu_train_decoder._case at K = 19 and a3_8 of 1 x 3 x 9 with dead channels in all five trained blocks; the moving
    statistics stay random: (a3_8, argmax2, argmax1, labels, mask, params, stats)"""
    import test_gpu_train_decoder as tgd
    x, am2, am1, labels, mask, params, stats = tgd._case(DEAD_DECODER_SEED, 1, 3, 9, k)
    for blk, _, _ in decoder_blocks():
        kill_channels(params, blk)
    return x, am2, am1, labels, mask, params, stats


def dead_decoder_entries(blocks=None):
    """dead_entries of the named blocks (default: all five) in one dictionary"""
    out = {}
    for blk, shapes, up in decoder_blocks():
        if blocks is None or blk in blocks:
            out.update(dead_entries(blk, shapes, up))
    return out
