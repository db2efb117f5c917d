"""The cases test_gpu_bf16x3_model.py runs on the GPU and test_split_operand_model_cpu.py proves things about without one:
weights (overrides of one layer's entries of the parameter dictionary) and inputs, built from seeds alone.

KINDS     regular (Bottleneck2_1; the dilated blocks 2_2 / 2_4 / 2_6 / 2_8 in the dense cases), asym (2_3), down (2_0), up (4_0)
dense     the seeded synthetic weights (signed), unit-normal inputs: routing at ragged shapes
live      all-positive data whose three split terms are all large, one K = 16 chunk of ONE stage holds dense positive
          weights, every other stage a positive three-term selector (one weight per output channel, one tap), batch norm folded
          to s == 1, t == 0.  The issue asked for dense weights in the other stages; under the bound's rule a dense
          18-chunk stage is allowed ~1000 u A of accumulation error, ten times what a lost 2^-16-level product moves, so
          no such case can show that a lost product breaks the bound.  A selector stage adds one non-zero product per
          instruction: its allowance is 2 u A, and every one of the six products still flows through it.
exact     selector weights 1 (one stage: 1 + 2^-8 + 2^-16), data +-(1 + 2^-8 + 2^-16) 2^e, PReLU slopes 2^-2: every partial
          sum of the six products is an fp32 number, so the mode's output is known bit for bit."""
import numpy as np

KINDS = {"regular": "Bottleneck2_1", "asym": "Bottleneck2_3", "down": "Bottleneck2_0", "up": "Bottleneck4_0"}
DILATED = {1: "Bottleneck2_1", 2: "Bottleneck2_2", 4: "Bottleneck2_4", 8: "Bottleneck2_6", 16: "Bottleneck2_8"}
STAGES = {"regular": ("projection", "convolution", "expansion"), "asym": ("projection", "convolution", "expansion"),
          "down": ("projection", "convolution", "expansion"), "up": ("projection", "convolution", "expansion", "residual")}
CHUNKS = {("regular", "projection"): 8, ("regular", "convolution"): 18, ("regular", "expansion"): 8,
          ("asym", "projection"): 8, ("asym", "convolution"): 20, ("asym", "expansion"): 8,
          ("down", "projection"): 16, ("down", "convolution"): 18, ("down", "expansion"): 8,
          ("up", "projection"): 8, ("up", "convolution"): 12, ("up", "expansion"): 2, ("up", "residual"): 16}
KERNEL = {"regular": "k_bottleneck_bf16x3", "asym": "k_bottleneck_asym_bf16x3", "down": "k_downsample_bf16x3",
          "up": "k_upsample_bf16x3"}
LIVE_SHAPE = {"regular": (1, 5, 7, 128), "asym": (1, 5, 7, 128), "down": (1, 6, 8, 64), "up": (1, 3, 4, 128)}
LIVE_CASES = [(kind, stage, chunk) for kind in KINDS for stage in STAGES[kind] for chunk in range(CHUNKS[kind, stage])]
EXACT_CASES = [(kind, stage) for kind in KINDS for stage in STAGES[kind]]
_UP_TAPS = ((0, 1), (2, -1), (6, 7), (8, -1), (3, 4), (5, -1))  # stacked transposed-conv slots: taps kh * 3 + kw of the two classes
_WIDTHS = {"regular": (128, 32, 32, 128), "asym": (128, 32, 32, 128), "down": (64, 32, 32, 128), "up": (128, 32, 16, 64)}


def rich(rng, shape, lo=-1, hi=1):
    """positive fp32 numbers in [2^lo, 2^(hi+1)) whose second and third split terms are both in the top eighth of their range"""
    top = rng.integers(0, 128, shape).astype(np.uint32)
    mid = rng.integers(0xE0, 0x100, shape).astype(np.uint32)
    low = rng.integers(0xE0, 0x100, shape).astype(np.uint32)
    e = rng.integers(127 + lo, 127 + hi + 1, shape).astype(np.uint32)
    return ((e << 23) | (top << 16) | (mid << 8) | low).view(np.float32)


def unit_variance():
    """a batch-norm variance v with 1 / sqrtf(v + 1e-3f) == 1 in fp32 (the fold the library and the oracle share)"""
    v = np.float32(1.0) - np.float32(1e-3)
    for _ in range(8):
        if np.float32(v + np.float32(1e-3)) == np.float32(1.0):
            return v
        v = np.nextafter(v, np.float32(2.0) if np.float32(v + np.float32(1e-3)) < 1 else np.float32(0.0))
    raise AssertionError("no fp32 variance folds to a unit scale")


def identity_bn(kind, alpha=0.25):
    cin, f, cf, cout = _WIDTHS[kind]
    o = {}
    for p, c in (("proj_", f), ("conv_", cf), ("exp_", cout)):
        o[p + "mean"] = np.zeros(c, np.float32)
        o[p + "beta"] = np.zeros(c, np.float32)
        o[p + "gamma"] = np.ones(c, np.float32)
        o[p + "variance"] = np.full(c, unit_variance(), np.float32)
    o["proj_alpha"] = np.full(f, alpha, np.float32)
    o["conv_alpha"] = np.full(cf, alpha, np.float32)
    o["residual_alpha"] = np.full(cout, alpha, np.float32)
    return o


def _selectors(kind, value):
    """one weight per output channel and one tap in every stage; value(n) -> n weights"""
    cin, f, cf, cout = _WIDTHS[kind]
    o = {}
    if kind == "down":
        wp = np.zeros((2, 2, 64, 32), np.float32)
        co = np.arange(32)
        wp[co % 2, (co // 2) % 2, 2 * co, co] = value(32)
    else:
        wp = np.zeros((1, 1, 128, 32), np.float32)
        wp[0, 0, 4 * np.arange(32), np.arange(32)] = value(32)
    o["proj_kernel"] = wp
    perm = (5 * np.arange(32) + 3) % 32
    if kind == "asym":
        w0, w1 = np.zeros((5, 1, 32, 32), np.float32), np.zeros((1, 5, 32, 32), np.float32)
        w0[2, 0, perm, np.arange(32)] = value(32)
        w1[0, 2, perm, np.arange(32)] = value(32)
        o["conv_kernel.0"], o["conv_kernel.1"] = w0, w1
    elif kind == "up":
        wc = np.zeros((3, 3, 16, 32), np.float32)  # HW-O-I; taps 0, 1, 3, 4 = the four parity classes' tap on P(i, j)
        for kh, kw in ((0, 0), (0, 1), (1, 0), (1, 1)):
            wc[kh, kw, np.arange(16), (2 * np.arange(16) + 1) % 32] = value(16)
        o["conv_kernel"] = wc
    else:
        wc = np.zeros((3, 3, 32, 32), np.float32)
        wc[1, 1, perm, np.arange(32)] = value(32)
        o["conv_kernel"] = wc
    we = np.zeros((1, 1, cf, cout), np.float32)
    we[0, 0, np.arange(cout) % cf, np.arange(cout)] = value(cout)
    o["exp_kernel"] = we
    if kind == "up":
        wr = np.zeros((1, 1, 128, 64), np.float32)
        wr[0, 0, 2 * np.arange(64), np.arange(64)] = value(64)
        o["res_kernel"] = wr
    return o


def _live_weights(kind, stage, chunk, rng, o):
    """replace the stage's kernel by zeros except K-chunk `chunk`, which gets dense positive weights"""
    def dense(shape):
        return rich(rng, shape, -4, -3)

    if stage == "projection":
        w = np.zeros_like(o["proj_kernel"])
        if kind == "down":  # chunk s = 4 cc + t, t = dy * 2 + dx
            cc, t = chunk >> 2, chunk & 3
            w[t >> 1, t & 1, 16 * cc:16 * cc + 16, :] = dense((16, 32))
        else:
            w[0, 0, 16 * chunk:16 * chunk + 16, :] = dense((16, 32))
        o["proj_kernel"] = w
    elif stage == "convolution":
        tap, c2 = chunk >> 1, chunk & 1
        if kind == "asym":  # taps 0..4 = the (5,1) kernel, 5..9 = the (1,5) kernel; the other kernel keeps its selector
            key = "conv_kernel.0" if tap < 5 else "conv_kernel.1"
            w = np.zeros_like(o[key])
            w.reshape(5, 32, 32)[tap % 5, 16 * c2:16 * c2 + 16, :] = dense((16, 32))
            o[key] = w
        elif kind == "up":  # chunk = 2 slot + c2 of the stacked kernel: the slot's one or two taps
            w = np.zeros_like(o["conv_kernel"])
            for tp in _UP_TAPS[tap]:
                if tp >= 0:
                    w.reshape(9, 16, 32)[tp, :, 16 * c2:16 * c2 + 16] = dense((16, 16))
            o["conv_kernel"] = w
        else:
            w = np.zeros_like(o["conv_kernel"])
            w.reshape(9, 32, 32)[tap, 16 * c2:16 * c2 + 16, :] = dense((16, 32))
            o["conv_kernel"] = w
    elif stage == "expansion":
        w = np.zeros_like(o["exp_kernel"])
        if kind == "up":  # chunk = nt (K = 16: one chunk)
            w[0, 0, :, 32 * chunk:32 * chunk + 32] = dense((16, 32))
        else:  # chunk = 2 nt + c
            nt, c = chunk >> 1, chunk & 1
            w[0, 0, 16 * c:16 * c + 16, 32 * nt:32 * nt + 32] = dense((16, 32))
        o["exp_kernel"] = w
    else:  # the upsample block's residual 1x1: chunk = 2 c + nt
        c, nt = chunk >> 1, chunk & 1
        w = np.zeros_like(o["res_kernel"])
        w[0, 0, 16 * c:16 * c + 16, 32 * nt:32 * nt + 32] = dense((16, 32))
        o["res_kernel"] = w
    return o


def pooling_indices(rng, n, h, w):
    """indices of a 2x2 / s2 max-pool of a random [n, 2h, 2w, 64] tensor, per image: (y * 2w + x) * 64 + c"""
    big = rng.normal(size=(n, 2 * h, 2 * w, 64)).astype(np.float32)
    win = big.reshape(n, h, 2, w, 2, 64).transpose(0, 1, 3, 5, 2, 4).reshape(n, h, w, 64, 4)
    code = win.argmax(-1)
    yy = 2 * np.arange(h)[None, :, None, None] + code // 2
    xx = 2 * np.arange(w)[None, None, :, None] + code % 2
    return ((yy * (2 * w) + xx) * 64 + np.arange(64)[None, None, None, :]).astype(np.int64)


def with_overrides(P, name, overrides):
    out = dict(P)
    for attr, val in overrides.items():
        assert out[name + "." + attr].shape == val.shape, (attr, val.shape)
        out[name + "." + attr] = np.ascontiguousarray(val, np.float32)
    return out


def _stage_keys(kind, stage):
    if stage == "convolution":
        return ["conv_kernel.0", "conv_kernel.1"] if kind == "asym" else ["conv_kernel"]
    return {"projection": ["proj_kernel"], "expansion": ["exp_kernel"], "residual": ["res_kernel"]}[stage]


def live_case(kind, stage, chunk, zero_stage=None):
    """-> (overrides, x, argmax or None).  zero_stage: the same case with that stage's kernels all zero (the outputs that change
    are the ones the stage reaches)"""
    seed = sum(ord(c) for c in kind + stage) * 131 + chunk
    rng = np.random.default_rng(seed)
    o = identity_bn(kind)
    o.update(_selectors(kind, lambda n: rich(rng, (n,), 0, 0)))
    x = rich(rng, LIVE_SHAPE[kind], -1, 1)
    o = _live_weights(kind, stage, chunk, rng, o)
    if zero_stage is not None:
        for key in _stage_keys(kind, zero_stage):
            o[key] = np.zeros_like(o[key])
    n, h, w, _ = LIVE_SHAPE[kind]
    return o, x, (pooling_indices(rng, n, h, w) if kind == "up" else None)


FAMILY = np.float32(1.0 + 2.0 ** -8 + 2.0 ** -16)


def exact_case(kind, stage):
    """-> (overrides, x, argmax or None): selector weights 1, FAMILY in `stage`; data +-FAMILY 2^e"""
    rng = np.random.default_rng(sum(ord(c) for c in kind + stage))
    o = identity_bn(kind)
    o.update(_selectors(kind, lambda n: np.ones(n, np.float32)))
    fam = _selectors(kind, lambda n: np.full(n, FAMILY, np.float32))
    for key in _stage_keys(kind, stage)[:1]:  # the asymmetric pair: the (5,1) kernel
        o[key] = fam[key]
    shape = LIVE_SHAPE[kind]
    e = rng.integers(-3, 4, shape).astype(np.float32)
    sign = np.where(rng.integers(0, 2, shape) > 0, np.float32(1), np.float32(-1))
    x = (sign * FAMILY * np.exp2(e)).astype(np.float32)
    n, h, w, _ = shape
    return o, x, (pooling_indices(rng, n, h, w) if kind == "up" else None)


def dense_input(kind, shape, seed=18):
    c = 64 if kind == "down" else 128
    n, h, w = shape
    return np.random.default_rng(seed + h * 131 + w).normal(size=(n, h, w, c)).astype(np.float32)


DENSE_CASES = ([("regular", d, s) for d in (1, 2, 4, 8, 16) for s in ((1, 9, 11), (2, 17, 35))]
               + [("asym", 1, s) for s in ((1, 9, 11), (2, 17, 35))]
               + [("down", 1, s) for s in ((1, 18, 22), (1, 2, 2))]
               + [("up", 1, s) for s in ((1, 9, 11), (1, 1, 1))])
SWEEP = ["2^-40", "2^-12", "2^12", "2^30", "span"]


def sweep_input(which):
    """the regular block at 1 x 9 x 11: unit-normal data scaled as a whole, or 128 channels spanning 2^-20 .. 2^20 per pixel"""
    x = dense_input("regular", (1, 9, 11), seed=77)
    if which == "span":
        return (x * np.exp2(np.round(np.linspace(-20, 20, 128))).astype(np.float32)).astype(np.float32)
    return (x * np.float32(2.0 ** int(which[2:]))).astype(np.float32)


ZERO_CASES = ["all", "channels"]


def zero_case(which):
    """the regular block at 1 x 9 x 11 on the seeded weights.  "all": every input +-0 and the first two batch norms without a
    shift, so every product of every stage is an exact zero; "channels": unit-normal data with every third input channel +-0,
    every seventh projection row and every fifth expansion column zero (outputs whose own chain is exact)"""
    rng = np.random.default_rng(len(which))
    sign = np.where(rng.integers(0, 2, (1, 9, 11, 128)) > 0, np.float32(0.0), np.float32(-0.0))
    if which == "all":
        z = np.zeros(32, np.float32)
        return {"proj_mean": z, "proj_beta": z, "conv_mean": z, "conv_beta": z}, sign

    def override(P, name):
        wp, we = P[name + ".proj_kernel"].copy(), P[name + ".exp_kernel"].copy()
        wp[:, :, ::7, :] = 0
        we[..., ::5] = 0
        return {"proj_kernel": wp, "exp_kernel": we}

    x = rng.normal(size=(1, 9, 11, 128)).astype(np.float32)
    x[..., ::3] = sign[..., ::3]
    return override, x


def run_model(model, P, kind, name, x, argmax=None, dil=1, **kw):
    """the model of the kind's block -> (value, bound)"""
    if kind == "down":
        return model.bottleneck_down(P, name, x, **kw)[:2]
    if kind == "up":
        return model.bottleneck_up(P, name, x, argmax, **kw)
    return model.bottleneck(P, name, x, dil=dil, asym=kind == "asym", **kw)
