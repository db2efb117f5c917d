"""TEST INFRASTRUCTURE ONLY -- never imported by the product.

Float64 restatement of the training step of ICNet's high-resolution branch down to the image, from
``conv5_4_k1``, ``conv3_1`` and the frame to the loss:
  * ``a_l = relu(BN(conv(a_{l-1}, K_l)))`` for ``conv1_sub1``, ``conv2_sub1``, ``conv3_sub1``: 3 x 3, stride 2, TF ``SAME`` on
    even sizes (no pad before, one zero row / column after), inference batch-norm, ``a_0`` the frame;
  * the cascade head on ``conv3_sub1 = a_3``: ``icnet_cascade_train_oracle`` and what it stands on.
Autograd supplies the gradients (``relu'(0) = 0``).  The 23 variables are packed as the product packs them: the branch's nine,
then ``icnet_cascade_train_oracle``'s fourteen.  The frozen statistics are packed unpadded: mean / variance of the three layers
at their own widths (32, 32, 32, 32, 64, 64), then the cascade oracle's [8 * 128].
"""
import numpy as np
import torch
import torch.nn.functional as F

import final_train_oracle as fto
import icnet_cascade_train_oracle as ico
import icnet_fusion_train_oracle as ifo
import icnet_head_train_oracle as iho

LAYERS = ("conv1_sub1", "conv2_sub1", "conv3_sub1")
BRANCH = tuple("%s.%s" % (l, a) for l in LAYERS for a in ("kernel", "gamma", "beta"))
NAMES = BRANCH + ico.NAMES
KERNELS = (BRANCH[0], BRANCH[3], BRANCH[6]) + ico.KERNELS  # what the l1_l2 regulariser reaches
STATS_OWN = 4 * 32 + 2 * 64
EPS = ico.EPS
# the chain-length constants of the bound (the kernels of ssal_train_icnet_highres.hip)
MAX_WG = 64          # split-K groups of the weight-gradient launches
DPROJ_CHAIN = 128    # k_icnet_highres_dproj: one accumulator adds its 128 products one after the other
DX_TAPS = 4          # k_icnet_highres_dx: at most four taps of CO products each on one accumulator
WG_TILE = (4, 16)    # k_icnet_highres_wgrad: 64 pixels of gz per tile, one after the other on one accumulator
W1_CHUNK, W1_GROUPS = 256, 8  # k_icnet_highres_wgrad1: 256-pixel chunks, 32 pixels per group and chunk, eight groups folded


def branch_shapes(c_in):
    return ((3, 3, c_in, 32), (32,), (32,), (3, 3, 32, 32), (32,), (32,), (3, 3, 32, 64), (64,), (64,))


def branch_floats(c_in):
    return 288 * c_in + 27904


def shapes(k, c_in=3):
    return branch_shapes(c_in) + ico.shapes(k)


def offsets(k, c_in=3):
    out, lo = {}, 0
    for name, shp in zip(NAMES, shapes(k, c_in)):
        out[name] = (lo, lo + int(np.prod(shp)))
        lo = out[name][1]
    return out


def floats(k, c_in=3):
    return branch_floats(c_in) + ico.floats(k)


def unpack(packed, k, c_in=3):
    packed = np.asarray(packed)
    off = offsets(k, c_in)
    return {n: packed[off[n][0]:off[n][1]].reshape(s) for n, s in zip(NAMES, shapes(k, c_in))}


def pack(d):
    return np.concatenate([np.asarray(d[n]).reshape(-1) for n in NAMES])


def split_stats(stats):
    """[256 + 8 * 128] -> [(mean_l, var_l)] of the three layers (float64 torch) and the cascade oracle's [8 * 128] (numpy)"""
    stats = np.asarray(stats, dtype=np.float64)
    cut = (0, 32, 64, 96, 128, 192, 256)
    rows = [torch.as_tensor(stats[a:b]) for a, b in zip(cut[:-1], cut[1:])]
    return [(rows[0], rows[1]), (rows[2], rows[3]), (rows[4], rows[5])], stats[STATS_OWN:]


def conv_s2(x, kern, pad_before=False):
    """3 x 3 stride-2 convolution of NHWC ``x`` with HWIO ``kern`` under TF ``SAME`` on even sizes: one zero row / column AFTER
    the map (``pad_before``: the wrong rule, one before)"""
    xp = F.pad(x.permute(0, 3, 1, 2), (1, 0, 1, 0) if pad_before else (0, 1, 0, 1))
    return F.conv2d(xp, kern.permute(3, 2, 0, 1), stride=2).permute(0, 2, 3, 1)


def _drop_last(a):
    out = a.clone()
    out[:, -1] = 0.0
    out[:, :, -1] = 0.0
    return out


def _branch(x, W, bn, at32=(None, None, None), variant=None, wmask=None):
    """a_1, a_2, a_3 (float64 torch); ``at32``: the fp32 activations the ReLUs are pinned to.  ``variant``: one of the
    deliberately wrong backward passes of the discrimination test (the forward values stay right but for "pad").
    ``wmask``: {layer index 0..2: [N, Ho, Wo, 1]}, a weight per pixel on gz_l inside the contraction of that layer's kernel,
    gamma and beta gradients only (0: left out of the split-K sum, 2: counted twice); the data gradient keeps every pixel"""
    acts, a = [], x
    for l, (layer, (mean, var)) in enumerate(zip(LAYERS, bn)):
        kern, gamma, beta = (W["%s.%s" % (layer, s)] for s in ("kernel", "gamma", "beta"))
        z = conv_s2(a, kern, pad_before=variant == "pad")
        if variant == "dk_edge":   # dK misses the last row and column of its input where they are NOT padding
            z = conv_s2(_drop_last(a.detach()), kern) + conv_s2(a, kern.detach()) - conv_s2(_drop_last(a.detach()), kern.detach())
        s = gamma / torch.sqrt(var + EPS)
        pre = z * s + (beta - mean * s)
        if variant == "no_scale" and l > 0:  # the data gradient without s_l
            zk = conv_s2(a.detach(), kern)
            za = conv_s2(a, kern.detach())
            pre = zk * s + (beta - mean * s) + (za - za.detach())
        if wmask is not None and l in wmask:
            pw = conv_s2(a.detach(), kern) * s + (beta - mean * s)
            sd = s.detach()
            pre = (conv_s2(a, kern.detach()) * sd + (beta.detach() - mean * sd)
                   + torch.as_tensor(np.asarray(wmask[l], dtype=np.float64)) * (pw - pw.detach()))
        act = ico._pinned_relu(pre, at32[l])
        if variant == "no_mask2" and l == 1:  # a_2's ReLU mask omitted from da_2
            act = pre + (act - pre).detach()
        acts.append(act)
        a = act
    return acts


def _tensors(c54, c31, x, packed, k, c_in, grad=True):
    W = {n: torch.as_tensor(np.asarray(v, dtype=np.float64).copy()).requires_grad_(grad)
         for n, v in unpack(packed, k, c_in).items()}
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))
    return t(c54), t(c31), t(x), W


def forward(c54, c31, x, packed, stats, k):
    """-> (a_1, a_2, F3, sub24_sum, sub12_sum, full-resolution logits) float64 numpy"""
    c_in = int(np.shape(x)[-1])
    x54, x31, xx, W = _tensors(c54, c31, x, packed, k, c_in, grad=False)
    bn, cstats = split_stats(stats)
    a1, a2, a3 = _branch(xx, W, bn)
    s24, s12, lg = ico.cascade_forward(c54, c31, a3.numpy(), pack_cascade(W), cstats)
    return a1.numpy(), a2.numpy(), a3.numpy(), s24, s12, lg


def pack_cascade(W):
    return np.concatenate([W[n].detach().numpy().reshape(-1) for n in ico.NAMES])


def _cascade_loss(x54, x31, a3, W, cstats, labels, mask, k, weight, label_smoothing, sub24_32, sub12_32, logits32):
    """``icnet_cascade_train_oracle.loss_and_grad``'s graph on torch tensors (so that it differentiates into a_3)"""
    on, off, w32, c_w = fto.xent_constants(k, weight, label_smoothing)
    s = fto.mask_scale(mask)
    mc, vc, md, vd, fstats = ico.split_stats(cstats)
    s24 = ico._pinned_relu(ico._pre24(x54, x31, W, mc, vc, md, vd), sub24_32)
    ma, va, mb, vb = ifo.split_stats(fstats)
    N = ifo.NAMES
    acc_a = ifo.conv_dilated(iho.resize_legacy(s24, 2), W[N[0]])
    acc_b = a3 @ W[N[3]].reshape(64, 128)
    sa, sb = W[N[1]] / torch.sqrt(va + EPS), W[N[4]] / torch.sqrt(vb + EPS)
    s12 = ico._pinned_relu(acc_a * sa + (W[N[2]] - ma * sa) + acc_b * sb + (W[N[5]] - mb * sb), sub12_32)
    _, lg = iho.head_logits(s12, W[N[6]].reshape(128, k), W[N[7]])
    if logits32 is not None:
        lg = lg + (torch.as_tensor(np.asarray(logits32, dtype=np.float64)) - lg).detach()
    y = fto.one_hot(labels, k, on, off)
    mk = torch.as_tensor(np.asarray(mask, dtype=np.float64))
    return fto.pixel_loss(lg, y, mk, w32, c_w, True).sum() * s


def loss_and_grad(c54, c31, x, packed, stats, labels, mask, k, weight, label_smoothing, at32=None, variant=None, wmask=None):
    """float64 (loss, packed gradient).  ``at32`` = (a_1, a_2, F3, sub24_sum, sub12_sum, logits) in fp32: every ReLU and the loss
    are evaluated at those values -- the point the GPU evaluates."""
    c_in = int(np.shape(x)[-1])
    at32 = (None,) * 6 if at32 is None else at32
    x54, x31, xx, W = _tensors(c54, c31, x, packed, k, c_in)
    bn, cstats = split_stats(stats)
    a3 = _branch(xx, W, bn, at32[:3], variant, wmask)[2]
    loss = _cascade_loss(x54, x31, a3, W, cstats, labels, mask, k, weight, label_smoothing, *at32[3:])
    loss.backward()
    return float(loss.detach()), pack({n: W[n].grad.numpy() for n in NAMES})


def grad_and_bound(c54, c31, x, packed, stats, labels, mask, k, weight, label_smoothing, at32):
    """(g64, C, loss64), packed: the float64 gradient at the fp32 activations, and section 29's contraction over absolute values
    continued below ``conv3_sub1``: the |conv3_sub1_proj| pull-back of sub12_sum's alive units onto the alive units of F3, the
    |K_3| and |K_2| pull-backs onto the alive units of a_2 and a_1, each contracted there with
      kernels   |s| sum_p |input| gabs     beta   sum_p gabs     gamma   rstd sum_p gabs (conv(|input|, |K|) + |mean|)."""
    c_in = int(np.shape(x)[-1])
    loss, g = loss_and_grad(c54, c31, x, packed, stats, labels, mask, k, weight, label_smoothing, at32)
    a1_32, a2_32, f3_32, sub24_32, sub12_32, logits32 = at32
    a = ifo.pixel_bound(logits32, labels, mask, k, weight, label_smoothing)
    x54, x31, xx, W = _tensors(np.abs(c54), np.abs(c31), np.abs(x), np.abs(np.asarray(packed)), k, c_in, grad=False)
    V = {n: torch.zeros(s, dtype=torch.float64, requires_grad=True) for n, s in zip(NAMES, shapes(k, c_in))}
    bn, cstats = split_stats(stats)
    tabs = lambda v: torch.as_tensor(np.abs(np.asarray(v, dtype=np.float64)))
    alive = lambda v: torch.as_tensor((np.asarray(v) > 0).astype(np.float64))
    # the branch: lin_l = the first-order change of a_l in absolute values
    inputs, lin = (xx, tabs(a1_32), tabs(a2_32)), None
    for l, (layer, (mean, var)) in enumerate(zip(LAYERS, bn)):
        kn, gn, bnm = ("%s.%s" % (layer, s) for s in ("kernel", "gamma", "beta"))
        r = 1.0 / torch.sqrt(var + EPS)
        cur = (conv_s2(inputs[l], V[kn]) * (W[gn] * r) + V[gn] * r * (conv_s2(inputs[l], W[kn]) + mean.abs()) + V[bnm])
        if lin is not None:
            cur = cur + conv_s2(lin, W[kn]) * (W[gn] * r)
        lin = alive((a1_32, a2_32, f3_32)[l]) * cur
    x3 = tabs(f3_32)
    mc, vc, md, vd, fstats = ico.split_stats(cstats)
    ma, va, mb, vb = ifo.split_stats(fstats)
    rc, rd, ra, rb = (1.0 / torch.sqrt(v + EPS) for v in (vc, vd, va, vb))
    B, N = ico.BLOCK, ifo.NAMES
    u1 = iho.resize_legacy(x54, 2)
    lin24 = (ifo.conv_dilated(u1, V[B[0]]) * (W[B[1]] * rc)
             + V[B[1]] * rc * (ifo.conv_dilated(u1, W[B[0]]) + mc.abs()) + V[B[2]]
             + (x31 @ V[B[3]].reshape(256, 128)) * (W[B[4]] * rd)
             + V[B[4]] * rd * (x31 @ W[B[3]].reshape(256, 128) + md.abs()) + V[B[5]])
    u = iho.resize_legacy(tabs(sub24_32), 2)
    lin12 = (ifo.conv_dilated(iho.resize_legacy(alive(sub24_32) * lin24, 2), W[N[0]]) * (W[N[1]] * ra)
             + ifo.conv_dilated(u, V[N[0]]) * (W[N[1]] * ra) + V[N[1]] * ra * (ifo.conv_dilated(u, W[N[0]]) + ma.abs())
             + V[N[2]]
             + (x3 @ V[N[3]].reshape(64, 128)) * (W[N[4]] * rb)
             + (lin @ W[N[3]].reshape(64, 128)) * (W[N[4]] * rb)
             + V[N[4]] * rb * (x3 @ W[N[3]].reshape(64, 128) + mb.abs()) + V[N[5]])
    s12 = tabs(sub12_32)
    lq = (iho.resize_legacy(alive(sub12_32) * lin12, 2) @ W[N[6]].reshape(128, k)
          + iho.resize_legacy(s12, 2) @ V[N[6]].reshape(128, k) + V[N[7]])
    (iho.resize_legacy(lq, 4) * a).sum().backward()
    return g, pack({n: V[n].grad.numpy() for n in NAMES}), loss


def workgroups(tiles, max_workgroups=0):
    g = min(tiles, MAX_WG)
    return min(g, max_workgroups) if max_workgroups > 0 else g


def kappa(name, n, h32, w32, k, weight, max_workgroups=0, c_in=3):
    """the error-bound factor of the gradient test, from the kernels' sequential chains.  The cascade
    trainer's fourteen tensors keep section 29's (their bits are its bits).  Behind one value of gz_3:
      section 28's chain behind one value of g   16 (K + 8) (1 + cond) + 64 + 3 + 16 + 4 + K
      3 + 1                                      s_b = gamma / sqrt(var + eps); the product s_b g, rounded once when staged
      128                                        k_icnet_highres_dproj: one accumulator, co ascending
    behind one value of gz_2, more:  3 + 1 (s_3; s_3 gz_3 rounded once when staged) + 4 * 64 (k_icnet_highres_dx<64>: at most
    four taps of 64 products on one accumulator); behind gz_1, more: 3 + 1 + 4 * 32.  Then, per tensor of layer l,
      64 ceil(tiles / G) + G                     layers 3, 2: the matrix-core chain over 4 x 16-pixel tiles of gz_l and the fold
      32 ceil(chunks / G) + 8 + G                layer 1: 32 pixels per group and 256-pixel chunk, eight groups, the fold
      3 + 2                                      s_l (kernels); the two final products
      C_in + 9 + 2 + 3 + 1                       gamma: the ci chain, the taps, - mean dBeta, rstd, the scale
    The activations a_{l-1} the weight gradient reads are the fp32 values the oracle is evaluated at: no term."""
    if name in ico.NAMES:
        return ico.kappa(name, n, h32, w32, k, weight, max_workgroups)
    w32f = float(np.float32(weight))
    cond = 1.0 / np.log(w32f) if w32f > 1.0 else 0.0
    kg = 16 * (k + 8) * (1.0 + cond) + 64 + 3 + 16 + 4 + k
    kgz = {3: kg + 3 + 1 + DPROJ_CHAIN}
    kgz[2] = kgz[3] + 3 + 1 + DX_TAPS * 64
    kgz[1] = kgz[2] + 3 + 1 + DX_TAPS * 32
    layer = 1 + LAYERS.index(name.split(".")[0])
    ho, wo = (32 >> layer) * h32, (32 >> layer) * w32  # the map of gz_l
    if layer == 1:
        chunks = -(-n * ho * wo // W1_CHUNK)
        groups = workgroups(chunks, max_workgroups)
        chain = kgz[1] + 32 * -(-chunks // groups) + W1_GROUPS + groups
        cin = c_in
    else:
        tiles = n * -(-ho // WG_TILE[0]) * -(-wo // WG_TILE[1])
        groups = workgroups(tiles, max_workgroups)
        chain = kgz[layer] + 64 * -(-tiles // groups) + groups
        cin = 32
    if name.endswith("kernel"):
        return chain + 3 + 2
    if name.endswith("beta"):
        return chain + 1
    return chain + cin + 9 + 2 + 3 + 1


STAT_WIDTHS = (32, 32, 32, 32, 64, 64) + (128,) * 8


def case(seed, n, h, w, k, c_in=3, coherent=False):
    """the inputs of one gradient case, shared by the GPU test and the CPU discrimination test (the same arrays, bit for bit):
    (conv5_4_k1, conv3_1, uint8 frame, {name: weights}, stats, labels, mask).
    Default: everything of random sign (20 % of the branch's gammas negative, projection gammas in +-1.5), ignored pixels, a
    label >= K.  The absolute-value contraction C_j then lies 10^3 .. 10^4 above |g_j| for the branch's tensors: such a case
    checks the arithmetic at every sign pattern, but the bound it checks against is loose.
    ``coherent``: the signs along the new backward path agree, so that C_j stays within a small factor of |g_j| and the bound
    bites: non-negative frame (it always is), non-negative branch kernels and conv3_sub1_proj kernel, positive gammas there,
    one label (class 0) everywhere, a head whose class-0 column is positive and dominates the others, logits near the (zero)
    bias so that no softmax saturates.  Then dL/dsub12_sum has one sign at every pixel and channel and nothing below it
    cancels."""
    rng = np.random.default_rng(seed)
    c54 = (rng.standard_normal((n, h, w, 256)) * 0.7).astype(np.float32)
    c31 = (rng.standard_normal((n, 2 * h, 2 * w, 256)) * 0.7).astype(np.float32)
    u8 = rng.integers(0, 256, (n, 32 * h, 32 * w, c_in)).astype(np.uint8)
    lim = {"conv1_sub1.kernel": 0.4, "conv2_sub1.kernel": 0.12, "conv3_sub1.kernel": 0.12, "conv_sub4.kernel": 0.03,
           "conv3_1_sub2_proj.kernel": 0.08, "conv_sub2.kernel": 0.04, "conv3_sub1_proj.kernel": 0.15, "conv6_cls.kernel": 0.3}
    d = {}
    for name, shp in zip(NAMES, shapes(k, c_in)):
        if name.endswith("kernel"):
            d[name] = rng.uniform(-lim[name], lim[name], shp)
        elif name.endswith("gamma"):
            d[name] = rng.uniform(0.5, 1.5, shp)
            if name in BRANCH:
                d[name] *= rng.choice([-1.0, 1.0], shp, p=[0.2, 0.8])
            elif "proj" in name:
                d[name] = rng.uniform(-1.5, 1.5, shp)
        else:
            d[name] = rng.uniform(-0.3, 0.3, shp)
    stats = np.concatenate([rng.uniform(0.5, 2.0, wd) if i % 2 else rng.uniform(-0.3, 0.3, wd)
                            for i, wd in enumerate(STAT_WIDTHS)]).astype(np.float32)
    labels = rng.integers(0, k, (n, 32 * h, 32 * w)).astype(np.uint8)
    mask = (rng.uniform(size=labels.shape) > 0.25).astype(np.float32)
    if coherent:
        # a frame with structure at the scale of F3's pixels, so that every layer's ReLU mask varies over the map
        coarse = rng.integers(0, 256, (n, 4 * h, 4 * w, c_in))
        u8 = np.clip(np.repeat(np.repeat(coarse, 8, 1), 8, 2) + rng.integers(-20, 21, u8.shape), 0, 255).astype(np.uint8)
        d["conv1_sub1.kernel"] = rng.uniform(0.0, 0.3, d["conv1_sub1.kernel"].shape)
        d["conv2_sub1.kernel"] = rng.uniform(0.0, 0.03, d["conv2_sub1.kernel"].shape)
        d["conv3_sub1.kernel"] = rng.uniform(0.0, 0.03, d["conv3_sub1.kernel"].shape)
        d["conv3_sub1_proj.kernel"] = rng.uniform(0.0, 0.05, d["conv3_sub1_proj.kernel"].shape)
        for layer in LAYERS + ("conv3_sub1_proj",):
            d[layer + ".gamma"] = np.abs(d[layer + ".gamma"]) + 0.5
        # every branch layer's beta puts the 30 % quantile of its pre-activation at 0: about 30 % of each channel is dead
        act = torch.as_tensor(unit(u8).astype(np.float64))
        cut = (0, 32, 64, 96, 128, 192, 256)
        for l, layer in enumerate(LAYERS):
            mean, var = stats[cut[2 * l]:cut[2 * l + 1]].astype(np.float64), stats[cut[2 * l + 1]:cut[2 * l + 2]].astype(np.float64)
            z = conv_s2(act, torch.as_tensor(d[layer + ".kernel"].astype(np.float32).astype(np.float64)))
            sc = d[layer + ".gamma"].astype(np.float32).astype(np.float64) / np.sqrt(var + EPS)
            q = np.quantile(z.numpy().reshape(-1, z.shape[-1]), 0.3, axis=0)
            d[layer + ".beta"] = (mean * sc - sc * q).astype(np.float32)
            act = torch.relu(z * torch.as_tensor(sc) + torch.as_tensor(d[layer + ".beta"].astype(np.float64) - mean * sc))
        d["conv3_sub1_proj.beta"] = rng.uniform(0.5, 1.0, 128)   # sub12_sum mostly alive
        # a head whose class-0 column is positive and dominates; scaled so that the logits stay within +-1 of the zero bias
        head = rng.uniform(-0.05, 0.05, (1, 1, 128, k))
        head[..., 0] = rng.uniform(0.5, 1.0, (1, 1, 128))
        d["conv6_cls.kernel"], d["conv6_cls.bias"] = head, np.zeros(k)
        d = {name: np.asarray(v).astype(np.float32) for name, v in d.items()}
        top = np.abs(forward(c54, c31, unit(u8), pack(d), stats, k)[5]).max()
        d["conv6_cls.kernel"] = (d["conv6_cls.kernel"] / np.float32(max(top, 1e-6))).astype(np.float32)
        labels[...] = 0
    else:
        labels[(rng.uniform(size=labels.shape) < 0.3) & (mask == 0)] = 255  # ignored pixels: label 255 under mask 0
        labels[0, 0, 0], mask[0, 0, 0] = k, 1.0                             # a label >= K under mask 1: the all-off row
        labels[-1, -1, -1], mask[-1, -1, -1] = 0, 1.0
    d = {name: np.asarray(v).astype(np.float32) for name, v in d.items()}
    return c54, c31, u8, d, stats, labels, mask


def unit(u8):
    """the frame as launch_conv_first reads a uint8 one"""
    return u8.astype(np.float32) * np.float32(1.0 / 255.0)


def adam_highres(w, m, v, g, k, lr, beta1, beta2, eps, b1p, b2p, l1=0.0, l2=0.0, c_in=3):
    """numpy float32 ApplyAdam on the packed vector: the l1_l2 regulariser goes to the eight kernels only"""
    out = [np.array(a, dtype=np.float32) for a in (w, m, v)]
    for name, (lo, hi) in offsets(k, c_in).items():
        reg = dict(l1=l1, l2=l2) if name in KERNELS else {}
        res = fto.adam_step(w[lo:hi], m[lo:hi], v[lo:hi], g[lo:hi], lr, beta1, beta2, eps, b1p, b2p, **reg)
        for o, r in zip(out, res):
            o[lo:hi] = r
    return tuple(out)
