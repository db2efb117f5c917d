"""Training of ICNet through ``conv5_2`` without a GPU: the trainer and the C ABI's symbols, the packed
layout, the refusals (judged before any device work), the workspace arithmetic and the statuses, the float64 oracle against an
independent autograd statement of the block and of the whole depth, against section 42's oracle above ``conv5_2`` and against
its own term-by-term backward pass, and the discrimination of the gradient test's bound on the sign-coherent cases: the wrong
backward passes leave it on every tensor they corrupt."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import semanticsegmentationactivelearning_amd as ssal
from semanticsegmentationactivelearning_amd import _lib, training

import icnet_bneck2_train_oracle as b2
import icnet_bneck_train_oracle as bo

AL_HYPER = {"learning_rate": 0.0005, "learning_rate_decay": 0.0,
            "optimizer": {"type": "Adam", "kwargs": {"beta1": 0.9, "beta2": 0.99}},
            "weight_reg": {"L2": 0.0002, "L1": 0.0, "glorot_scaling": False},
            "softmax": {"label_smoothing": 0.0, "loginverse_scaling": 1.02, "multiscale": False}}
ABI = ("ssal_icnet_bneck2_grad_workspace_bytes", "ssal_icnet_bneck2_grad_nhwc", "ssal_icnet_train_bneck2_workspace_bytes",
       "ssal_icnet_train_bneck2_nhwc", "ssal_icnet_update_bneck2")


def _icnet(k=19):
    net = ssal.ICNet(k)
    net.build((None, None, None, 3))
    return net


def test_trainer_and_abi_symbols_exist():
    """fails on a library / package without the feature"""
    assert issubclass(training.ICNetDeepBottleneckTrainer, training.ICNetBottleneckTrainer)
    assert not issubclass(training.ICNetDeepBottleneckTrainer, training.ICNetHighResTrainer)
    assert "ICNetDeepBottleneckTrainer" in training.__all__
    L = _lib.lib()
    i, i64, f, vp = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
    want = {ABI[0]: (i64, [i, i, i, i]),
            ABI[1]: (i, [vp, vp, vp, i, i, i, i, vp, vp, vp, f, f, vp, i, vp, vp, vp, i64, vp]),
            ABI[2]: (i64, [vp, i, i, i]),
            ABI[3]: (i, [vp, vp, i, i, i, i, vp, vp, vp, f, f, vp, i, vp, vp, vp, i64, vp]),
            ABI[4]: (i, [vp, vp, vp])}
    for name in ABI:
        assert _lib.PROTOTYPES[name] == want[name], name
        assert hasattr(L, name)


@pytest.mark.parametrize("k", [2, 19, 32])
def test_packed_offsets_names_and_float_count(k):
    net = _icnet(k)
    tr = training.ICNetDeepBottleneckTrainer(net, 1e-3)
    assert tr.variable_names == list(b2.NAMES) and len(b2.NAMES) == 35
    assert tr.variable_names[9:] == training.ICNetBottleneckTrainer.variable_names
    want = [getattr(getattr(net, n.split(".")[0]), n.split(".")[1]) for n in b2.NAMES]
    assert all(a is b for a, b in zip(tr._vars(), want))
    assert [tuple(v.shape) for v in want] == list(b2.shapes(k))
    assert tr._floats() == b2.floats(k) == 1117184 + bo.floats(k)
    off = b2.offsets(k)
    assert off[b2.BLOCK_R[0]] == (0, 262144) and off[b2.BLOCK_3[0]] == (262656, 852480)
    assert off[b2.BLOCK_I[0]] == (852992, 1115136) and off[b2.BLOCK_I[1]] == (1115136, 1116160)
    assert off[b2.BLOCK_I[2]] == (1116160, 1117184) and off[bo.BLOCK_R[0]][0] == 1117184
    assert tr._offsets() == [off[n] for n in b2.NAMES]
    packed = tr._pack()
    assert packed.dtype == np.float32 and np.array_equal(packed, b2.pack({n: v.numpy() for n, v in zip(b2.NAMES, want)}))
    # one Adam range per variable, the regulariser on the twelve kernels only
    assert tr._adam_ranges() == tuple(off[n] + (n in b2.KERNELS,) for n in b2.NAMES)
    assert len(b2.KERNELS) == 12 and all(n in b2.KERNELS for n in (b2.BLOCK_R[0], b2.BLOCK_3[0], b2.BLOCK_I[0]))
    # the frozen statistics: the three layers' six rows first, then the bottleneck trainer's
    assert list(tr._STATS[:6]) == [(layer, attr) for layer in (b2.REDUCE, b2.CONV3, b2.INCREASE) for attr in ("mean", "variance")]
    assert tuple(tr._STATS[6:]) == tuple(training.ICNetBottleneckTrainer._STATS)
    assert tr._FEATURE_NAMES == ("conv5_1", "conv3_1", "conv3_sub1") and tr._SEMI_NOUN != training.ICNetBottleneckTrainer._SEMI_NOUN
    # the trained variables and nothing else are released from the handle-reuse predicate
    allv = net.variables
    trained = [j for j, v in enumerate(allv) if any(v is t for t in tr._vars())]
    assert len(trained) == 35
    base = tuple(v.version for v in allv)
    ent = [object(), base]
    for j in trained:
        assert tr._handle_reusable(ent, base[:j] + (base[j] + 1,) + base[j + 1:])
    stat = [j for j, v in enumerate(allv) if v is net.conv5_2_3x3.variance][0]
    assert not tr._handle_reusable(ent, base[:stat] + (base[stat] + 1,) + base[stat + 1:])


def test_refusals_come_before_any_device_work(monkeypatch):
    def no_gpu():
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    enet = ssal.ENet(19)
    enet.build((None, None, None, 3))
    with pytest.raises(NotImplementedError):
        training.ICNetDeepBottleneckTrainer(enet, 1e-3)
    net = _icnet()
    with pytest.raises(NotImplementedError):
        training.ICNetDeepBottleneckTrainer.from_params(net, {"hyperparams": dict(AL_HYPER, softmax={"multiscale": True})})
    with pytest.raises(NotImplementedError):
        training.ICNetDeepBottleneckTrainer.from_params(net, {"hyperparams": dict(AL_HYPER, optimizer={"type": "SGD", "kwargs": {}})})
    tr = training.ICNetDeepBottleneckTrainer.from_params(net, {"hyperparams": AL_HYPER})
    assert tr._semi_keywords is False
    assert (tr.learning_rate, tr.beta1, tr.beta2, tr.l2, tr.weight) == (0.0005, 0.9, 0.99, 0.0002, 1.02)
    c51 = np.zeros((1, 1, 2, 1024), np.float32)
    c31, c3 = np.zeros((1, 2, 4, 256), np.float32), np.zeros((1, 4, 8, 64), np.float32)
    lab, msk = np.zeros((1, 32, 64), np.uint8), np.ones((1, 32, 64), np.float32)
    img = np.zeros((1, 32, 32, 3), np.float32)
    ilab, imsk = np.zeros((1, 32, 32), np.uint8), np.ones((1, 32, 32), np.float32)
    # the semi-supervised keywords raise the existing NotImplementedError, under this trainer's own noun
    for kw in ({"labelled": np.array([1])}, {"confusion": np.zeros((19, 19), np.int64)}, {"return_pseudo_pixels": True}):
        with pytest.raises(NotImplementedError, match="deep bottleneck"):
            tr.gradient_features(c51, c31, c3, lab, msk, **kw)
        with pytest.raises(NotImplementedError):
            tr.step_features(c51, c31, c3, lab, msk, **kw)
        with pytest.raises(NotImplementedError):
            tr.step(img, ilab, imsk, **kw)
        with pytest.raises(NotImplementedError):
            tr.gradient(img, ilab, imsk, **kw)
    for call in (lambda: tr.gradient_features(c51[..., :256], c31, c3, lab, msk),               # channels
                 lambda: tr.gradient_features(c51, c31[..., :128], c3, lab, msk),
                 lambda: tr.gradient_features(c51, c31, c3[..., :32], lab, msk),
                 lambda: tr.gradient_features(c51, c31[:, :1], c3, lab, msk),                   # conv3_1 is not 2x
                 lambda: tr.gradient_features(c51, c31, c3[:, :2], lab, msk),                   # conv3_sub1 is not 4x
                 lambda: tr.gradient_features(c51, c31, c3, lab[:, :16], msk),                  # labels / mask are not 32x
                 lambda: tr.gradient_features(c51, c31, c3, lab.astype(np.float32), msk),       # dtypes
                 lambda: tr.gradient_features(c51.astype(np.uint8), c31, c3, lab, msk),
                 lambda: tr.gradient_features(c51, c31.astype(np.uint8), c3, lab, msk),
                 lambda: tr.gradient_features(c51, c31, c3, lab, msk, max_workgroups=-1),
                 lambda: tr.step_features(c51, c31[:, :1], c3, lab, msk),
                 lambda: tr.step(img, ilab[:, :16], imsk),
                 lambda: tr.gradient(img, ilab, imsk, max_workgroups=-1),
                 lambda: tr.gradient_features(c51, c31, c3, lab, msk, params={b2.CONV3 + ".mean": np.zeros(256)}),
                 lambda: tr.gradient_features(c51, c31, c3, lab, msk, params={b2.BLOCK_I[0]: np.zeros((1, 1, 256, 1023))})):
        with pytest.raises(ValueError):
            call()


def test_workspace_arithmetic_and_abi_statuses():
    """the workspace query is the dry form of the size guard (the bottleneck depth's, icnet_bneck_fits): no allocation, no launch"""
    L = _lib.lib()
    ws = L.ssal_icnet_bneck2_grad_workspace_bytes
    top = 1 << 25
    for h, w in ((1, 1), (top, 1), (top + 1, 1), (1, top), (1, top + 1), (46340, 46340), (46341, 46341), (0, 8), (8, 0), (-1, 8),
                 (3, 5)):
        assert (ws(1, h, w, 2) > 0) == (L.ssal_icnet_bneck_grad_workspace_bytes(1, h, w, 2) > 0), (h, w)
    assert ws(1, top + 1, 1, 2) == -1  # an oversize shape: the size query returns -1
    k = 19
    # its own pieces, carved ahead of the bottleneck depth's: the three re-laid-out kernels and their six batch-norm rows,
    # conv5_2_1x1_reduce and conv5_2_3x3 at 256 channels, conv5_2 and g52 at 1024; NO partials of its own: conv5_2's weight
    # gradients reuse conv5_3's, so the bound on the partials' bytes is the bottleneck depth's, whatever the shape
    for n, h, w in ((8, 32, 64), (1, 3, 5)):
        own = (262144 + 589824 + 262144 + 3072 + n * h * w * (2 * 256 + 2 * 1024)) * 4
        up = L.ssal_icnet_bneck_grad_workspace_bytes(n, h, w, k)
        assert own + up - 256 <= ws(n, h, w, k) <= own + up + (1 << 16)
    assert ws(1, 8, 8, 1) == -1 and ws(1, 8, 8, 33) == -1 and ws(0, 8, 8, k) == -1
    p = ctypes.c_void_p(256)
    call = L.ssal_icnet_bneck2_grad_nhwc
    big = 1 << 40
    assert call(p, p, p, 1, 1, 1, 33, p, p, p, 0.0, 0.0, p, 0, p, p, p, big, None) == _lib.SSAL_EINVAL
    assert call(p, p, p, 0, 1, 1, k, p, p, p, 0.0, 0.0, p, 0, p, p, p, big, None) == _lib.SSAL_EINVAL
    assert call(p, p, p, 1, 1, 1, k, p, p, p, 0.0, 0.0, p, -1, p, p, p, big, None) == _lib.SSAL_EINVAL
    assert call(None, p, p, 1, 1, 1, k, p, p, p, 0.0, 0.0, p, 0, p, p, p, big, None) == _lib.SSAL_EINVAL
    assert call(p, None, p, 1, 1, 1, k, p, p, p, 0.0, 0.0, p, 0, p, p, p, big, None) == _lib.SSAL_EINVAL
    assert call(p, p, p, 1, 1, 1, k, p, p, p, 0.0, 0.0, None, 0, p, p, p, big, None) == _lib.SSAL_EINVAL
    assert call(p, p, p, 1, top + 1, 1, k, p, p, p, 0.0, 0.0, p, 0, p, p, p, big, None) == _lib.SSAL_EINVAL  # never launched
    assert call(p, p, p, 1, 1, 1, k, p, p, p, 0.0, 0.0, p, 0, p, p, p, ws(1, 1, 1, k) - 512, None) == _lib.SSAL_ENOMEM
    hd = ctypes.c_void_p()
    _lib.check(L.ssal_icnet_create(3, k, ctypes.byref(hd)))
    assert L.ssal_icnet_train_bneck2_workspace_bytes(hd, 1, 64, 64) == -1
    assert L.ssal_icnet_train_bneck2_nhwc(hd, p, 0, 1, 64, 64, p, p, p, 0.0, 0.0, p, 0, p, p, p, big, None) == _lib.SSAL_ESTATE
    assert L.ssal_icnet_update_bneck2(hd, p, None) == _lib.SSAL_ESTATE
    assert L.ssal_icnet_update_bneck2(None, p, None) == _lib.SSAL_EINVAL
    _lib.check(L.ssal_icnet_destroy(hd))


# ---- an independent float64 statement of conv5_2: torch's own convolutions ----
def _independent_conv5_2(x, d, stats):
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))
    W = {n: t(d[n]).requires_grad_(True) for n in b2.BLOCK}
    bn = lambda y, row, blk: (y - t(stats[row[0]:row[1]])) / torch.sqrt(t(stats[row[1]:row[2]]) + 1e-3) * W[blk[1]] + W[blk[2]]
    nchw = t(x).permute(0, 3, 1, 2)
    r = torch.relu(bn(F.conv2d(nchw, W[b2.BLOCK_R[0]].permute(3, 2, 0, 1)).permute(0, 2, 3, 1), (0, 256, 512), b2.BLOCK_R))
    a = torch.relu(bn(F.conv2d(r.permute(0, 3, 1, 2), W[b2.BLOCK_3[0]].permute(3, 2, 0, 1), padding=4, dilation=4)
                      .permute(0, 2, 3, 1), (512, 768, 1024), b2.BLOCK_3))
    y = bn(F.conv2d(a.permute(0, 3, 1, 2), W[b2.BLOCK_I[0]].permute(3, 2, 0, 1)).permute(0, 2, 3, 1), (1024, 2048, 3072), b2.BLOCK_I)
    return r, a, torch.relu(y + t(x)), W


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 2, 3), (1, 3, 9), (2, 5, 9), (1, 9, 10)])
def test_block_agrees_with_torch_convolutions_and_their_autograd(shape):
    """conv5_2_1x1_reduce, conv5_2_3x3 and conv5_2 of the oracle are torch.conv2d's (dilation 4, padding 4), and the link's
    term-by-term weight gradients are its autograd's for a random un-masked dL/dconv5_2"""
    n, h, w = shape
    x, c31, c3, d, labels, mask = b2.case(31 + h, n, h, w, 3)
    stats = b2.draw_stats(5)
    acts = b2.block_forward(x, b2.pack(d), stats)
    r, a, c52, W = _independent_conv5_2(x, d, stats)
    for got, want in zip(acts, (r, a, c52)):
        assert np.abs(got - want.detach().numpy()).max() <= 1e-12 * max(np.abs(got).max(), 1.0)
    for t in acts:
        assert (t > 0).any() and not (t > 0).all()
    dout = np.random.default_rng(1).standard_normal(c52.shape)
    (c52 * torch.as_tensor(dout)).sum().backward()
    g52 = dout * (acts[2] > 0)
    st = stats.astype(np.float64)
    s = lambda blk, lo: d[blk[1]].astype(np.float64) / np.sqrt(st[lo + len(d[blk[1]]):lo + 2 * len(d[blk[1]])] + 1e-3)
    s_r, s_3, s_i = s(b2.BLOCK_R, 0), s(b2.BLOCK_3, 512), s(b2.BLOCK_I, 1024)
    g3 = ((g52 * s_i) @ d[b2.BLOCK_I[0]].astype(np.float64).reshape(256, 1024).T) * (acts[1] > 0)
    K3 = d[b2.BLOCK_3[0]].astype(np.float64)
    gr = sum(bo.shift(g3 * s_3, -4 * (ky - 1), -4 * (kx - 1)) @ K3[ky, kx].T for ky in range(3) for kx in range(3)) * (acts[0] > 0)
    dK3 = np.stack([np.stack([bo.shift(acts[0], 4 * (ky - 1), 4 * (kx - 1)).reshape(-1, 256).T @ g3.reshape(-1, 256)
                              for kx in range(3)]) for ky in range(3)]) * s_3
    dKr = (x.astype(np.float64).reshape(-1, 1024).T @ gr.reshape(-1, 256)) * s_r
    dKi = (acts[1].reshape(-1, 256).T @ g52.reshape(-1, 1024)) * s_i
    for got, name in ((dK3, b2.BLOCK_3[0]), (dKr.reshape(1, 1, 1024, 256), b2.BLOCK_R[0]), (dKi.reshape(1, 1, 256, 1024), b2.BLOCK_I[0]),
                      (g3.sum((0, 1, 2)), b2.BLOCK_3[2]), (gr.sum((0, 1, 2)), b2.BLOCK_R[2]), (g52.sum((0, 1, 2)), b2.BLOCK_I[2])):
        want = W[name].grad.numpy()
        assert np.abs(got - want).max() <= 1e-9 * max(np.abs(want).max(), 1e-300), name


@pytest.mark.parametrize("shape,k,wl", [((1, 1, 1), 3, (1.02, 0.1)), ((2, 2, 3), 5, (0.0, 0.0)), ((1, 3, 9), 2, (1.02, 0.0))])
def test_oracle_agrees_with_its_term_by_term_backward_and_the_bottleneck_oracle(shape, k, wl):
    n, h, w = shape
    x, c31, c3, d, labels, mask = b2.case(7 + h, n, h, w, k)
    stats = b2.draw_stats(5)
    p = b2.pack(d)
    loss, g = b2.loss_and_grad(x, c31, c3, p, stats, labels, mask, *wl)
    # above conv5_2 the function is icnet_bneck_train_oracle's: the same loss and the same 26 gradients
    c52 = b2.block_forward(x, p, stats)[2]
    bloss, bg = bo.loss_and_grad(c52, c31, c3, p[b2.BLOCK_FLOATS:], stats[b2.STATS_OWN:], labels, mask, *wl)
    assert abs(loss - bloss) <= 1e-12 * abs(bloss)
    assert np.abs(g[b2.BLOCK_FLOATS:] - bg).max() <= 1e-9 * np.abs(bg).max()
    # the term-by-term backward pass of the block (what the kernels compute) is autograd's gradient of the whole depth
    kb = b2.bneck2_backward(x, c31, c3, p, stats, labels, mask, *wl)
    gd = b2.unpack(g)
    for name in b2.BLOCK:
        assert np.abs(gd[name]).max() > 0
        assert np.abs(kb[name] - gd[name]).max() <= 1e-9 * np.abs(gd[name]).max(), name


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 5, 9), (1, 9, 10), (8, 32, 64)])
@pytest.mark.parametrize("k,weight,mw", [(2, 0.0, 0), (19, 1.02, 1), (19, 1.02, 2)])
def test_kappa_continues_section_42s_chain(shape, k, weight, mw):
    """the chain behind gr is section 42's: the new tensors' kappa is the reduce layer's plus exactly the terms section 43 adds"""
    n, h, w = shape
    beta_r = bo.kappa(bo.BLOCK_R[2], n, h, w, k, weight, mw)
    kap = lambda name: b2.kappa(name, n, h, w, k, weight, mw)
    assert kap(b2.BLOCK_I[2]) == beta_r + 3 + 1 + 256 + 1
    assert kap(b2.BLOCK_3[2]) == kap(b2.BLOCK_I[2]) + 3 + 1 + 1024
    assert kap(b2.BLOCK_R[2]) == kap(b2.BLOCK_3[2]) + 3 + 1 + 9 * 256
    assert kap(b2.BLOCK_I[0]) - kap(b2.BLOCK_I[2]) == 3 + 2 - 1 == kap(b2.BLOCK_R[0]) - kap(b2.BLOCK_R[2])
    assert kap(b2.BLOCK_I[1]) - kap(b2.BLOCK_I[2]) == 256 + 2 + 3
    assert kap(b2.BLOCK_3[1]) - kap(b2.BLOCK_3[2]) == 9 * 256 + 9 + 2 + 3
    assert kap(b2.BLOCK_R[1]) - kap(b2.BLOCK_R[2]) == 1024 + 2 + 3
    for name in (bo.BLOCK_R[0], "conv6_cls.bias"):
        assert kap(name) == bo.kappa(name, n, h, w, k, weight, mw)


# the GPU test's sign-coherent cases: shape (N x h32 x w32) x (K, weight, smoothing); seed COHERENT_SEED
COHERENT_SEED = 7
COHERENT_SHAPES = [(2, 5, 9), (1, 9, 10)]
COHERENT_LOSSES = [(2, 0.0, 0.0), (19, 1.02, 0.1)]


@pytest.mark.parametrize("k,weight,ls", COHERENT_LOSSES)
@pytest.mark.parametrize("shape", COHERENT_SHAPES)
def test_bound_discriminates_wrong_backward_passes(shape, k, weight, ls):
    """on the arrays of the GPU test's sign-coherent cases (icnet_bneck2_train_oracle.coherent_case, the same seed), at every
    shape and loss of those cases and at the loosest kappa over max_workgroups 0 / 1 / 2: the three new pre-activations have
    their 30 % quantile at 0, their masks both signs, the last pixel alive; the float64 term-by-term pass stays inside kappa
    2^-24 C_j, and each wrong backward pass of icnet_bneck2_train_oracle.WRONG / WRONG_LOCAL exceeds it at one or more entries
    of EACH tensor it corrupts (icnet_bneck2_train_oracle.CORRUPTS).  Both shapes have 90 pixels: two whole 32-pixel tiles and
    one of 26, so the last pixel and the last split-K group are ragged ones."""
    n, h, w = shape
    x, c31, c3, d, stats, labels, mask = b2.coherent_case(COHERENT_SEED, n, h, w, k)
    p = b2.pack(d)
    acts64 = b2.bneck2_forward(x, c31, c3, p, stats)
    acts = tuple(t.astype(np.float32) for t in acts64)
    for i, c in ((0, 256), (1, 256), (2, 1024)):
        dead = (acts64[i] <= 0).reshape(-1, c).mean(0)
        assert (np.abs(dead - 0.3) <= 2.0 / (n * h * w) + 1e-12).all(), (i, dead.min(), dead.max())
        alive = acts[i] > 0
        assert alive.any() and not alive.all()
        assert alive.reshape(-1, c)[-1].any()  # the last pixel is alive: leaving it out changes the gradients
    for i in (3, 4, 5, 7):  # conv5_3's three masks and conv5_4_k1's vary too
        assert (acts[i] > 0).any() and not (acts[i] > 0).all(), i
    assert ((acts[2] > 0) != (acts[5] > 0)).any()  # conv5_3's mask is another one than conv5_2's
    g, c, _ = b2.grad_and_bound(x, c31, c3, p, stats, labels, mask, weight, ls, acts)
    assert (np.abs(g) <= c * (1 + 1e-9) + 1e-300).all()  # the contraction over magnitudes dominates the gradient
    off = b2.offsets(k)
    bound = {}
    for name in b2.BLOCK:
        lo, hi = off[name]
        bound[name] = max(b2.kappa(name, n, h, w, k, weight, mw) for mw in (0, 1, 2)) * 2.0 ** -24 * c[lo:hi]
        live = np.abs(g[lo:hi]) > 0
        print("%s: median bound / |g| %.3g" % (name, np.median(bound[name][live] / np.abs(g[lo:hi][live]))))
    right = b2.bneck2_backward(x, c31, c3, p, stats, labels, mask, weight, ls, acts)
    for name in b2.BLOCK:
        lo, hi = off[name]
        assert (np.abs(right[name].reshape(-1) - g[lo:hi]) <= 1e-6 * bound[name] + 1e-300).all(), name
    # (the last split-K group at the default grid, 3 groups of one tile, and at max_workgroups = 2, where it is the middle tile)
    for wrong, mw in [(w_, 0) for w_ in b2.WRONG + b2.WRONG_LOCAL] + [("drop_last_group", 2)]:
        got = b2.bneck2_backward(x, c31, c3, p, stats, labels, mask, weight, ls, acts, wrong=wrong, max_workgroups=mw)
        for name in b2.CORRUPTS[wrong]:
            lo, hi = off[name]
            err = np.abs(got[name].reshape(-1) - g[lo:hi])
            over = err > bound[name]
            print("%s mw=%d %s: %d of %d entries beyond the bound, worst x%.3g"
                  % (wrong, mw, name, int(over.sum()), over.size, (err / np.maximum(bound[name], 1e-300)).max()))
            assert over.any(), (wrong, name)
