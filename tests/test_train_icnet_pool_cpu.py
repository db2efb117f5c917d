"""Training of ICNet through its pyramid pooling without a GPU: the trainer and the C ABI's symbols, the
packed layout, the refusals (judged before any device work), the size guard against its Python restatement, the float64 oracle
against an independent autograd statement of the same spec rows and against its own term-by-term backward pass, the pooling
adjoint's matrices against the forward, and the discrimination of the gradient test's bound on the sign-coherent cases: the
wrong backward passes leave it on every tensor they corrupt."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import semanticsegmentationactivelearning_amd as ssal
from semanticsegmentationactivelearning_amd import _lib, training

import final_train_oracle as fto
import icnet_pool_train_oracle as po
import icnet_pyramid_train_oracle as ipo

AL_HYPER = {"learning_rate": 0.0005, "learning_rate_decay": 0.0,
            "optimizer": {"type": "Adam", "kwargs": {"beta1": 0.9, "beta2": 0.99}},
            "weight_reg": {"L2": 0.0002, "L1": 0.0, "glorot_scaling": False},
            "softmax": {"label_smoothing": 0.0, "loginverse_scaling": 1.02, "multiscale": False}}
ABI = ("ssal_icnet_pool_grad_workspace_bytes", "ssal_icnet_pool_grad_nhwc", "ssal_icnet_train_pool_workspace_bytes",
       "ssal_icnet_train_pool_nhwc", "ssal_icnet_update_pool")


def _icnet(k=19):
    net = ssal.ICNet(k)
    net.build((None, None, None, 3))
    return net


def test_trainer_and_abi_symbols_exist():
    """fails on a library / package without the feature"""
    assert issubclass(training.ICNetPoolingTrainer, training.ICNetPyramidTrainer)
    assert not issubclass(training.ICNetPoolingTrainer, training.ICNetHighResTrainer)
    assert "ICNetPoolingTrainer" in training.__all__
    L = _lib.lib()
    i, i64, f, vp = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
    want = {ABI[0]: (i64, [i, i, i, i]),
            ABI[1]: (i, [vp, vp, vp, vp, i, i, i, i, vp, vp, vp, f, f, vp, i, vp, vp, vp, i64, vp]),
            ABI[2]: (i64, [vp, i, i, i]),
            ABI[3]: (i, [vp, vp, i, i, i, i, vp, vp, vp, f, f, vp, i, vp, vp, vp, i64, vp]),
            ABI[4]: (i, [vp, vp, vp])}
    for name in ABI:
        assert _lib.PROTOTYPES[name] == want[name], name
        assert hasattr(L, name)


@pytest.mark.parametrize("k", [2, 19, 32])
def test_packed_offsets_names_and_float_count(k):
    net = _icnet(k)
    tr = training.ICNetPoolingTrainer(net, 1e-3)
    assert tr.variable_names == list(po.NAMES) and len(po.NAMES) == 20
    assert tr.variable_names[3:] == training.ICNetPyramidTrainer.variable_names
    # the names are the model's own attributes for the layer
    assert net.conv5_3_1x1_increase.kernel is tr._vars()[0]
    want = [getattr(getattr(net, n.split(".")[0]), n.split(".")[1]) for n in po.NAMES]
    assert all(a is b for a, b in zip(tr._vars(), want))
    assert [tuple(v.shape) for v in want] == list(po.shapes(k))
    assert tr._floats() == po.floats(k) == 264192 + ipo.floats(k)
    off = po.offsets(k)
    assert off[po.BLOCK[0]] == (0, 262144) and off[po.BLOCK[1]] == (262144, 263168)
    assert off[po.BLOCK[2]] == (263168, 264192) and off["conv5_4_k1.kernel"][0] == 264192
    assert tr._offsets() == [off[n] for n in po.NAMES]
    packed = tr._pack()
    assert packed.dtype == np.float32 and np.array_equal(packed, po.pack({n: v.numpy() for n, v in zip(po.NAMES, want)}))
    # one Adam range per variable, the regulariser on the seven kernels only
    assert tr._adam_ranges() == tuple(off[n] + (n in po.KERNELS,) for n in po.NAMES)
    assert len(po.KERNELS) == 7 and po.BLOCK[0] in po.KERNELS
    # the frozen statistics: the increase layer's two rows first, then the pyramid trainer's
    assert list(tr._STATS[:2]) == [(po.LAYER, "mean"), (po.LAYER, "variance")]
    assert tuple(tr._STATS[2:]) == tuple(training.ICNetPyramidTrainer._STATS)
    # the trained variables and nothing else are released from the handle-reuse predicate
    allv = net.variables
    trained = [j for j, v in enumerate(allv) if any(v is t for t in tr._vars())]
    assert len(trained) == 20
    base = tuple(v.version for v in allv)
    ent = [object(), base]
    for j in trained:
        assert tr._handle_reusable(ent, base[:j] + (base[j] + 1,) + base[j + 1:])
    stat = [j for j, v in enumerate(allv) if v is net.conv5_3_1x1_increase.variance][0]
    assert not tr._handle_reusable(ent, base[:stat] + (base[stat] + 1,) + base[stat + 1:])


def test_refusals_come_before_any_device_work(monkeypatch):
    def no_gpu():
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    enet = ssal.ENet(19)
    enet.build((None, None, None, 3))
    with pytest.raises(NotImplementedError):
        training.ICNetPoolingTrainer(enet, 1e-3)
    net = _icnet()
    with pytest.raises(NotImplementedError):
        training.ICNetPoolingTrainer.from_params(net, {"hyperparams": dict(AL_HYPER, softmax={"multiscale": True})})
    with pytest.raises(NotImplementedError):
        training.ICNetPoolingTrainer.from_params(net, {"hyperparams": dict(AL_HYPER, weight_reg={"L2": 1e-4, "glorot_scaling": True})})
    with pytest.raises(NotImplementedError):
        training.ICNetPoolingTrainer.from_params(net, {"hyperparams": dict(AL_HYPER, optimizer={"type": "SGD", "kwargs": {}})})
    tr = training.ICNetPoolingTrainer.from_params(net, {"hyperparams": AL_HYPER})
    assert tr._semi_keywords is False
    assert (tr.learning_rate, tr.beta1, tr.beta2, tr.l2, tr.weight) == (0.0005, 0.9, 0.99, 0.0002, 1.02)
    a, c52 = np.zeros((1, 1, 2, 256), np.float32), np.zeros((1, 1, 2, 1024), np.float32)
    c31, c3 = np.zeros((1, 2, 4, 256), np.float32), np.zeros((1, 4, 8, 64), np.float32)
    lab, msk = np.zeros((1, 32, 64), np.uint8), np.ones((1, 32, 64), np.float32)
    img = np.zeros((1, 32, 32, 3), np.float32)
    ilab, imsk = np.zeros((1, 32, 32), np.uint8), np.ones((1, 32, 32), np.float32)
    for kw in ({"labelled": np.array([1])}, {"confusion": np.zeros((19, 19), np.int64)}, {"return_pseudo_pixels": True}):
        with pytest.raises(NotImplementedError):
            tr.gradient_features(a, c52, c31, c3, lab, msk, **kw)
        with pytest.raises(NotImplementedError):
            tr.step_features(a, c52, c31, c3, lab, msk, **kw)
        with pytest.raises(NotImplementedError):
            tr.step(img, ilab, imsk, **kw)
        with pytest.raises(NotImplementedError):
            tr.gradient(img, ilab, imsk, **kw)
    for call in (lambda: tr.gradient_features(a[..., :128], c52, c31, c3, lab, msk),            # channels
                 lambda: tr.gradient_features(a, c52[..., :256], c31, c3, lab, msk),
                 lambda: tr.gradient_features(a, c52, c31[..., :128], c3, lab, msk),
                 lambda: tr.gradient_features(a, c52, c31, c3[..., :32], lab, msk),
                 lambda: tr.gradient_features(a, c52[:, :, :1], c31, c3, lab, msk),             # conv5_2 is not conv5_3_3x3's map
                 lambda: tr.gradient_features(a, c52, c31[:, :1], c3, lab, msk),                # conv3_1 is not 2x
                 lambda: tr.gradient_features(a, c52, c31, c3[:, :2], lab, msk),                # conv3_sub1 is not 4x
                 lambda: tr.gradient_features(a, c52, c31, c3, lab[:, :16], msk),               # labels / mask are not 32x
                 lambda: tr.gradient_features(a, c52, c31, c3, lab.astype(np.float32), msk),    # dtypes
                 lambda: tr.gradient_features(a.astype(np.uint8), c52, c31, c3, lab, msk),
                 lambda: tr.gradient_features(a, c52.astype(np.uint8), c31, c3, lab, msk),
                 lambda: tr.gradient_features(a, c52, c31, c3, lab, msk, max_workgroups=-1),
                 lambda: tr.step_features(a, c52, c31[:, :1], c3, lab, msk),
                 lambda: tr.step(img, ilab[:, :16], imsk),
                 lambda: tr.gradient(img, ilab, imsk, max_workgroups=-1),
                 lambda: tr.gradient_features(a, c52, c31, c3, lab, msk, params={po.LAYER + ".mean": np.zeros(1024)}),
                 lambda: tr.gradient_features(a, c52, c31, c3, lab, msk, params={po.BLOCK[1]: np.zeros(1023)})):
        with pytest.raises(ValueError):
            call()


def pool_fits(h32, w32):
    """icnet_pool_fits restated: the cascade depth's limits -- 2 h32 <= 2^26 coordinates, and fewer than 2^31 tiles of the head
    kernel (one 8 x 8 tile of lq per pixel of conv5_3 and image)"""
    top = 1 << 25
    return 1 <= h32 <= top and 1 <= w32 <= top and h32 * w32 < (1 << 31)


def test_size_guard_agrees_with_its_restatement_and_abi_statuses():
    """the workspace query is the dry form of icnet_pool_fits: no allocation, no launch"""
    L = _lib.lib()
    ws = L.ssal_icnet_pool_grad_workspace_bytes
    top = 1 << 25
    for h, w in ((1, 1), (top, 1), (top + 1, 1), (1, top), (1, top + 1), (top, 63), (top, 64), (46340, 46340), (46341, 46341),
                 (0, 8), (8, 0), (-1, 8), (3, 5)):
        assert (ws(1, h, w, 2) > 0) == pool_fits(h, w), (h, w)
        assert (ws(1, h, w, 2) > 0) == (L.ssal_icnet_pyramid_grad_workspace_bytes(1, h, w, 2) > 0), (h, w)
    k = 19
    # its own pieces, carved ahead of the pyramid depth's: conv5_3, conv5_3_sum, dsum and g53 at 1024 channels, the pooling's
    # scratch (50 bins and 12 column slots a row), the adjoint's column sums and bin gradients, 16 split-K partials of 257 x 1024
    # and their fold, the re-laid-out kernel and its batch-norm row; then everything the pyramid entry takes
    n, h, w = 8, 32, 64
    own = (4 * n * h * w * 1024 + n * (50 + 12 * h) * 1024 + n * h * 12 * 1024 + n * 50 * 1024 + 17 * 257 * 1024 + 262144
           + 2048) * 4
    pyramid = L.ssal_icnet_pyramid_grad_workspace_bytes(n, h, w, k)
    assert own + pyramid - 256 <= ws(n, h, w, k) <= own + pyramid + (1 << 16)
    assert ws(1, 8, 8, 1) == -1 and ws(1, 8, 8, 33) == -1 and ws(0, 8, 8, k) == -1
    p = ctypes.c_void_p(256)
    call = L.ssal_icnet_pool_grad_nhwc
    big = 1 << 40
    assert call(p, p, p, p, 1, 1, 1, 33, p, p, p, 0.0, 0.0, p, 0, p, p, p, big, None) == _lib.SSAL_EINVAL
    assert call(p, p, p, p, 0, 1, 1, k, p, p, p, 0.0, 0.0, p, 0, p, p, p, big, None) == _lib.SSAL_EINVAL
    assert call(p, p, p, p, 1, 1, 1, k, p, p, p, 0.0, 0.0, p, -1, p, p, p, big, None) == _lib.SSAL_EINVAL
    assert call(None, p, p, p, 1, 1, 1, k, p, p, p, 0.0, 0.0, p, 0, p, p, p, big, None) == _lib.SSAL_EINVAL
    assert call(p, None, p, p, 1, 1, 1, k, p, p, p, 0.0, 0.0, p, 0, p, p, p, big, None) == _lib.SSAL_EINVAL
    assert call(p, p, p, p, 1, 1, 1, k, p, p, p, 0.0, 0.0, None, 0, p, p, p, big, None) == _lib.SSAL_EINVAL
    assert call(p, p, p, p, 1, top + 1, 1, k, p, p, p, 0.0, 0.0, p, 0, p, p, p, big, None) == _lib.SSAL_EINVAL  # never launched
    assert call(p, p, p, p, 1, 1, 1, k, p, p, p, 0.0, 0.0, p, 0, p, p, p, ws(1, 1, 1, k) - 512, None) == _lib.SSAL_ENOMEM
    hd = ctypes.c_void_p()
    _lib.check(L.ssal_icnet_create(3, k, ctypes.byref(hd)))
    assert L.ssal_icnet_train_pool_workspace_bytes(hd, 1, 64, 64) == -1
    assert L.ssal_icnet_train_pool_nhwc(hd, p, 0, 1, 64, 64, p, p, p, 0.0, 0.0, p, 0, p, p, p, big, None) == _lib.SSAL_ESTATE
    assert L.ssal_icnet_update_pool(hd, p, None) == _lib.SSAL_ESTATE
    assert L.ssal_icnet_update_pool(None, p, None) == _lib.SSAL_EINVAL
    _lib.check(L.ssal_icnet_destroy(hd))


# ---- an independent float64 statement of spec rows conv5_3 ... conv5_3_sum: torch's own convolution and adaptive pooling (whose
# bins are [floor(i h / b), ceil((i + 1) h / b)) too), a select-and-blend resize on the spec's fp32 source positions ----
def _resize_to(v, size, axis):
    bins = v.shape[axis]
    src = np.arange(size, dtype=np.float32) * (np.float32(bins) / np.float32(size))
    i0 = np.floor(src).astype(np.int64)
    i1 = np.minimum(i0 + 1, bins - 1)
    frac = torch.as_tensor((src - i0.astype(np.float32)).astype(np.float64))
    shape = [1, 1, 1, 1]
    shape[axis] = -1
    frac = frac.reshape(shape)
    return v.index_select(axis, torch.as_tensor(i0)) * (1.0 - frac) + v.index_select(axis, torch.as_tensor(i1)) * frac


def _independent_sum(a, c52, d, stats):
    t = lambda x: torch.as_tensor(np.asarray(x, dtype=np.float64))
    W = {n: t(d[n]).requires_grad_(True) for n in po.BLOCK}
    y = F.conv2d(t(a).permute(0, 3, 1, 2), W[po.BLOCK[0]].permute(3, 2, 0, 1)).permute(0, 2, 3, 1)
    y = (y - t(stats[:1024])) / torch.sqrt(t(stats[1024:2048]) + 1e-3) * W[po.BLOCK[1]] + W[po.BLOCK[2]]
    c53 = torch.relu(y + t(c52))
    h, w = c53.shape[1:3]
    out = c53
    for b in (1, 2, 3, 6):
        v = F.adaptive_avg_pool2d(c53.permute(0, 3, 1, 2), b).permute(0, 2, 3, 1)
        out = out + _resize_to(_resize_to(v, w, 2), h, 1)
    return out, W


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 2, 3), (1, 3, 2), (1, 3, 5), (2, 5, 9)])
def test_pooling_forward_and_adjoint_agree_with_an_independent_statement(shape):
    """conv5_3_sum of the oracle is the independent statement's; the explicit per-level matrices reproduce it (forward) and their
    transposes are autograd's adjoint of the independent statement; the adds per pixel the bound counts are those of the bins"""
    n, h, w = shape
    a, c52, c31, c3, d, labels, mask = po.case(31 + h, n, h, w, 3)
    stats = po.draw_stats(5)
    c53, s53 = po.pool_forward(a, c52, c31, c3, po.pack(d), stats)[:2]
    want, W = _independent_sum(a, c52, d, stats)
    assert np.abs(s53 - want.detach().numpy()).max() <= 1e-12 * np.abs(s53).max()
    flat = c53.reshape(n, h * w, 1024)
    viam = flat.copy()
    for b in po.LEVELS:
        R, A = po.level_matrices(b, h, w)
        assert np.allclose(R.sum(1), 1.0) and np.allclose(A.sum(1), 1.0)
        viam = viam + np.einsum("pq,nqc->npc", R @ A, flat)
    assert np.abs(viam.reshape(s53.shape) - s53).max() <= 1e-12 * np.abs(s53).max()
    rng = np.random.default_rng(1)
    dsum = rng.standard_normal(s53.shape)
    (want * torch.as_tensor(dsum)).sum().backward()
    mine = po.ppm_adjoint(dsum) * (c53 > 0)
    g = mine.reshape(-1, 1024)
    s = d[po.BLOCK[1]].astype(np.float64) / np.sqrt(stats[1024:2048].astype(np.float64) + 1e-3)
    dK = (a.astype(np.float64).reshape(-1, 256).T @ g) * s
    assert np.abs(dK - W[po.BLOCK[0]].grad.numpy().reshape(256, 1024)).max() <= 1e-9 * np.abs(dK).max()
    assert np.abs(g.sum(0) - W[po.BLOCK[2]].grad.numpy()).max() <= 1e-9 * np.abs(g.sum(0)).max()
    assert 5 <= po.bins_per_pixel(h, w) <= 50


@pytest.mark.parametrize("shape,k,wl", [((1, 1, 1), 3, (1.02, 0.1)), ((2, 2, 3), 5, (0.0, 0.0)), ((1, 3, 5), 2, (1.02, 0.0))])
def test_oracle_agrees_with_its_term_by_term_backward_and_the_pyramid_oracle(shape, k, wl):
    n, h, w = shape
    a, c52, c31, c3, d, labels, mask = po.case(7 + h, n, h, w, k)
    stats = po.draw_stats(5)
    p = po.pack(d)
    loss, g = po.loss_and_grad(a, c52, c31, c3, p, stats, labels, mask, *wl)
    # above conv5_3_sum the function is icnet_pyramid_train_oracle's: the same loss and the same seventeen gradients
    s53 = po.pool_forward(a, c52, c31, c3, p, stats)[1]
    ploss, pg = ipo.loss_and_grad(s53, c31, c3, p[po.BLOCK_FLOATS:], stats[po.STATS_OWN:], labels, mask, *wl)
    assert abs(loss - ploss) <= 1e-12 * abs(ploss)
    assert np.abs(g[po.BLOCK_FLOATS:] - pg).max() <= 1e-9 * np.abs(pg).max()
    # the term-by-term backward pass of the increase layer (what the kernels compute) is the same gradient
    kb = po.pool_backward(a, c52, c31, c3, p, stats, labels, mask, *wl)
    gd = po.unpack(g)
    for name in po.BLOCK:
        assert np.abs(gd[name]).max() > 0
        assert np.abs(kb[name] - gd[name]).max() <= 1e-9 * np.abs(gd[name]).max(), name


# the GPU test's sign-coherent cases: shape (N x h32 x w32) x (K, weight, smoothing); seed COHERENT_SEED
COHERENT_SEED = 7
COHERENT_SHAPES = [(1, 3, 5), (2, 5, 9)]
COHERENT_LOSSES = [(2, 0.0, 0.0), (19, 1.02, 0.1)]
# what each wrong pass corrupts: the first seven change g53 itself, so all three tensors; the kernel-local ones as stated
CORRUPTS = {w: po.BLOCK for w in po.WRONG}
CORRUPTS.update({"drop_last_pixel": po.BLOCK, "drop_last_group": po.BLOCK, "no_mean_term": (po.BLOCK[1],),
                 "kernel_10_percent": po.BLOCK[:2]})


@pytest.mark.parametrize("k,weight,ls", COHERENT_LOSSES)
@pytest.mark.parametrize("shape", COHERENT_SHAPES)
def test_bound_discriminates_wrong_backward_passes(shape, k, weight, ls):
    """on the arrays of the GPU test's sign-coherent cases (icnet_pool_train_oracle.coherent_case, the same seed), at every
    shape and loss of those cases and at the loosest kappa over max_workgroups 0 / 1 / 2: the float64 reference stays inside
    kappa 2^-24 C_j, and each wrong backward pass -- no conv5_3 > 0 mask, the identity term only, the pooled levels only,
    non-overlapping bins, no division by the count, the half-pixel resize adjoint, no s1, the last pixel or (at the ragged shape)
    the last split-K group left out of the weight gradient -- exceeds it at one or more entries of EACH of the increase layer's
    three tensors; a dGamma without - mean dBeta leaves it on dGamma, a kernel gradient 10 % off on the kernel and on dGamma."""
    n, h, w = shape
    a, c52, c31, c3, d, stats, labels, mask = po.coherent_case(COHERENT_SEED, n, h, w, k)
    p = po.pack(d)
    acts = tuple(t.astype(np.float32) for t in po.pool_forward(a, c52, c31, c3, p, stats))
    alive = acts[0] > 0
    assert alive.any() and not alive.all()  # conv5_3's ReLU mask varies
    alive1 = acts[2] > 0
    assert alive1.any() and not alive1.all()  # and conv5_4_k1's
    g, c, _ = po.grad_and_bound(a, c52, c31, c3, p, stats, labels, mask, weight, ls, acts)
    assert (np.abs(g) <= c * (1 + 1e-9) + 1e-300).all()  # the contraction over magnitudes dominates the gradient
    off = po.offsets(k)
    bound = {}
    for name in po.BLOCK:
        lo, hi = off[name]
        bound[name] = max(po.kappa(name, n, h, w, k, weight, mw) for mw in (0, 1, 2)) * 2.0 ** -24 * c[lo:hi]
        live = np.abs(g[lo:hi]) > 0
        print("%s: median bound / |g| %.3g" % (name, np.median(bound[name][live] / np.abs(g[lo:hi][live]))))
    right = po.pool_backward(a, c52, c31, c3, p, stats, labels, mask, weight, ls, acts)
    for name in po.BLOCK:
        lo, hi = off[name]
        assert (np.abs(right[name].reshape(-1) - g[lo:hi]) <= 1e-6 * bound[name] + 1e-300).all(), name
    for wrong in po.WRONG + po.WRONG_LOCAL:
        if wrong.startswith("drop_last") and n * h * w <= 64:
            # the ragged shape's variants: P = 90 is two whole 32-pixel tiles and one of 26.  (At (1, 3, 5) the last of the 15
            # pixels carries one of the small per-pixel factors and lies under the 30 % quantile in every channel: conv5_3 is
            # dead there, g53 is zero, and leaving the pixel out changes no gradient -- nothing to discriminate.)
            continue
        got = po.pool_backward(a, c52, c31, c3, p, stats, labels, mask, weight, ls, acts, wrong=wrong)
        for name in CORRUPTS[wrong]:
            lo, hi = off[name]
            err = np.abs(got[name].reshape(-1) - g[lo:hi])
            over = err > bound[name]
            print("%s %s: %d of %d entries beyond the bound, worst x%.3g"
                  % (wrong, name, int(over.sum()), over.size, (err / np.maximum(bound[name], 1e-300)).max()))
            assert over.any(), (wrong, name)
