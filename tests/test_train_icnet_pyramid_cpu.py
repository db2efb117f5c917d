"""Training of ICNet's pyramid head without a GPU: the trainer and the C ABI's symbols, the packed layout,
the refusals (judged before any device work), the size guard against its Python restatement, the float64 oracle against an
independent autograd statement of the same spec rows and against its own term-by-term backward pass, and the discrimination of
the gradient test's bound on the sign-coherent cases: nine wrong backward passes leave it on every tensor they corrupt."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import semanticsegmentationactivelearning_amd as ssal
from semanticsegmentationactivelearning_amd import _lib, training

import final_train_oracle as fto
import icnet_cascade_train_oracle as ico
import icnet_pyramid_train_oracle as ipo

AL_HYPER = {"learning_rate": 0.0005, "learning_rate_decay": 0.0,
            "optimizer": {"type": "Adam", "kwargs": {"beta1": 0.9, "beta2": 0.99}},
            "weight_reg": {"L2": 0.0002, "L1": 0.0, "glorot_scaling": False},
            "softmax": {"label_smoothing": 0.0, "loginverse_scaling": 1.02, "multiscale": False}}
ABI = ("ssal_icnet_pyramid_grad_workspace_bytes", "ssal_icnet_pyramid_grad_nhwc", "ssal_icnet_train_pyramid_workspace_bytes",
       "ssal_icnet_train_pyramid_nhwc", "ssal_icnet_update_pyramid")


def _icnet(k=19):
    net = ssal.ICNet(k)
    net.build((None, None, None, 3))
    return net


def test_trainer_and_abi_symbols_exist():
    """fails on a library / package without the feature"""
    assert issubclass(training.ICNetPyramidTrainer, training.ICNetCascadeTrainer)
    assert not issubclass(training.ICNetPyramidTrainer, training.ICNetHighResTrainer)  # siblings
    assert not issubclass(training.ICNetHighResTrainer, training.ICNetPyramidTrainer)
    assert "ICNetPyramidTrainer" in training.__all__
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
    tr = training.ICNetPyramidTrainer(net, 1e-3)
    assert tr.variable_names == list(ipo.NAMES) and len(ipo.NAMES) == 17
    assert tr.variable_names[3:] == training.ICNetCascadeTrainer.variable_names
    want = [getattr(getattr(net, n.split(".")[0]), n.split(".")[1]) for n in ipo.NAMES]
    assert all(a is b for a, b in zip(tr._vars(), want))
    assert [tuple(v.shape) for v in want] == list(ipo.shapes(k))
    assert tr._floats() == ipo.floats(k) == 262656 + ico.floats(k)
    off = ipo.offsets(k)
    assert off["conv5_4_k1.kernel"] == (0, 262144) and off["conv5_4_k1.gamma"] == (262144, 262400)
    assert off["conv5_4_k1.beta"] == (262400, 262656) and off["conv_sub4.kernel"][0] == 262656
    assert tr._offsets() == [off[n] for n in ipo.NAMES]
    packed = tr._pack()
    assert packed.dtype == np.float32 and np.array_equal(packed, ipo.pack({n: v.numpy() for n, v in zip(ipo.NAMES, want)}))
    # one Adam range per variable, the regulariser on the six kernels only
    assert tr._adam_ranges() == tuple(off[n] + (n in ipo.KERNELS,) for n in ipo.NAMES)
    assert len(ipo.KERNELS) == 6 and "conv5_4_k1.kernel" in ipo.KERNELS
    # the frozen statistics: conv5_4_k1's two rows first, then the cascade trainer's
    assert list(tr._STATS[:2]) == [("conv5_4_k1", "mean"), ("conv5_4_k1", "variance")]
    assert tuple(tr._STATS[2:]) == tuple(training.ICNetCascadeTrainer._STATS)
    # the trained variables and nothing else are released from the handle-reuse predicate
    allv = net.variables
    trained = [j for j, v in enumerate(allv) if any(v is t for t in tr._vars())]
    assert len(trained) == 17
    base = tuple(v.version for v in allv)
    ent = [object(), base]
    for j in trained:
        assert tr._handle_reusable(ent, base[:j] + (base[j] + 1,) + base[j + 1:])
    stat = [j for j, v in enumerate(allv) if v is net.conv5_4_k1.variance][0]
    assert not tr._handle_reusable(ent, base[:stat] + (base[stat] + 1,) + base[stat + 1:])


def test_refusals_come_before_any_device_work(monkeypatch):
    def no_gpu():
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    enet = ssal.ENet(19)
    enet.build((None, None, None, 3))
    with pytest.raises(NotImplementedError):
        training.ICNetPyramidTrainer(enet, 1e-3)
    net = _icnet()
    with pytest.raises(NotImplementedError):
        training.ICNetPyramidTrainer.from_params(net, {"hyperparams": dict(AL_HYPER, softmax={"multiscale": True})})
    with pytest.raises(NotImplementedError):
        training.ICNetPyramidTrainer.from_params(net, {"hyperparams": dict(AL_HYPER, weight_reg={"L2": 1e-4, "glorot_scaling": True})})
    with pytest.raises(NotImplementedError):
        training.ICNetPyramidTrainer.from_params(net, {"hyperparams": dict(AL_HYPER, optimizer={"type": "SGD", "kwargs": {}})})
    tr = training.ICNetPyramidTrainer.from_params(net, {"hyperparams": AL_HYPER})
    assert tr._semi_keywords is False
    assert (tr.learning_rate, tr.beta1, tr.beta2, tr.l2, tr.weight) == (0.0005, 0.9, 0.99, 0.0002, 1.02)
    c53, c31 = np.zeros((1, 1, 2, 1024), np.float32), np.zeros((1, 2, 4, 256), np.float32)
    c3 = np.zeros((1, 4, 8, 64), np.float32)
    lab, msk = np.zeros((1, 32, 64), np.uint8), np.ones((1, 32, 64), np.float32)
    img = np.zeros((1, 32, 32, 3), np.float32)
    ilab, imsk = np.zeros((1, 32, 32), np.uint8), np.ones((1, 32, 32), np.float32)
    for kw in ({"labelled": np.array([1])}, {"confusion": np.zeros((19, 19), np.int64)}, {"return_pseudo_pixels": True}):
        with pytest.raises(NotImplementedError):
            tr.gradient_features(c53, c31, c3, lab, msk, **kw)
        with pytest.raises(NotImplementedError):
            tr.step_features(c53, c31, c3, lab, msk, **kw)
        with pytest.raises(NotImplementedError):
            tr.step(img, ilab, imsk, **kw)
        with pytest.raises(NotImplementedError):
            tr.gradient(img, ilab, imsk, **kw)
    for call in (lambda: tr.gradient_features(c53[..., :256], c31, c3, lab, msk),            # channels
                 lambda: tr.gradient_features(c53, c31[..., :128], c3, lab, msk),
                 lambda: tr.gradient_features(c53, c31, c3[..., :32], lab, msk),
                 lambda: tr.gradient_features(c53, c31[:, :1], c3, lab, msk),                # conv3_1 is not 2x conv5_3_sum
                 lambda: tr.gradient_features(c53, c31, c3[:, :2], lab, msk),                # conv3_sub1 is not 4x
                 lambda: tr.gradient_features(c53, c31, c3, lab[:, :16], msk),               # labels / mask are not 32x
                 lambda: tr.gradient_features(c53, c31, c3, lab.astype(np.float32), msk),    # dtypes
                 lambda: tr.gradient_features(c53.astype(np.uint8), c31, c3, lab, msk),
                 lambda: tr.gradient_features(c53, c31, c3, lab, msk, max_workgroups=-1),
                 lambda: tr.step_features(c53, c31[:, :1], c3, lab, msk),
                 lambda: tr.step(img, ilab[:, :16], imsk),
                 lambda: tr.gradient(img, ilab, imsk, max_workgroups=-1),
                 lambda: tr.gradient_features(c53, c31, c3, lab, msk, params={"conv5_4_k1.mean": np.zeros(256)}),
                 lambda: tr.gradient_features(c53, c31, c3, lab, msk, params={"conv5_4_k1.gamma": np.zeros(255)})):
        with pytest.raises(ValueError):
            call()


def pyramid_fits(h32, w32):
    """icnet_pyramid_fits restated: the cascade depth's limits -- 2 h32 <= 2^26 coordinates, and fewer than 2^31 tiles of the
    head kernel (one 8 x 8 tile of lq per pixel of conv5_4_k1 and image)"""
    top = 1 << 25
    return 1 <= h32 <= top and 1 <= w32 <= top and h32 * w32 < (1 << 31)


def test_size_guard_agrees_with_its_restatement_and_abi_statuses():
    """the workspace query is the dry form of icnet_pyramid_fits: no allocation, no launch"""
    L = _lib.lib()
    ws = L.ssal_icnet_pyramid_grad_workspace_bytes
    top = 1 << 25
    for h, w in ((1, 1), (top, 1), (top + 1, 1), (1, top), (1, top + 1), (top, 63), (top, 64), (46340, 46340), (46341, 46341),
                 (0, 8), (8, 0), (-1, 8), (3, 5)):
        assert (ws(1, h, w, 2) > 0) == pyramid_fits(h, w), (h, w)
        assert (ws(1, h, w, 2) > 0) == (L.ssal_icnet_cascade_grad_workspace_bytes(1, h, w, 2) > 0), (h, w)
    k = 19
    # its own pieces: conv5_4_k1, g32 and the four-fold du at 256 channels, 16 split-K partials of 1025 x 256 and their fold,
    # the re-laid-out kernel; then everything the cascade entry takes
    n, h, w = 8, 32, 64
    own = (6 * n * h * w * 256 + 17 * 1025 * 256 + 262144 + 512) * 4
    cascade = L.ssal_icnet_cascade_grad_workspace_bytes(n, h, w, k)
    assert own + cascade - 256 <= ws(n, h, w, k) <= own + cascade + (1 << 16)
    assert ws(1, 8, 8, 1) == -1 and ws(1, 8, 8, 33) == -1 and ws(0, 8, 8, k) == -1
    p = ctypes.c_void_p(256)
    call = L.ssal_icnet_pyramid_grad_nhwc
    big = 1 << 40
    assert call(p, p, p, 1, 1, 1, 33, p, p, p, 0.0, 0.0, p, 0, p, p, p, big, None) == _lib.SSAL_EINVAL
    assert call(p, p, p, 0, 1, 1, k, p, p, p, 0.0, 0.0, p, 0, p, p, p, big, None) == _lib.SSAL_EINVAL
    assert call(p, p, p, 1, 1, 1, k, p, p, p, 0.0, 0.0, p, -1, p, p, p, big, None) == _lib.SSAL_EINVAL
    assert call(None, p, p, 1, 1, 1, k, p, p, p, 0.0, 0.0, p, 0, p, p, p, big, None) == _lib.SSAL_EINVAL
    assert call(p, p, p, 1, 1, 1, k, p, p, p, 0.0, 0.0, None, 0, p, p, p, big, None) == _lib.SSAL_EINVAL
    assert call(p, p, p, 1, top + 1, 1, k, p, p, p, 0.0, 0.0, p, 0, p, p, p, big, None) == _lib.SSAL_EINVAL  # never launched
    assert call(p, p, p, 1, 1, 1, k, p, p, p, 0.0, 0.0, p, 0, p, p, p, ws(1, 1, 1, k) - 512, None) == _lib.SSAL_ENOMEM
    hd = ctypes.c_void_p()
    _lib.check(L.ssal_icnet_create(3, k, ctypes.byref(hd)))
    assert L.ssal_icnet_train_pyramid_workspace_bytes(hd, 1, 64, 64) == -1
    assert L.ssal_icnet_train_pyramid_nhwc(hd, p, 0, 1, 64, 64, p, p, p, 0.0, 0.0, p, 0, p, p, p, big, None) == _lib.SSAL_ESTATE
    assert L.ssal_icnet_update_pyramid(hd, p, None) == _lib.SSAL_ESTATE
    assert L.ssal_icnet_update_pyramid(None, p, None) == _lib.SSAL_EINVAL
    _lib.check(L.ssal_icnet_destroy(hd))


# ---- an independent float64 statement of spec rows conv5_4_k1 ... logits: torch's own convolutions, an index-gather resize ----
def _resize_gather(x, f):
    """legacy bilinear (src = dst / f, the +1 tap clamped to the map) on NHWC by explicit gathers"""
    for axis in (1, 2):
        size = x.shape[axis]
        dst = torch.arange(f * size)
        i0 = dst // f
        i1 = torch.clamp(i0 + 1, max=size - 1)
        frac = (dst - f * i0).double() / f
        shape = [1, 1, 1, 1]
        shape[axis] = -1
        frac = frac.reshape(shape)
        x = x.index_select(axis, i0) * (1.0 - frac) + x.index_select(axis, i1) * frac
    return x


def _independent_loss(c53, c31, c3, d, stats, labels, mask, weight, ls):
    k = int(np.asarray(d["conv6_cls.bias"]).size)
    W = {n: torch.as_tensor(np.asarray(v, dtype=np.float64)).requires_grad_(True) for n, v in d.items()}
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))
    rows, lo = {}, 0
    for layer, width in (("conv5_4_k1", 256), ("conv_sub4", 128), ("conv3_1_sub2_proj", 128), ("conv_sub2", 128),
                         ("conv3_sub1_proj", 128)):
        rows[layer] = (t(stats[lo:lo + width]), t(stats[lo + width:lo + 2 * width]))
        lo += 2 * width

    def conv_bn(x, layer, dil=1):
        kern = W[layer + ".kernel"]
        pad = dil * (kern.shape[0] // 2)
        y = F.conv2d(x.permute(0, 3, 1, 2), kern.permute(3, 2, 0, 1), padding=pad, dilation=dil).permute(0, 2, 3, 1)
        mean, var = rows[layer]
        return (y - mean) / torch.sqrt(var + 1e-3) * W[layer + ".gamma"] + W[layer + ".beta"]

    f1 = torch.relu(conv_bn(t(c53), "conv5_4_k1"))
    s24 = torch.relu(conv_bn(_resize_gather(f1, 2), "conv_sub4", 2) + conv_bn(t(c31), "conv3_1_sub2_proj"))
    s12 = torch.relu(conv_bn(_resize_gather(s24, 2), "conv_sub2", 2) + conv_bn(t(c3), "conv3_sub1_proj"))
    lq = _resize_gather(s12, 2) @ W["conv6_cls.kernel"].reshape(128, k) + W["conv6_cls.bias"]
    lg = _resize_gather(lq, 4)
    on, off, w32, c_w = fto.xent_constants(k, weight, ls)
    loss = fto.pixel_loss(lg, fto.one_hot(labels, k, on, off), t(mask), w32, c_w, True).sum() * fto.mask_scale(mask)
    loss.backward()
    return float(loss.detach()), ipo.pack({n: W[n].grad.numpy() for n in ipo.NAMES})


@pytest.mark.parametrize("shape,k,wl", [((1, 1, 1), 3, (1.02, 0.1)), ((2, 2, 3), 5, (0.0, 0.0))])
def test_oracle_agrees_with_an_independent_autograd_statement(shape, k, wl):
    n, h, w = shape
    c53, c31, c3, d, labels, mask = ipo.case(7 + h, n, h, w, k)
    stats = ipo.draw_stats(5)
    loss, g = ipo.loss_and_grad(c53, c31, c3, ipo.pack(d), stats, labels, mask, *wl)
    iloss, ig = _independent_loss(c53, c31, c3, d, stats, labels, mask, *wl)
    assert abs(loss - iloss) <= 1e-12 * abs(iloss)
    for name, (lo, hi) in ipo.offsets(k).items():
        scale = np.abs(ig[lo:hi]).max()
        assert scale > 0 or name.endswith("kernel"), name
        # two float64 evaluations of one function in different association orders
        assert np.abs(g[lo:hi] - ig[lo:hi]).max() <= 1e-9 * max(scale, 1e-30), name
    # the term-by-term backward pass of conv5_4_k1 (what the kernels compute) is the same gradient
    kb = ipo.k1_backward(c53, c31, c3, ipo.pack(d), stats, labels, mask, *wl)
    gd = ipo.unpack(g)
    for name in ipo.BLOCK:
        assert np.abs(kb[name] - gd[name]).max() <= 1e-9 * np.abs(gd[name]).max(), name


# the GPU test's sign-coherent cases: shape (N x h32 x w32) x (K, weight, smoothing); seed COHERENT_SEED
COHERENT_SEED = 7
COHERENT_SHAPES = [(1, 3, 5), (2, 5, 9)]
COHERENT_LOSSES = [(2, 0.0, 0.0), (19, 1.02, 0.1)]
# what each wrong pass corrupts: the issue's five change g32 itself, so all three tensors; the kernel-local ones as stated
CORRUPTS = {w: ipo.BLOCK for w in ipo.WRONG}
CORRUPTS.update({"drop_last_pixel": ipo.BLOCK, "drop_last_group": ipo.BLOCK, "no_mean_term": (ipo.BLOCK[1],),
                 "kernel_10_percent": ipo.BLOCK[:2]})


@pytest.mark.parametrize("k,weight,ls", COHERENT_LOSSES)
@pytest.mark.parametrize("shape", COHERENT_SHAPES)
def test_bound_discriminates_wrong_backward_passes(shape, k, weight, ls):
    """on the arrays of the GPU test's sign-coherent cases (icnet_pyramid_train_oracle.coherent_case, the same seed), at every
    shape and loss of those cases and at the loosest kappa over max_workgroups 0 / 1 / 2: a backward pass without the ReLU mask
    of conv5_4_k1, with the half-pixel resize adjoint, without scale_c in the data gradient, with dilation 1, or with the padding
    after instead of before exceeds kappa 2^-24 C_j at one or more entries of EACH of conv5_4_k1's three tensors; so does a
    weight gradient that leaves out the last pixel (a ragged tile cut short) or, at the ragged shape, everything past the
    second 32-pixel tile (a split-K group dropped); a dGamma without - mean dBeta leaves the bound on dGamma, a kernel gradient
    10 % off on the kernel and on dGamma.  On the inputs of random sign of the other cases C_j lies 10^2 .. 10^5 above |g_j|
    and most of these stay inside the bound (dGamma: 0.03 - 0.11 of it); that is why the coherent cases exist."""
    n, h, w = shape
    c53, c31, c3, d, stats, labels, mask = ipo.coherent_case(COHERENT_SEED, n, h, w, k)
    p = ipo.pack(d)
    acts = [a.astype(np.float32) for a in ipo.pyramid_forward(c53, c31, c3, p, stats)]
    alive = acts[0] > 0
    assert alive.any() and not alive.all()  # conv5_4_k1's ReLU mask varies
    g, c, _ = ipo.grad_and_bound(c53, c31, c3, p, stats, labels, mask, weight, ls, *acts)
    assert (np.abs(g) <= c * (1 + 1e-9) + 1e-300).all()  # the contraction over magnitudes dominates the gradient
    off = ipo.offsets(k)
    bound = {}
    for name in ipo.BLOCK:
        lo, hi = off[name]
        bound[name] = max(ipo.kappa(name, n, h, w, k, weight, mw) for mw in (0, 1, 2)) * 2.0 ** -24 * c[lo:hi]
        live = np.abs(g[lo:hi]) > 0
        print("%s: median bound / |g| %.3g" % (name, np.median(bound[name][live] / np.abs(g[lo:hi][live]))))
    right = ipo.k1_backward(c53, c31, c3, p, stats, labels, mask, weight, ls, *acts)
    for name in ipo.BLOCK:
        lo, hi = off[name]
        assert (np.abs(right[name].reshape(-1) - g[lo:hi]) <= 1e-6 * bound[name] + 1e-300).all(), name
    for wrong in ipo.WRONG + ipo.WRONG_LOCAL:
        if wrong.startswith("drop_last") and n * h * w <= 64:
            continue  # (the ragged shape's variants: P = 90 is two whole 32-pixel tiles and one of 26)
        got = ipo.k1_backward(c53, c31, c3, p, stats, labels, mask, weight, ls, *acts, wrong=wrong)
        for name in CORRUPTS[wrong]:
            lo, hi = off[name]
            err = np.abs(got[name].reshape(-1) - g[lo:hi])
            over = err > bound[name]
            print("%s %s: %d of %d entries beyond the bound, worst x%.3g"
                  % (wrong, name, int(over.sum()), over.size, (err / np.maximum(bound[name], 1e-300)).max()))
            assert over.any(), (wrong, name)
