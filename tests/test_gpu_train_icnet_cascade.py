"""Training of ICNet's whole cascade head on the MI355X: all fourteen gradients against the float64
oracle, elementwise; the loss and the fusion trainer's eight gradients against ``ICNetFusionTrainer`` on the forward path's
``sub24_sum``, bit for bit; determinism; dead channels; Adam bit for bit against the float32 restatement; the images entry
against the features entry and the model's handle after training; a short end-to-end run against its float64 restatement."""
import numpy as np
import pytest
import torch

import semanticsegmentationactivelearning_amd as ssal
from semanticsegmentationactivelearning_amd import inference
from semanticsegmentationactivelearning_amd import synthetic as syn
from semanticsegmentationactivelearning_amd.models.util import conv_ops as cops
from semanticsegmentationactivelearning_amd.training import ICNetCascadeTrainer, ICNetFusionTrainer

import icnet_cascade_train_oracle as ico
import icnet_fusion_train_oracle as ifo
from helpers import frames

pytestmark = pytest.mark.gpu

STAT_NAMES = ("conv_sub4.mean", "conv_sub4.variance", "conv3_1_sub2_proj.mean", "conv3_1_sub2_proj.variance",
              "conv_sub2.mean", "conv_sub2.variance", "conv3_sub1_proj.mean", "conv3_sub1_proj.variance")


def _var(net, name):
    layer, attr = name.split(".")
    return getattr(getattr(net, layer), attr)


def _net(k):
    net = ssal.ICNet(k)
    net.build((None, None, None, 3))
    return net


_NETS = {}


def _shared_net(k):
    """one model per class count for the gradient cases (they pass the weights as ``params`` and change nothing); its moving
    statistics are drawn once"""
    if k not in _NETS:
        net = _net(k)
        rng = np.random.default_rng(177 + k)
        for name in STAT_NAMES:
            _var(net, name).assign((rng.uniform(0.5, 2.0, 128) if name.endswith("variance")
                                    else rng.uniform(-0.3, 0.3, 128)).astype(np.float32))
        _NETS[k] = net
    return _NETS[k]


def _stats(net):
    return np.concatenate([_var(net, n).numpy() for n in STAT_NAMES])


def _case(seed, n, h, w, k):
    rng = np.random.default_rng(seed)
    c54 = (rng.standard_normal((n, h, w, 256)) * 0.7).astype(np.float32)
    c31 = (rng.standard_normal((n, 2 * h, 2 * w, 256)) * 0.7).astype(np.float32)
    c3 = (rng.standard_normal((n, 4 * h, 4 * w, 64)) * 0.7).astype(np.float32)
    d = {"conv_sub4.kernel": rng.uniform(-0.03, 0.03, (3, 3, 256, 128)), "conv_sub4.gamma": rng.uniform(0.5, 1.5, 128),
         "conv_sub4.beta": rng.uniform(-0.3, 0.3, 128), "conv3_1_sub2_proj.kernel": rng.uniform(-0.08, 0.08, (1, 1, 256, 128)),
         "conv3_1_sub2_proj.gamma": rng.uniform(-1.5, 1.5, 128), "conv3_1_sub2_proj.beta": rng.uniform(-0.3, 0.3, 128),
         "conv_sub2.kernel": rng.uniform(-0.04, 0.04, (3, 3, 128, 128)), "conv_sub2.gamma": rng.uniform(0.5, 1.5, 128),
         "conv_sub2.beta": rng.uniform(-0.3, 0.3, 128), "conv3_sub1_proj.kernel": rng.uniform(-0.15, 0.15, (1, 1, 64, 128)),
         "conv3_sub1_proj.gamma": rng.uniform(-1.5, 1.5, 128), "conv3_sub1_proj.beta": rng.uniform(-0.3, 0.3, 128),
         "conv6_cls.kernel": rng.uniform(-0.3, 0.3, (1, 1, 128, k)), "conv6_cls.bias": rng.uniform(-0.5, 0.5, k)}
    d = {name: v.astype(np.float32) for name, v in d.items()}
    labels = rng.integers(0, k, (n, 32 * h, 32 * w)).astype(np.uint8)
    mask = (rng.uniform(size=labels.shape) > 0.25).astype(np.float32)
    labels[(rng.uniform(size=labels.shape) < 0.3) & (mask == 0)] = 255  # ignored pixels: label 255 under mask 0
    labels[0, 0, 0], mask[0, 0, 0] = k, 1.0                             # a label >= K under mask 1: the all-off row
    labels[-1, -1, -1], mask[-1, -1, -1] = 0, 1.0
    return c54, c31, c3, d, labels, mask


def _forward(net, c54, c31, c3, d):
    """(sub24_sum, sub12_sum, full-resolution logits) as the forward path's own operators compute them from the same weights"""
    bn = lambda layer: (_var(net, layer + ".mean").numpy(), _var(net, layer + ".variance").numpy(), d[layer + ".gamma"],
                        d[layer + ".beta"])
    p24 = cops.conv_bn_act(torch.as_tensor(c31).cuda(), d["conv3_1_sub2_proj.kernel"], bn=bn("conv3_1_sub2_proj"), relu=False)
    sub24 = cops.conv_bn_act(torch.as_tensor(c54).cuda(), d["conv_sub4.kernel"], dilation=2, bn=bn("conv_sub4"), residual=p24,
                             relu=True, upsample2x=True)
    proj = cops.conv_bn_act(torch.as_tensor(c3).cuda(), d["conv3_sub1_proj.kernel"], bn=bn("conv3_sub1_proj"), relu=False)
    sub12 = cops.conv_bn_act(sub24, d["conv_sub2.kernel"], dilation=2, bn=bn("conv_sub2"), residual=proj, relu=True,
                             upsample2x=True)
    lq = cops.conv_bn_act(sub12, d["conv6_cls.kernel"], bias=d["conv6_cls.bias"], relu=False, upsample2x=True)
    return sub24, sub12, inference.resize_bilinear(lq, (4 * lq.shape[1], 4 * lq.shape[2]))


def _pack(gd):
    return np.concatenate([gd[n].cpu().numpy().reshape(-1) for n in ico.NAMES])


def _check_gradient(net, k, c54, c31, c3, d, labels, mask, weight, ls, mw, tag):
    n, h, w, _ = c54.shape
    tr = ICNetCascadeTrainer(net, 1e-3, loginverse_scaling=weight, label_smoothing=ls)
    dev = [torch.as_tensor(a).cuda() for a in (c54, c31, c3)]
    loss, gd = tr.gradient_features(*dev, labels, mask, params=d, max_workgroups=mw)
    loss2, gd2 = tr.gradient_features(*dev, labels, mask, params=d, max_workgroups=mw)
    sub24, sub12, logits = _forward(net, c54, c31, c3, d)
    fus = ICNetFusionTrainer(net, 1e-3, loginverse_scaling=weight, label_smoothing=ls)
    floss, fgd = fus.gradient_features(sub24, dev[2], labels, mask, params={n_: d[n_] for n_ in ifo.NAMES}, max_workgroups=mw)
    torch.cuda.synchronize()
    g = _pack(gd)
    assert np.array_equal(g, _pack(gd2)) and torch.equal(loss, loss2), "two calls differ"
    # the loss and the eight gradients of section 28: the bits of the fusion trainer on the forward path's sub24_sum
    assert torch.equal(loss, floss), "loss %.17g != fusion trainer's %.17g" % (float(loss[0]), float(floss[0]))
    for name in ifo.NAMES:
        assert torch.equal(gd[name], fgd[name]), name
    g64, c, loss64 = ico.grad_and_bound(c54, c31, c3, ico.pack(d), _stats(net), labels, mask, weight, ls,
                                        sub24.cpu().numpy(), sub12.cpu().numpy(), logits.cpu().numpy())
    dlt = np.abs(g.astype(np.float64) - g64)
    bad = []
    for name, (lo, hi) in ico.offsets(k).items():
        kap = ico.kappa(name, n, h, w, k, weight, mw)
        bound = kap * 2.0 ** -24 * c[lo:hi]
        ratio = (dlt[lo:hi] / np.maximum(bound, 1e-300)).max()
        print("%s %s: kappa %.0f, max |g - g64| %.3e, max |g - g64| / bound %.3e, max |g64| %.3e"
              % (tag, name, kap, dlt[lo:hi].max(), ratio, np.abs(g64[lo:hi]).max()))
        if (dlt[lo:hi] > bound).any():
            bad.append((name, int((dlt[lo:hi] > bound).sum()), float(ratio)))
    assert not bad, "entries beyond kappa 2^-24 C: %r" % (bad,)
    assert abs(float(loss[0]) - loss64) <= 1e-5 * abs(loss64)
    return gd, g64, sub24


# N x h32 x w32
SHAPES = [(1, 1, 1),   # h16 = 2: every off-centre tap of conv_sub4 is padding; h8 = 4
          (2, 2, 3),
          (1, 3, 2),
          (1, 3, 5)]   # h16 x w16 = 6 x 10 crosses the 4 x 8 tile edge both ways; h8 x w8 = 12 x 20 crosses the data-gradient
                       # kernel's 8 x 16 tile edges and meets the clamped last row and column
CASES = [(s, mw, k, wl) for s in SHAPES for mw in (1, 2) for k in (2, 19, 32) for wl in ((0.0, 0.0), (1.02, 0.1))]


@pytest.mark.parametrize("shape,mw,k,wl", CASES)
def test_gradients_bits_and_determinism(shape, mw, k, wl):
    """|g - g64| <= kappa 2^-24 C_j for every entry of all fourteen gradients; the loss and section 28's eight gradients
    bit-identical to ICNetFusionTrainer on the forward path's sub24_sum; two calls give the same bits"""
    n, h, w = shape
    c54, c31, c3, d, labels, mask = _case(3000 + CASES.index((shape, mw, k, wl)), n, h, w, k)
    _check_gradient(_shared_net(k), k, c54, c31, c3, d, labels, mask, wl[0], wl[1], mw,
                    "K=%d w=%g ls=%g %s mw=%d" % (k, wl[0], wl[1], shape, mw))


@pytest.mark.parametrize("mw", [1, 2])
def test_dead_channels(mw):
    """a beta that drives channels 0..4 of sub24_sum to exactly 0 everywhere and a gamma of 0 in each new branch: relu'(0) = 0
    (g24 is exactly 0 on dead units, so nothing of the block's gradients reaches them), a zero scale passes no kernel gradient
    and still gets its own"""
    k = 19
    c54, c31, c3, d, labels, mask = _case(41, 2, 2, 3, k)
    d["conv_sub4.beta"][:5] = -1e4
    d["conv3_1_sub2_proj.beta"][:5] = -1e4
    d["conv_sub4.gamma"][7] = 0.0
    d["conv3_1_sub2_proj.gamma"][9] = 0.0
    net = _shared_net(k)
    gd, g64, sub24 = _check_gradient(net, k, c54, c31, c3, d, labels, mask, 1.02, 0.1, mw, "dead channels mw=%d" % mw)
    assert not sub24[..., :5].any() and sub24[..., 5:].any()
    g64d = ico.unpack(g64)
    for name in ico.BLOCK:
        # every entry of these tensors along a dead output channel is a sum over pixels of g24 = 0 there: exactly 0, as the
        # oracle has it
        assert not gd[name][..., :5].any() and not g64d[name][..., :5].any(), name
    assert not gd["conv_sub2.kernel"][:, :, :5].any()  # sub24_sum's dead channels are conv_sub2's dead inputs
    assert not gd["conv_sub4.kernel"][..., 7].any() and float(gd["conv_sub4.gamma"][7]) != 0.0
    assert not gd["conv3_1_sub2_proj.kernel"][..., 9].any() and float(gd["conv3_1_sub2_proj.gamma"][9]) != 0.0
    assert not g64d["conv_sub4.kernel"][..., 7].any() and not g64d["conv3_1_sub2_proj.kernel"][..., 9].any()


def _assign(net, d):
    for name, v in d.items():
        _var(net, name).assign(v)


def _host(net):
    return np.concatenate([_var(net, n).numpy().reshape(-1) for n in ico.NAMES])


def test_adam_three_steps_bit_identical_to_float32_restatement():
    k = 19
    c54, c31, c3, d, labels, mask = _case(12, 2, 2, 3, k)
    d["conv_sub4.kernel"][0, 0, :3] = 0.0  # exact zeros: sign(0) = 0
    net = _net(k)
    for name, v in zip(STAT_NAMES, np.split(_stats(_shared_net(k)), 8)):
        _var(net, name).assign(v)
    _assign(net, d)
    tr = ICNetCascadeTrainer(net, 5e-4, 0.9, 0.99, l1=1e-4, l2=2e-4, loginverse_scaling=1.02, learning_rate_decay=0.5,
                             decay_steps=4)
    dev = [torch.as_tensor(a).cuda() for a in (c54, c31, c3)]
    w = ico.pack(d).astype(np.float32)
    m, v = np.zeros_like(w), np.zeros_like(w)
    b1p, b2p = np.float32(0.9), np.float32(0.99)
    for step in range(3):
        _, gd = tr.gradient_features(*dev, labels, mask)
        lr = tr.current_learning_rate()
        tr.step_features(*dev, labels, mask)
        w, m, v = ico.adam_cascade(w, m, v, _pack(gd), k, lr, 0.9, 0.99, 1e-8, b1p, b2p, l1=1e-4, l2=2e-4)
        b1p, b2p = np.float32(b1p * np.float32(0.9)), np.float32(b2p * np.float32(0.99))
        st = tr.state
        assert np.array_equal(ico.pack(st["m"]), m), "m differs at step %d" % step
        assert np.array_equal(ico.pack(st["v"]), v), "v differs at step %d" % step
        assert np.array_equal(_host(net), w), "weights differ at step %d" % step
    assert tr.state["t"] == 3
    # the regulariser reached the five kernels only: a zero gradient moves gamma / beta / bias by Adam alone
    z = np.zeros_like(w)
    _, m1, _ = ico.adam_cascade(w, z, z, z, k, 5e-4, 0.9, 0.99, 1e-8, b1p, b2p, l1=1e-4, l2=2e-4)
    for name, (lo, hi) in ico.offsets(k).items():
        assert bool(m1[lo:hi].any()) == (name in ico.KERNELS), name


@pytest.fixture(scope="module")
def icnet19():
    net = _net(19)
    syn.randomize_icnet(net, seed=0)
    return net


def _targets(seed=9):
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, 19, (2, 64, 128)).astype(np.uint8)
    labels[:, :4] = 255
    mask = (rng.uniform(size=(2, 64, 128)) > 0.2).astype(np.float32)
    mask[:, :4] = 0.0
    return labels, mask


@pytest.mark.parametrize("u8", [False, True])
def test_step_from_frames_equals_step_from_features_and_the_model_sees_the_weights(icnet19, u8):
    from oracle import icnet_oracle as icor
    net = _net(19)
    net.assign_named({v.name: v.numpy() for v in icnet19.variables})
    start = {n: _var(net, n).numpy().copy() for n in ico.NAMES}
    x = syn.synth_frames_device(3, 2, 64, 128, 3, dtype=torch.uint8 if u8 else None)
    labels, mask = _targets()
    tr = ICNetCascadeTrainer(net, 5e-4, 0.9, 0.99, loginverse_scaling=1.02, label_smoothing=0.1, l2=2e-4)
    feats = tr.features(x)
    assert [tuple(t.shape) for t in feats] == [(2, 2, 4, 256), (2, 4, 8, 256), (2, 8, 16, 64)]
    tr.reinitialize(seed=4)
    la = [float(tr.step(x, labels, mask)) for _ in range(2)]
    wa = _host(net)
    _assign(net, {n: start[n] for n in ico.NAMES[:12]})
    tr.reinitialize(seed=4)
    lb = [float(tr.step_features(*feats, labels, mask)) for _ in range(2)]
    wb = _host(net)
    assert la == lb, "step(images) losses %r != step_features losses %r" % (la, lb)
    assert np.array_equal(wa, wb)
    assert tr.state["t"] == 2
    # the model and its handle see the trained weights (ssal_icnet_update_cascade): logits bit-identical to the C oracle's
    # forward, labels likewise
    tr.step(x, labels, mask)
    P = syn.icnet_params_dict(net)
    for layer in ("conv_sub4", "conv3_1_sub2_proj", "conv_sub2"):
        assert np.array_equal(P[layer + ".kernel"], _var(net, layer + ".kernel").numpy())
        assert not np.array_equal(start[layer + ".kernel"], _var(net, layer + ".kernel").numpy())
    x_host = frames([3, 4], 64, 128, 3)
    want_logits = icor.icnet_forward(P, x_host)
    _, _, want_label, _ = icor.score_images(P, x_host, "margin")
    _, ex = net.score(x, return_label=True)
    logits = net(x, training=False)
    torch.cuda.synchronize()
    assert np.array_equal(logits.cpu().numpy(), want_logits)
    assert np.array_equal(ex["label"].cpu().numpy(), want_label)


def test_end_to_end_learns_as_its_float64_restatement(icnet19):
    """section 23's 50-step run (same seed, labels and hyper-parameters) on cached features: the loss falls, and final / first
    is within 0.01 of the same ratio of the float64 restatement of the loop (section 23's margin).  The fusion trainer reached
    x0.003053 there; no ordering between the two is asserted."""
    net = _net(19)
    net.assign_named({v.name: v.numpy() for v in icnet19.variables})
    x = syn.synth_frames_device(0, 2, 64, 128, 3)
    _, extra = net.score(x, return_label=True)
    labels = extra["label"].clone()
    mask = torch.ones((2, 64, 128), dtype=torch.float32, device=x.device)
    params = {"hyperparams": {"learning_rate": 0.0005, "learning_rate_decay": 0.0,
                              "optimizer": {"type": "Adam", "kwargs": {"beta1": 0.9, "beta2": 0.99}},
                              "weight_reg": {"L2": 0.0002, "L1": 0.0},
                              "softmax": {"label_smoothing": 0.0, "loginverse_scaling": 1.02, "multiscale": False}}}
    tr = ICNetCascadeTrainer.from_params(net, params)
    feats = tr.features(x)
    tr.reinitialize(seed=0)
    w0 = _host(net)
    got = [float(tr.step_features(*feats, labels, mask)) for _ in range(50)]
    want = ico.train_float64(*(t.cpu().numpy() for t in feats), w0, _stats(net), labels.cpu().numpy(), mask.cpu().numpy(),
                             19, 50, 0.0005, 0.9, 0.99, 1e-8, 1.02, 0.0, 0.0002)
    r, r64 = got[-1] / got[0], want[-1] / want[0]
    print("end to end: loss %.6g -> %.6g (x%.6f); float64 restatement %.6g -> %.6g (x%.6f); fusion trainer: x0.003053"
          % (got[0], got[-1], r, want[0], want[-1], r64))
    assert got[-1] < got[0]
    assert abs(r - r64) <= 0.01
