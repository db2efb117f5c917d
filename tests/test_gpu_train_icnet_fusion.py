"""Training of ICNet's last fusion stage on the MI355X: all eight gradients against the float64
oracle, elementwise; the conv6_cls gradients and the loss against ``ICNetHeadTrainer`` on the forward path's ``sub12_sum``,
bit for bit; determinism; dead channels; Adam bit for bit against the float32 restatement; the images entry against the
features entry and the model's handle after training; a short end-to-end run against its float64 restatement."""
import numpy as np
import pytest
import torch

import semanticsegmentationactivelearning_amd as ssal
from semanticsegmentationactivelearning_amd import inference
from semanticsegmentationactivelearning_amd import synthetic as syn
from semanticsegmentationactivelearning_amd.models.util import conv_ops as cops
from semanticsegmentationactivelearning_amd.training import ICNetFusionTrainer, ICNetHeadTrainer

import icnet_fusion_train_oracle as ifo
from helpers import frames

pytestmark = pytest.mark.gpu

STAT_NAMES = ("conv_sub2.mean", "conv_sub2.variance", "conv3_sub1_proj.mean", "conv3_sub1_proj.variance")


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
        rng = np.random.default_rng(77 + k)
        for name in STAT_NAMES:
            _var(net, name).assign((rng.uniform(0.5, 2.0, 128) if name.endswith("variance")
                                    else rng.uniform(-0.3, 0.3, 128)).astype(np.float32))
        _NETS[k] = net
    return _NETS[k]


def _stats(net):
    return np.concatenate([_var(net, n).numpy() for n in STAT_NAMES])


def _case(seed, n, h, w, k):
    rng = np.random.default_rng(seed)
    s24 = (rng.standard_normal((n, h, w, 128)) * 0.7).astype(np.float32)
    c3 = (rng.standard_normal((n, 2 * h, 2 * w, 64)) * 0.7).astype(np.float32)
    d = {"conv_sub2.kernel": rng.uniform(-0.04, 0.04, (3, 3, 128, 128)), "conv_sub2.gamma": rng.uniform(0.5, 1.5, 128),
         "conv_sub2.beta": rng.uniform(-0.3, 0.3, 128), "conv3_sub1_proj.kernel": rng.uniform(-0.15, 0.15, (1, 1, 64, 128)),
         "conv3_sub1_proj.gamma": rng.uniform(-1.5, 1.5, 128), "conv3_sub1_proj.beta": rng.uniform(-0.3, 0.3, 128),
         "conv6_cls.kernel": rng.uniform(-0.3, 0.3, (1, 1, 128, k)), "conv6_cls.bias": rng.uniform(-0.5, 0.5, k)}
    d = {name: v.astype(np.float32) for name, v in d.items()}
    labels = rng.integers(0, k, (n, 16 * h, 16 * w)).astype(np.uint8)
    mask = (rng.uniform(size=labels.shape) > 0.25).astype(np.float32)
    labels[(rng.uniform(size=labels.shape) < 0.3) & (mask == 0)] = 255  # ignored pixels: label 255 under mask 0
    labels[0, 0, 0], mask[0, 0, 0] = k, 1.0                             # a label >= K under mask 1: the all-off row
    labels[-1, -1, -1], mask[-1, -1, -1] = 0, 1.0
    return s24, c3, d, labels, mask


def _forward(net, s24, c3, d):
    """(sub12_sum, full-resolution logits) as the forward path's own operators compute them from the same weights"""
    bn = lambda layer: (_var(net, layer + ".mean").numpy(), _var(net, layer + ".variance").numpy(), d[layer + ".gamma"],
                        d[layer + ".beta"])
    proj = cops.conv_bn_act(torch.as_tensor(c3).cuda(), d["conv3_sub1_proj.kernel"], bn=bn("conv3_sub1_proj"), relu=False)
    sub12 = cops.conv_bn_act(torch.as_tensor(s24).cuda(), d["conv_sub2.kernel"], dilation=2, bn=bn("conv_sub2"),
                             residual=proj, relu=True, upsample2x=True)
    lq = cops.conv_bn_act(sub12, d["conv6_cls.kernel"], bias=d["conv6_cls.bias"], relu=False, upsample2x=True)
    return sub12, inference.resize_bilinear(lq, (4 * lq.shape[1], 4 * lq.shape[2]))


def _pack(gd):
    return np.concatenate([gd[n].cpu().numpy().reshape(-1) for n in ifo.NAMES])


def _check_gradient(net, k, s24, c3, d, labels, mask, weight, ls, mw, tag):
    n, h, w, _ = s24.shape
    tr = ICNetFusionTrainer(net, 1e-3, loginverse_scaling=weight, label_smoothing=ls)
    a, b = torch.as_tensor(s24).cuda(), torch.as_tensor(c3).cuda()
    loss, gd = tr.gradient_features(a, b, labels, mask, params=d, max_workgroups=mw)
    loss2, gd2 = tr.gradient_features(a, b, labels, mask, params=d, max_workgroups=mw)
    sub12, logits = _forward(net, s24, c3, d)
    head = ICNetHeadTrainer(net, 1e-3, loginverse_scaling=weight, label_smoothing=ls)
    hloss, hgd = head.gradient_features(sub12, labels, mask, params={n_: d[n_] for n_ in ifo.NAMES[6:]}, max_workgroups=mw)
    torch.cuda.synchronize()
    g = _pack(gd)
    assert np.array_equal(g, _pack(gd2)) and torch.equal(loss, loss2), "two calls differ"
    # conv6_cls and the loss: the bits of the head trainer on the forward path's sub12_sum
    assert torch.equal(loss, hloss), "loss %.17g != head trainer's %.17g" % (float(loss[0]), float(hloss[0]))
    for name in ifo.NAMES[6:]:
        assert torch.equal(gd[name], hgd[name]), name
    g64, c, loss64 = ifo.grad_and_bound(s24, c3, ifo.pack(d), _stats(net), labels, mask, weight, ls, sub12.cpu().numpy(),
                                        logits.cpu().numpy())
    dlt = np.abs(g.astype(np.float64) - g64)
    bad = []
    for name, (lo, hi) in ifo.offsets(k).items():
        kap = ifo.kappa(name, n, h, w, k, weight, mw)
        bound = kap * 2.0 ** -24 * c[lo:hi]
        ratio = (dlt[lo:hi] / np.maximum(bound, 1e-300)).max()
        print("%s %s: kappa %.0f, max |g - g64| %.3e, max |g - g64| / bound %.3e, max |g64| %.3e"
              % (tag, name, kap, dlt[lo:hi].max(), ratio, np.abs(g64[lo:hi]).max()))
        if (dlt[lo:hi] > bound).any():
            bad.append((name, int((dlt[lo:hi] > bound).sum()), float(ratio)))
    assert not bad, "entries beyond kappa 2^-24 C: %r" % (bad,)
    assert abs(float(loss[0]) - loss64) <= 1e-5 * abs(loss64)
    return gd, g64


# N x h16 x w16 (the weight-gradient kernel's tile is 4 x 8 pixels of sub12_sum = 2 x 4 of sub24_sum)
SHAPES = [(1, 1, 1),   # h8 = w8 = 2: every off-centre dilated tap is padding
          (2, 2, 3),
          (1, 3, 2),
          (1, 3, 5)]   # h8 x w8 = 6 x 10: the smallest that crosses a tile edge in both directions
CASES = [(s, mw, k, wl) for s in SHAPES for mw in (1, 2) for k in (2, 19, 32) for wl in ((0.0, 0.0), (1.02, 0.1))]


@pytest.mark.parametrize("shape,mw,k,wl", CASES)
def test_gradients_bits_and_determinism(shape, mw, k, wl):
    """|g - g64| <= kappa 2^-24 C_j for every entry of all eight gradients; conv6_cls' gradients and the loss bit-identical
    to ICNetHeadTrainer on the forward path's sub12_sum; two calls give the same bits"""
    n, h, w = shape
    s24, c3, d, labels, mask = _case(2000 + CASES.index((shape, mw, k, wl)), n, h, w, k)
    _check_gradient(_shared_net(k), k, s24, c3, d, labels, mask, wl[0], wl[1], mw,
                    "K=%d w=%g ls=%g %s mw=%d" % (k, wl[0], wl[1], shape, mw))


@pytest.mark.parametrize("mw", [1, 2])
def test_dead_channels(mw):
    """a beta that drives channels 0..4 of sub12_sum to exactly 0 everywhere and a gamma of 0: relu'(0) = 0, a zero scale
    passes no kernel gradient and still gets its own"""
    k = 19
    s24, c3, d, labels, mask = _case(31, 2, 2, 3, k)
    d["conv_sub2.beta"][:5] = -1e4
    d["conv3_sub1_proj.beta"][:5] = -1e4
    d["conv_sub2.gamma"][7] = 0.0
    d["conv3_sub1_proj.gamma"][9] = 0.0
    net = _shared_net(k)
    sub12, _ = _forward(net, s24, c3, d)
    assert not sub12[..., :5].any() and sub12[..., 5:].any()
    gd, g64 = _check_gradient(net, k, s24, c3, d, labels, mask, 1.02, 0.1, mw, "dead channels mw=%d" % mw)
    for name in ifo.NAMES[:6]:
        assert not gd[name][..., :5].any(), name
    assert not gd["conv6_cls.kernel"][0, 0, :5].any()
    assert not gd["conv_sub2.kernel"][..., 7].any() and float(gd["conv_sub2.gamma"][7]) != 0.0
    assert not gd["conv3_sub1_proj.kernel"][..., 9].any() and float(gd["conv3_sub1_proj.gamma"][9]) != 0.0
    assert not ifo.unpack(g64)["conv_sub2.kernel"][..., 7].any()


def _assign(net, d):
    for name, v in d.items():
        _var(net, name).assign(v)


def _host(net):
    return np.concatenate([_var(net, n).numpy().reshape(-1) for n in ifo.NAMES])


def test_adam_three_steps_bit_identical_to_float32_restatement():
    k = 19
    s24, c3, d, labels, mask = _case(11, 2, 2, 3, k)
    d["conv_sub2.kernel"][0, 0, :3] = 0.0  # exact zeros: sign(0) = 0
    net = _net(k)
    for name, v in zip(STAT_NAMES, np.split(_stats(_shared_net(k)), 4)):
        _var(net, name).assign(v)
    _assign(net, d)
    tr = ICNetFusionTrainer(net, 5e-4, 0.9, 0.99, l1=1e-4, l2=2e-4, loginverse_scaling=1.02, learning_rate_decay=0.5,
                            decay_steps=4)
    a, b = torch.as_tensor(s24).cuda(), torch.as_tensor(c3).cuda()
    w = ifo.pack(d).astype(np.float32)
    m, v = np.zeros_like(w), np.zeros_like(w)
    b1p, b2p = np.float32(0.9), np.float32(0.99)
    for step in range(3):
        _, gd = tr.gradient_features(a, b, labels, mask)
        lr = tr.current_learning_rate()
        tr.step_features(a, b, labels, mask)
        w, m, v = ifo.adam_fusion(w, m, v, _pack(gd), k, lr, 0.9, 0.99, 1e-8, b1p, b2p, l1=1e-4, l2=2e-4)
        b1p, b2p = np.float32(b1p * np.float32(0.9)), np.float32(b2p * np.float32(0.99))
        st = tr.state
        assert np.array_equal(ifo.pack(st["m"]), m), "m differs at step %d" % step
        assert np.array_equal(ifo.pack(st["v"]), v), "v differs at step %d" % step
        assert np.array_equal(_host(net), w), "weights differ at step %d" % step
    assert tr.state["t"] == 3
    # the regulariser reached the three kernels only: a zero gradient moves gamma / beta / bias by Adam alone
    z = np.zeros_like(w)
    _, m1, _ = ifo.adam_fusion(w, z, z, z, k, 5e-4, 0.9, 0.99, 1e-8, b1p, b2p, l1=1e-4, l2=2e-4)
    for name, (lo, hi) in ifo.offsets(k).items():
        assert bool(m1[lo:hi].any()) == (name in ifo.KERNELS), name


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
    from oracle import icnet_oracle as ico
    net = _net(19)
    net.assign_named({v.name: v.numpy() for v in icnet19.variables})
    start = {n: _var(net, n).numpy().copy() for n in ifo.NAMES}
    x = syn.synth_frames_device(3, 2, 64, 128, 3, dtype=torch.uint8 if u8 else None)
    labels, mask = _targets()
    tr = ICNetFusionTrainer(net, 5e-4, 0.9, 0.99, loginverse_scaling=1.02, label_smoothing=0.1, l2=2e-4)
    s24, c3 = tr.features(x)
    assert tuple(s24.shape) == (2, 4, 8, 128) and tuple(c3.shape) == (2, 8, 16, 64)
    tr.reinitialize(seed=4)
    la = [float(tr.step(x, labels, mask)) for _ in range(2)]
    wa = _host(net)
    _assign(net, {n: start[n] for n in ifo.NAMES[:6]})
    tr.reinitialize(seed=4)
    lb = [float(tr.step_features(s24, c3, labels, mask)) for _ in range(2)]
    wb = _host(net)
    assert la == lb, "step(images) losses %r != step_features losses %r" % (la, lb)
    assert np.array_equal(wa, wb)
    assert tr.state["t"] == 2
    # the model and its handle see the trained weights: logits bit-identical to the C oracle's forward, labels likewise
    tr.step(x, labels, mask)
    P = syn.icnet_params_dict(net)
    assert np.array_equal(P["conv_sub2.kernel"], net.conv_sub2.kernel.numpy())
    assert not np.array_equal(start["conv_sub2.kernel"], net.conv_sub2.kernel.numpy())
    x_host = frames([3, 4], 64, 128, 3)
    want_logits = ico.icnet_forward(P, x_host)
    _, _, want_label, _ = ico.score_images(P, x_host, "margin")
    _, ex = net.score(x, return_label=True)
    logits = net(x, training=False)
    torch.cuda.synchronize()
    assert np.array_equal(logits.cpu().numpy(), want_logits)
    assert np.array_equal(ex["label"].cpu().numpy(), want_label)


def test_end_to_end_learns_as_its_float64_restatement(icnet19):
    """section 23's 50-step run (same seed, labels and hyper-parameters) on cached features: the loss falls, and final / first
    is within 0.01 of the same ratio of the float64 restatement of the loop (section 23's margin).  The head-only trainer
    reached x0.225188 there; no ordering between the two is asserted."""
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
    tr = ICNetFusionTrainer.from_params(net, params)
    s24, c3 = tr.features(x)
    tr.reinitialize(seed=0)
    w0 = _host(net)
    got = [float(tr.step_features(s24, c3, labels, mask)) for _ in range(50)]
    want = ifo.train_float64(s24.cpu().numpy(), c3.cpu().numpy(), w0, _stats(net), labels.cpu().numpy(), mask.cpu().numpy(),
                             19, 50, 0.0005, 0.9, 0.99, 1e-8, 1.02, 0.0, 0.0002)
    r, r64 = got[-1] / got[0], want[-1] / want[0]
    print("end to end: loss %.6g -> %.6g (x%.6f); float64 restatement %.6g -> %.6g (x%.6f); head only: x0.225188"
          % (got[0], got[-1], r, want[0], want[-1], r64))
    assert got[-1] < got[0]
    assert abs(r - r64) <= 0.01
