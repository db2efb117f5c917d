"""Training of ICNet's output layer on the MI355X: the fused head gradient against the float64
oracle, elementwise; the loss against the forward op, bit for bit; determinism; Adam bit for bit against the float32
restatement; the images entry against the features entry; a short end-to-end run against its float64 restatement."""
import numpy as np
import pytest
import torch

import semanticsegmentationactivelearning_amd as ssal
from semanticsegmentationactivelearning_amd import _lib, inference
from semanticsegmentationactivelearning_amd import synthetic as syn
from semanticsegmentationactivelearning_amd.models.util import conv_ops as cops
from semanticsegmentationactivelearning_amd.tensortools import losses
from semanticsegmentationactivelearning_amd.training import ICNetHeadTrainer

import icnet_head_train_oracle as iho
from helpers import frames

pytestmark = pytest.mark.gpu


def _case(seed, n, h, w, k):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, h, w, 128)) * 0.7).astype(np.float32)
    head = np.concatenate([rng.uniform(-0.3, 0.3, 128 * k), rng.uniform(-0.5, 0.5, k)]).astype(np.float32)
    labels = rng.integers(0, k, (n, 8 * h, 8 * w)).astype(np.uint8)
    mask = (rng.uniform(size=labels.shape) > 0.25).astype(np.float32)
    labels[(rng.uniform(size=labels.shape) < 0.3) & (mask == 0)] = 255  # ignored pixels: label 255 under mask 0
    labels[0, 0, 0], mask[0, 0, 0] = k, 1.0                             # a label >= K under mask 1: the all-off row
    labels[-1, -1, -1], mask[-1, -1, -1] = 0, 1.0
    return x, head, labels, mask


def _net(k):
    net = ssal.ICNet(k)
    net.build((None, None, None, 3))
    return net


_NETS = {}


def _shared_net(k):
    """one model per class count for the gradient cases (they pass the head as ``params`` and change nothing)"""
    if k not in _NETS:
        _NETS[k] = _net(k)
    return _NETS[k]


def _params(head, k):
    return {"conv6_cls.kernel": head[:128 * k].reshape(1, 1, 128, k), "conv6_cls.bias": head[128 * k:]}


def _pack(gd):
    return np.concatenate([gd["conv6_cls.kernel"].cpu().numpy().reshape(-1), gd["conv6_cls.bias"].cpu().numpy()])


def _forward_logits(x, head, k):
    """the logits the forward path computes from the same head: its fused 2x + 1x1 launch, then its 4x resize"""
    lq = cops.conv_bn_act(torch.as_tensor(x).cuda(), head[:128 * k].reshape(1, 1, 128, k), bias=head[128 * k:], relu=False,
                          upsample2x=True)
    return inference.resize_bilinear(lq, (4 * lq.shape[1], 4 * lq.shape[2]))


# N x h8 x w8 (the tile is 8 x 8 pixels of lq = 4 x 4 of sub12_sum), max_workgroups
SHAPES = [((1, 1, 1), 0),   # lq 2 x 2: every +1 tap is clamped
          ((2, 3, 5), 0),   # two tiles across, both partial, two images
          ((1, 5, 3), 0),   # a vertical tile boundary
          ((1, 3, 9), 1),   # three tiles in one workgroup
          ((1, 3, 9), 2)]   # ... in two: the fold
CASES = [(s, mw, k, wl) for s, mw in SHAPES for k in (2, 19, 32) for wl in ((0.0, 0.0), (1.02, 0.1))]


def _check_gradient(k, x, head, labels, mask, weight, ls, mw):
    n, h, w, _ = x.shape
    shape = (n, h, w)
    tr = ICNetHeadTrainer(_shared_net(k), 1e-3, loginverse_scaling=weight, label_smoothing=ls)
    xd = torch.as_tensor(x).cuda()
    loss, gd = tr.gradient_features(xd, labels, mask, params=_params(head, k), max_workgroups=mw)
    loss2, gd2 = tr.gradient_features(xd, labels, mask, params=_params(head, k), max_workgroups=mw)
    logits = _forward_logits(x, head, k)
    want = losses.masked_softmax_cross_entropy(torch.as_tensor(labels).cuda(), logits, torch.as_tensor(mask).cuda(), k,
                                               weight, ls)
    torch.cuda.synchronize()
    g = _pack(gd)
    assert np.array_equal(g, _pack(gd2)) and torch.equal(loss, loss2), "two calls differ"
    print("loss: forward op %.17g, gradient kernel %.17g" % (float(want), float(loss[0])))
    assert float(loss[0]) == float(want)
    g64, c, loss64 = iho.grad_and_bound(x, head, labels, mask, weight, ls, logits.cpu().numpy())
    kap = iho.kappa(n, h, w, k, weight, mw)
    bound = kap * 2.0 ** -24 * c
    d = np.abs(g.astype(np.float64) - g64)
    s = 128 * k
    for name, sl in (("kernel", slice(0, s)), ("bias", slice(s, None))):
        print("%s K=%d w=%g ls=%g %s mw=%d: kappa %.0f, max |g - g64| %.3e, max |g - g64| / bound %.3e, max |g64| %.3e"
              % (name, k, weight, ls, shape, mw, kap, d[sl].max(), (d[sl] / np.maximum(bound[sl], 1e-300)).max(),
                 np.abs(g64[sl]).max()))
    bad = d > bound
    assert not bad.any(), "%d of %d entries beyond kappa 2^-24 C (first at %d)" % (int(bad.sum()), bad.size,
                                                                                   int(np.argwhere(bad)[0]))
    assert abs(float(loss[0]) - loss64) <= 1e-5 * abs(loss64)
    return gd


@pytest.mark.parametrize("shape,mw,k,wl", CASES)
def test_gradient_loss_and_determinism(shape, mw, k, wl):
    """|g - g64| <= kappa 2^-24 C_j for every entry of dKernel and dBias; the loss bit-identical to the forward op on the
    forward path's logits; two calls give the same bits"""
    n, h, w = shape
    x, head, labels, mask = _case(1000 + CASES.index((shape, mw, k, wl)), n, h, w, k)
    _check_gradient(k, x, head, labels, mask, wl[0], wl[1], mw)


def test_adam_three_steps_bit_identical_to_float32_restatement():
    k = 19
    x, head, labels, mask = _case(11, 2, 3, 5, k)
    head[:3 * k] = 0.0  # exact zeros: sign(0) = 0
    net = _net(k)
    net.conv6_cls.kernel.assign(head[:128 * k].reshape(1, 1, 128, k))
    net.conv6_cls.bias.assign(head[128 * k:])
    tr = ICNetHeadTrainer(net, 5e-4, 0.9, 0.99, l1=1e-4, l2=2e-4, loginverse_scaling=1.02, learning_rate_decay=0.5,
                          decay_steps=4)
    xd = torch.as_tensor(x).cuda()
    w, m, v = head.copy(), np.zeros_like(head), np.zeros_like(head)
    b1p, b2p = np.float32(0.9), np.float32(0.99)
    for step in range(3):
        _, gd = tr.gradient_features(xd, labels, mask)
        lr = tr.current_learning_rate()
        tr.step_features(xd, labels, mask)
        w, m, v = iho.adam_head(w, m, v, _pack(gd), k, lr, 0.9, 0.99, 1e-8, b1p, b2p, l1=1e-4, l2=2e-4)
        b1p, b2p = np.float32(b1p * np.float32(0.9)), np.float32(b2p * np.float32(0.99))
        st = tr.state
        got = np.concatenate([net.conv6_cls.kernel.numpy().reshape(-1), net.conv6_cls.bias.numpy()])
        gm = np.concatenate([st["m"]["conv6_cls.kernel"].reshape(-1), st["m"]["conv6_cls.bias"]])
        gv = np.concatenate([st["v"]["conv6_cls.kernel"].reshape(-1), st["v"]["conv6_cls.bias"]])
        assert np.array_equal(gm, m), "m differs at step %d" % step
        assert np.array_equal(gv, v), "v differs at step %d" % step
        assert np.array_equal(got, w), "kernel / bias differ at step %d" % step
    assert tr.state["t"] == 3


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


def _head(net):
    return net.conv6_cls.kernel.numpy().copy(), net.conv6_cls.bias.numpy().copy()


@pytest.mark.parametrize("u8", [False, True])
def test_step_from_frames_equals_step_from_features_and_the_model_sees_the_head(icnet19, u8):
    from oracle import icnet_oracle as ico
    net0 = icnet19
    net = _net(19)
    net.assign_named({v.name: v.numpy() for v in net0.variables})
    x = syn.synth_frames_device(3, 2, 64, 128, 3, dtype=torch.uint8 if u8 else None)
    labels, mask = _targets()
    tr = ICNetHeadTrainer(net, 5e-4, 0.9, 0.99, loginverse_scaling=1.02, label_smoothing=0.1, l2=2e-4)
    feats = tr.features(x)
    assert tuple(feats.shape) == (2, 8, 16, 128)
    tr.reinitialize(seed=4)
    la = [float(tr.step(x, labels, mask)) for _ in range(2)]
    ka, ba = _head(net)
    tr.reinitialize(seed=4)
    lb = [float(tr.step_features(feats, labels, mask)) for _ in range(2)]
    kb, bb = _head(net)
    assert la == lb, "step(images) losses %r != step_features losses %r" % (la, lb)
    assert np.array_equal(ka, kb) and np.array_equal(ba, bb)
    assert tr.state["t"] == 2
    # the model and its handle see the trained head: logits bit-identical to the C oracle's forward, labels likewise
    tr.step(x, labels, mask)
    P = syn.icnet_params_dict(net)
    assert np.array_equal(P["conv6_cls.kernel"], net.conv6_cls.kernel.numpy())
    x_host = frames([3, 4], 64, 128, 3)
    want_logits = ico.icnet_forward(P, x_host)
    _, _, want_label, _ = ico.score_images(P, x_host, "margin")
    _, ex = net.score(x, return_label=True)
    logits = net(x, training=False)
    torch.cuda.synchronize()
    assert np.array_equal(logits.cpu().numpy(), want_logits)
    assert np.array_equal(ex["label"].cpu().numpy(), want_label)


def test_end_to_end_reinitialized_head_learns_as_its_float64_restatement(icnet19):
    """labels from the original head's argmax, reinitialize(0), 50 steps at the reference's settings
    (conf/enet_cityscapes_active_learning.json): the loss falls, and final / first is within 0.01 of the same ratio of the
    float64 restatement of the 50-step loop run on the CPU from the GPU's features (fp32 Adam departs from float64 in the
    seventh digit per step)"""
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
    tr = ICNetHeadTrainer.from_params(net, params)
    feats = tr.features(x)
    tr.reinitialize(seed=0)
    head0 = np.concatenate([a.reshape(-1) for a in _head(net)])
    got = [float(tr.step(x, labels, mask)) for _ in range(50)]
    want = iho.train_float64(feats.cpu().numpy(), head0, labels.cpu().numpy(), mask.cpu().numpy(), 19, 50, 0.0005, 0.9,
                             0.99, 1e-8, 1.02, 0.0, 0.0002)
    r, r64 = got[-1] / got[0], want[-1] / want[0]
    print("end to end: loss %.6g -> %.6g (x%.6f); float64 restatement %.6g -> %.6g (x%.6f)"
          % (got[0], got[-1], r, want[0], want[-1], r64))
    assert got[-1] < got[0]
    assert abs(r - r64) <= 0.01
