"""Training of ICNet through ``conv5_2`` on the MI355X: all 35 gradients against the float64 oracle,
elementwise, on inputs of random sign and on sign-coherent ones where the bound is tight; the loss and the bottleneck trainer's
26 gradients against ``ICNetBottleneckTrainer`` on the forward path's ``conv5_2``, bit for bit; determinism; dead channels and an
exactly-zero ``conv5_2``; Adam bit for bit against the float32 restatement; the images entries against the features entries, the
truncated trunk against the unfused forward, and the model's handle after training; section 15's 50-step run next to the
bottleneck trainer's."""
import numpy as np
import pytest
import torch

from semanticsegmentationactivelearning_amd import synthetic as syn
from semanticsegmentationactivelearning_amd.models.util import conv_ops as cops
from semanticsegmentationactivelearning_amd.training import ICNetBottleneckTrainer, ICNetDeepBottleneckTrainer

import icnet_bneck2_train_oracle as b2
import icnet_bneck_train_oracle as bo
import test_gpu_train_icnet_bneck as tb
from helpers import frames
from test_gpu_train_icnet_pool import _assign, _net, _targets, _var

pytestmark = pytest.mark.gpu

STAT_NAMES = tuple("%s.%s" % (layer, attr) for layer in (b2.REDUCE, b2.CONV3, b2.INCREASE) for attr in ("mean", "variance")) \
    + tb.STAT_NAMES
STAT_SEED = 431
BLOCK_LAYERS = ("conv5_2_1x1_reduce", "conv5_2_3x3", "conv5_2", "conv5_3_1x1_reduce", "conv5_3_3x3", "conv5_3")


def _assign_stats(net, stats):
    lo = 0
    for name in STAT_NAMES:
        size = int(np.prod(_var(net, name).shape))
        _var(net, name).assign(stats[lo:lo + size])
        lo += size
    assert lo == len(stats)


_NETS = {}


def _shared_net(k):
    """one model per class count for the gradient cases (they pass the weights as ``params`` and change nothing); its moving
    statistics are ``b2.draw_stats(STAT_SEED)``"""
    if k not in _NETS:
        net = _net(k)
        _assign_stats(net, b2.draw_stats(STAT_SEED))
        _NETS[k] = net
    return _NETS[k]


def _stats(net):
    return np.concatenate([_var(net, n).numpy() for n in STAT_NAMES])


def _forward(net, x, c31, c3, d):
    """(conv5_2_1x1_reduce, conv5_2_3x3, conv5_2) and the bottleneck test's eight above them, as the forward path's own operators
    compute them from the same weights"""
    bn = lambda layer: (_var(net, layer + ".mean").numpy(), _var(net, layer + ".variance").numpy(), d[layer + ".gamma"],
                        d[layer + ".beta"])
    x51 = torch.as_tensor(x).cuda()
    r = cops.conv_bn_act(x51, d[b2.BLOCK_R[0]], bn=bn(b2.REDUCE), relu=True)
    a = cops.conv_bn_act(r, d[b2.BLOCK_3[0]], dilation=4, bn=bn(b2.CONV3), relu=True)
    c52 = cops.conv_bn_act(a, d[b2.BLOCK_I[0]], bn=bn(b2.INCREASE), residual=x51, relu=True)
    return (r, a, c52) + tuple(tb._forward(net, c52.cpu().numpy(), c31, c3, d))


def _pack(gd):
    return np.concatenate([gd[n].cpu().numpy().reshape(-1) for n in b2.NAMES])


_ORACLE = {}


def _oracle(key, net, x, c31, c3, d, labels, mask, weight, ls, acts):
    """the float64 gradient, its magnitude sums and the loss: they do not depend on ``max_workgroups``, so the cases that
    differ in it alone share one evaluation (``acts``, the fp32 forward values, do not depend on it either)"""
    if key not in _ORACLE:
        _ORACLE[key] = b2.grad_and_bound(x, c31, c3, b2.pack(d), _stats(net), labels, mask, weight, ls,
                                         tuple(t.cpu().numpy() for t in acts))
    return _ORACLE[key]


def _check_gradient(net, k, x, c31, c3, d, labels, mask, weight, ls, mw, tag, key):
    n, h, w, _ = x.shape
    tr = ICNetDeepBottleneckTrainer(net, 1e-3, loginverse_scaling=weight, label_smoothing=ls)
    dev = [torch.as_tensor(t).cuda() for t in (x, c31, c3)]
    loss, gd = tr.gradient_features(*dev, labels, mask, params=d, max_workgroups=mw)
    loss2, gd2 = tr.gradient_features(*dev, labels, mask, params=d, max_workgroups=mw)
    acts = _forward(net, x, c31, c3, d)
    up = ICNetBottleneckTrainer(net, 1e-3, loginverse_scaling=weight, label_smoothing=ls)
    uloss, ugd = up.gradient_features(acts[2], dev[1], dev[2], labels, mask, params={n_: d[n_] for n_ in bo.NAMES},
                                      max_workgroups=mw)
    torch.cuda.synchronize()
    g = _pack(gd)
    assert np.array_equal(g, _pack(gd2)) and torch.equal(loss, loss2), "two calls differ"
    # the loss and the 26 gradients of section 42: the bits of the bottleneck trainer on the forward path's conv5_2
    assert torch.equal(loss, uloss), "loss %.17g != bottleneck trainer's %.17g" % (float(loss[0]), float(uloss[0]))
    for name in bo.NAMES:
        assert torch.equal(gd[name], ugd[name]), name
    for i in (0, 1, 2):
        sign = acts[i].cpu().numpy() > 0
        assert sign.any() and not sign.all(), "the three new pre-activations must have both signs"
    g64, c, loss64 = _oracle(key, net, x, c31, c3, d, labels, mask, weight, ls, acts)
    dlt = np.abs(g.astype(np.float64) - g64)
    bad = []
    for name, (lo, hi) in b2.offsets(k).items():
        kap = b2.kappa(name, n, h, w, k, weight, mw)
        bound = kap * 2.0 ** -24 * c[lo:hi]
        ratio = (dlt[lo:hi] / np.maximum(bound, 1e-300)).max()
        print("%s %s: kappa %.0f, max |g - g64| %.3e, max |g - g64| / bound %.3e, max |g64| %.3e"
              % (tag, name, kap, dlt[lo:hi].max(), ratio, np.abs(g64[lo:hi]).max()))
        if (dlt[lo:hi] > bound).any():
            bad.append((name, int((dlt[lo:hi] > bound).sum()), float(ratio)))
    assert not bad, "entries beyond kappa 2^-24 C: %r" % (bad,)
    assert abs(float(loss[0]) - loss64) <= 1e-5 * abs(loss64)
    return gd, g64, acts


# N x h32 x w32: section 42's shapes.  The tiles: 64 pixels (linear) in the new kernel and in the increase layer's data gradient,
# 8 x 8 pixels of one image in the 3 x 3's, 32 pixels (linear) in the three weight gradients
SHAPES = [(1, 1, 1),    # only the centre tap lies inside the map
          (2, 2, 3),
          (1, 3, 9),    # taps at +-4 live on the long axis only
          (2, 5, 9),    # P = 90: the new kernel's last 64-pixel tile is ragged (64 + 26), and at max_workgroups = 2 the split-K
                        # groups take 2 and 1 tiles (a ragged last group)
          (1, 9, 10)]   # the centre pixels have all nine taps inside; 64 + 26 again
GROUPS = [(s, k, wl) for s in SHAPES for k in (2, 19) for wl in ((0.0, 0.0), (1.02, 0.1))]
CASES = [(s, mw, k, wl) for (s, k, wl) in GROUPS for mw in (0, 1, 2)]


@pytest.mark.parametrize("shape,mw,k,wl", CASES)
def test_gradients_bits_and_determinism(shape, mw, k, wl):
    """|g - g64| <= kappa 2^-24 C_j for every entry of all 35 gradients; the loss within 1e-5 of float64; the loss and section
    42's 26 gradients bit-identical to ICNetBottleneckTrainer on the forward path's conv5_2; two calls give the same bits"""
    n, h, w = shape
    key = GROUPS.index((shape, k, wl))
    x, c31, c3, d, labels, mask = b2.case(8000 + key, n, h, w, k)
    _check_gradient(_shared_net(k), k, x, c31, c3, d, labels, mask, wl[0], wl[1], mw,
                    "K=%d w=%g ls=%g %s mw=%d" % (k, wl[0], wl[1], shape, mw), key)


# the sign-coherent inputs (icnet_bneck2_train_oracle.coherent_case): tests/test_train_icnet_bneck2_cpu.py shows on these very
# arrays that the wrong backward passes leave the bound on every tensor they corrupt
COHERENT_SEED = 7
COHERENT = [(s, mw, k, wl) for s in ((2, 5, 9), (1, 9, 10)) for k, wl in ((2, (0.0, 0.0)), (19, (1.02, 0.1))) for mw in (0, 1, 2)]
_COHERENT = {}


@pytest.mark.parametrize("shape,mw,k,wl", COHERENT)
def test_gradients_on_sign_coherent_inputs(shape, mw, k, wl):
    """the same checks where the bound is tight: the CPU discrimination test's arrays"""
    n, h, w = shape
    if (shape, k) not in _COHERENT:
        arrays = b2.coherent_case(COHERENT_SEED, n, h, w, k)
        net = _net(k)
        _assign_stats(net, arrays[4])
        _COHERENT[(shape, k)] = (arrays, net)
    (x, c31, c3, d, stats, labels, mask), net = _COHERENT[(shape, k)]
    assert np.array_equal(_stats(net), stats)
    _check_gradient(net, k, x, c31, c3, d, labels, mask, wl[0], wl[1], mw,
                    "coherent K=%d w=%g %s mw=%d" % (k, wl[0], shape, mw), ("coherent", shape, k))


@pytest.mark.parametrize("mw", [0, 2])
def test_dead_channels(mw):
    """a beta of -1e4 on channels 0..4 of each new layer makes its output exactly 0 there: relu'(0) = 0, so the layer's three
    gradients along them are exactly 0, in the GPU result and in the oracle -- and so are the kernel gradients of the 3 x 3 and of
    the increase layer along their dead INPUT channels (a zero operand); a gamma of 0 passes no kernel gradient along its
    output and still gets its own"""
    k = 19
    x, c31, c3, d, labels, mask = b2.case(43, 2, 5, 9, k)
    x[..., :5] = 0.0  # (conv5_2 = relu(BN(..) + conv5_1): the shortcut must not revive the increase layer's dead channels)
    for blk in (b2.BLOCK_R, b2.BLOCK_3, b2.BLOCK_I):
        d[blk[2]][:5] = -1e4
        d[blk[1]][7] = 0.0
        d[blk[2]][7] = 0.2
    net = _shared_net(k)
    gd, g64, acts = _check_gradient(net, k, x, c31, c3, d, labels, mask, 1.02, 0.1, mw, "dead channels mw=%d" % mw, ("dead", mw))
    g64d = b2.unpack(g64)
    for i, blk in enumerate((b2.BLOCK_R, b2.BLOCK_3, b2.BLOCK_I)):
        act = acts[i].cpu().numpy()
        assert not act[..., :5].any() and act[..., 5:].any()
        for name in blk:
            assert not gd[name][..., :5].any() and not g64d[name][..., :5].any(), name
        assert not gd[blk[0]][..., 7].any() and float(gd[blk[1]][7]) != 0.0
        assert not g64d[blk[0]][..., 7].any() and float(g64d[blk[1]][7]) != 0.0
    for name in (b2.BLOCK_3[0], b2.BLOCK_I[0]):
        assert not gd[name][:, :, :5].any() and not g64d[name][:, :, :5].any(), name


def test_an_exactly_zero_conv5_2_gets_no_gradient():
    """conv5_2 == 0.0 exactly at every pixel of channels 0..2 (a zero shortcut under gamma = beta = 0: the pre-activation is
    fmaf(-mean, 0, 0) + 0) while conv5_3 is alive there and hands down a gradient: relu'(0) = 0, so the kernel's mask is `> 0` and
    not `>= 0` -- the increase layer's beta gradient, sum_p g52, is exactly 0 on those channels, as in the oracle; one channel
    more is 0 at the first and the last pixel only and stays inside the bound"""
    k = 19
    x, c31, c3, d, labels, mask = b2.case(47, 2, 5, 9, k)
    x[..., :4] = np.abs(x[..., :4]) + 0.1
    x[..., :3] = 0.0
    x[0, 0, 0, 3] = x[-1, -1, -1, 3] = 0.0
    d[b2.BLOCK_I[1]][:4] = 0.0
    d[b2.BLOCK_I[2]][:4] = 0.0
    d[bo.po.BLOCK[2]][:4] = 0.5  # conv5_3 = relu(BN(..) + conv5_2) alive on those channels: g53 is not masked away there
    net = _shared_net(k)
    gd, g64, acts = _check_gradient(net, k, x, c31, c3, d, labels, mask, 1.02, 0.1, 0, "zero conv5_2", ("zero", 0))
    c52, c53 = acts[2].cpu().numpy(), acts[5].cpu().numpy()
    assert not c52[..., :3].any() and c52[0, 0, 0, 3] == 0.0 and c52[-1, -1, -1, 3] == 0.0 and c52[..., 3].any()
    assert (c53[..., :3] > 0).any()
    g64d = b2.unpack(g64)
    assert not gd[b2.BLOCK_I[2]][:3].any() and not g64d[b2.BLOCK_I[2]][:3].any()
    assert float(gd[b2.BLOCK_I[2]][3]) != 0.0 and float(gd[b2.BLOCK_I[2]][5]) != 0.0


def _host(net):
    return np.concatenate([_var(net, n).numpy().reshape(-1) for n in b2.NAMES])


def test_adam_three_steps_bit_identical_to_float32_restatement():
    k = 19
    x, c31, c3, d, labels, mask = b2.case(12, 2, 2, 3, k)
    d[b2.BLOCK_3[0]][0, 0, 0, :3] = 0.0  # exact zeros: sign(0) = 0
    net = _net(k)
    _assign_stats(net, b2.draw_stats(STAT_SEED))
    _assign(net, d)
    tr = ICNetDeepBottleneckTrainer(net, 5e-4, 0.9, 0.99, l1=1e-4, l2=2e-4, loginverse_scaling=1.02, learning_rate_decay=0.5,
                                    decay_steps=4)
    dev = [torch.as_tensor(t).cuda() for t in (x, c31, c3)]
    w = b2.pack(d).astype(np.float32)
    m, v = np.zeros_like(w), np.zeros_like(w)
    b1p, b2p = np.float32(0.9), np.float32(0.99)
    for step in range(3):
        _, gd = tr.gradient_features(*dev, labels, mask)
        lr = tr.current_learning_rate()
        tr.step_features(*dev, labels, mask)
        w, m, v = b2.adam_bneck2(w, m, v, _pack(gd), k, lr, 0.9, 0.99, 1e-8, b1p, b2p, l1=1e-4, l2=2e-4)
        b1p, b2p = np.float32(b1p * np.float32(0.9)), np.float32(b2p * np.float32(0.99))
        st = tr.state
        assert np.array_equal(b2.pack(st["m"]), m), "m differs at step %d" % step
        assert np.array_equal(b2.pack(st["v"]), v), "v differs at step %d" % step
        assert np.array_equal(_host(net), w), "weights differ at step %d" % step
    assert tr.state["t"] == 3
    # the regulariser reached the twelve kernels only
    z = np.zeros_like(w)
    _, m1, _ = b2.adam_bneck2(w, z, z, z, k, 5e-4, 0.9, 0.99, 1e-8, b1p, b2p, l1=1e-4, l2=2e-4)
    for name, (lo, hi) in b2.offsets(k).items():
        assert bool(m1[lo:hi].any()) == (name in b2.KERNELS), name
    assert len(b2.KERNELS) == 12


@pytest.fixture(scope="module")
def icnet19():
    net = _net(19)
    syn.randomize_icnet(net, seed=0)
    return net


@pytest.mark.parametrize("u8", [False, True])
def test_entries_from_frames_equal_entries_from_features_and_the_model_sees_the_weights(icnet19, u8):
    from oracle import icnet_oracle as icor
    net = _net(19)
    net.assign_named({v.name: v.numpy() for v in icnet19.variables})
    start = {v.name: v.numpy().copy() for v in net.variables}
    x = syn.synth_frames_device(3, 2, 64, 128, 3, dtype=torch.uint8 if u8 else None)
    labels, mask = _targets()
    tr = ICNetDeepBottleneckTrainer(net, 5e-4, 0.9, 0.99, loginverse_scaling=1.02, label_smoothing=0.1, l2=2e-4)
    feats = tr.features(x)
    assert [tuple(t.shape) for t in feats] == [(2, 2, 4, 1024), (2, 4, 8, 256), (2, 8, 16, 64)]
    assert torch.equal(feats[0], net.endpoint("conv5_1"))  # readable as an endpoint after a plain forward
    # gradient(images) == gradient_features(features(images)), bit for bit: the truncated schedule changes no bits
    tr.reinitialize(seed=4)
    li, gi = tr.gradient(x, labels, mask)
    lf, gf = tr.gradient_features(*feats, labels, mask)
    assert torch.equal(li, lf)
    for name in b2.NAMES:
        assert torch.equal(gi[name], gf[name]), name
    head0 = {n: _var(net, n).numpy().copy() for n in b2.NAMES}
    la = [float(tr.step(x, labels, mask)) for _ in range(2)]
    wa = _host(net)
    _assign(net, head0)
    tr.reinitialize(seed=4)
    _assign(net, {n: head0[n] for n in b2.NAMES[-2:]})  # (reinitialize re-drew conv6_cls from the same seed: the same values)
    lb = [float(tr.step_features(*feats, labels, mask)) for _ in range(2)]
    wb = _host(net)
    assert la == lb, "step(images) losses %r != step_features losses %r" % (la, lb)
    assert np.array_equal(wa, wb)
    assert tr.state["t"] == 2
    # after three steps the model and its handle see the trained weights (ssal_icnet_update_bneck2): net.score and the logits
    # equal a fresh ICNet's with the same variables assigned, and the C oracle's forward
    tr.step(x, labels, mask)
    trained = {id(_var(net, n)) for n in b2.NAMES}
    for name in b2.KERNELS:
        assert not np.array_equal(start[_var(net, name).name], _var(net, name).numpy()), name
    for v in net.variables:
        if id(v) not in trained:
            assert np.array_equal(start[v.name], v.numpy()), "frozen variable %s changed" % v.name
    fresh = _net(19)
    fresh.assign_named({v.name: v.numpy() for v in net.variables})
    s_got, ex = net.score(x, return_label=True)
    s_want, ex_want = fresh.score(x, return_label=True)
    logits = net(x, training=False)
    torch.cuda.synchronize()
    assert torch.equal(s_got, s_want) and torch.equal(ex["label"], ex_want["label"])
    assert torch.equal(logits, fresh(x, training=False))
    P = syn.icnet_params_dict(net)
    for name in (b2.BLOCK_R[0], b2.BLOCK_3[0], b2.BLOCK_I[0]):
        assert np.array_equal(P[name], _var(net, name).numpy())
    assert np.array_equal(logits.cpu().numpy(), icor.icnet_forward(P, frames([3, 4], 64, 128, 3)))


@pytest.mark.parametrize("u8", [False, True])
def test_truncated_trunk_writes_the_bits_of_the_unfused_forward(icnet19, u8):
    """the images entry's trunk ends behind conv5_1; what it leaves in conv5_1 / conv3_1 / conv3_sub1 are the bits of the unfused
    forward, and the six layers of conv5_2 and conv5_3 that the trained forward writes are too (the trainer's weights are the
    model's): a gradient from frames equals, bit for bit, the gradient from the forward call's endpoints, on a handle whose
    endpoints were overwritten in between"""
    net = _net(19)
    net.assign_named({v.name: v.numpy() for v in icnet19.variables})
    x = syn.synth_frames_device(5, 2, 64, 128, 3, dtype=torch.uint8 if u8 else None)
    other = syn.synth_frames_device(6, 2, 64, 128, 3, dtype=torch.uint8 if u8 else None)
    labels, mask = _targets(11)
    tr = ICNetDeepBottleneckTrainer(net, 5e-4, loginverse_scaling=1.02)
    feats = tr.features(x)
    net(x, training=False)
    for name, t in zip(tr._FEATURE_NAMES, feats):
        assert torch.equal(t, net.endpoint(name)), name
    inner = {name: net.endpoint(name).clone() for name in BLOCK_LAYERS}
    net(other, training=False)  # other values in every endpoint
    li, gi = tr.gradient(x, labels, mask)
    for name, t in zip(tr._FEATURE_NAMES, feats):
        assert torch.equal(t, net.endpoint(name)), "the truncated trunk's %s differs from the unfused forward's" % name
    for name, t in inner.items():
        assert torch.equal(t, net.endpoint(name)), name
    lf, gf = tr.gradient_features(*feats, labels, mask)
    assert torch.equal(li, lf)
    for name in b2.NAMES:
        assert torch.equal(gi[name], gf[name]), name


def test_end_to_end_fifty_steps_next_to_the_bottleneck_trainer(icnet19):
    """section 15's 50-step run (same seed, labels and hyper-parameters) on cached features: the loss falls; final / first is
    printed next to the bottleneck trainer's on the same frames (recorded in DESIGN.md section 43, not asserted against it:
    nine more variables under Adam need not fall faster in 50 steps)"""
    x = syn.synth_frames_device(0, 2, 64, 128, 3)
    params = {"hyperparams": {"learning_rate": 0.0005, "learning_rate_decay": 0.0,
                              "optimizer": {"type": "Adam", "kwargs": {"beta1": 0.9, "beta2": 0.99}},
                              "weight_reg": {"L2": 0.0002, "L1": 0.0},
                              "softmax": {"label_smoothing": 0.0, "loginverse_scaling": 1.02, "multiscale": False}}}
    for cls in (ICNetDeepBottleneckTrainer, ICNetBottleneckTrainer):
        net = _net(19)
        net.assign_named({v.name: v.numpy() for v in icnet19.variables})
        _, extra = net.score(x, return_label=True)
        labels = extra["label"].clone()
        mask = torch.ones((2, 64, 128), dtype=torch.float32, device=x.device)
        tr = cls.from_params(net, params)
        feats = tr.features(x)
        tr.reinitialize(seed=0)
        got = [float(tr.step_features(*feats, labels, mask)) for _ in range(50)]
        assert np.isfinite(got).all() and got[-1] < got[0]
        print("end to end %s: loss %.6g -> %.6g (x%.6f)" % (cls.__name__, got[0], got[-1], got[-1] / got[0]))
