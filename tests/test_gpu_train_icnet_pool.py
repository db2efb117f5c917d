"""Training of ICNet through its pyramid pooling on the MI355X: all twenty gradients against the float64
oracle, elementwise, on inputs of random sign and on sign-coherent ones where the bound is tight; the loss and the pyramid
trainer's seventeen gradients against ``ICNetPyramidTrainer`` on the forward path's ``conv5_3_sum``, bit for bit; determinism;
dead channels; Adam bit for bit against the float32 restatement; the images entries against the features entries, the truncated
trunk against the unfused forward, and the model's handle after training; a short end-to-end run against its float64
restatement."""
import numpy as np
import pytest
import torch

import semanticsegmentationactivelearning_amd as ssal
from semanticsegmentationactivelearning_amd import inference
from semanticsegmentationactivelearning_amd import synthetic as syn
from semanticsegmentationactivelearning_amd.models.util import conv_ops as cops
from semanticsegmentationactivelearning_amd.training import ICNetPoolingTrainer, ICNetPyramidTrainer

import icnet_pool_train_oracle as po
import icnet_pyramid_train_oracle as ipo
from helpers import frames

pytestmark = pytest.mark.gpu

STAT_NAMES = (po.LAYER + ".mean", po.LAYER + ".variance", "conv5_4_k1.mean", "conv5_4_k1.variance", "conv_sub4.mean",
              "conv_sub4.variance", "conv3_1_sub2_proj.mean", "conv3_1_sub2_proj.variance", "conv_sub2.mean",
              "conv_sub2.variance", "conv3_sub1_proj.mean", "conv3_sub1_proj.variance")
STAT_SEED = 411


def _var(net, name):
    layer, attr = name.split(".")
    return getattr(getattr(net, layer), attr)


def _net(k):
    net = ssal.ICNet(k)
    net.build((None, None, None, 3))
    return net


def _assign(net, d):
    for name, v in d.items():
        _var(net, name).assign(v)


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
    statistics are ``po.draw_stats(STAT_SEED)``"""
    if k not in _NETS:
        net = _net(k)
        _assign_stats(net, po.draw_stats(STAT_SEED))
        _NETS[k] = net
    return _NETS[k]


def _stats(net):
    return np.concatenate([_var(net, n).numpy() for n in STAT_NAMES])


def _forward(net, a, c52, c31, c3, d):
    """(conv5_3, conv5_3_sum, conv5_4_k1, sub24_sum, sub12_sum, full-resolution logits) as the forward path's own operators
    compute them from the same weights"""
    bn = lambda layer: (_var(net, layer + ".mean").numpy(), _var(net, layer + ".variance").numpy(), d[layer + ".gamma"],
                        d[layer + ".beta"])
    c53 = cops.conv_bn_act(torch.as_tensor(a).cuda(), d[po.BLOCK[0]], bn=bn(po.LAYER), residual=torch.as_tensor(c52).cuda(),
                           relu=True)
    s53 = cops.pyramid_pooling(c53)
    f1 = cops.conv_bn_act(s53, d["conv5_4_k1.kernel"], bn=bn("conv5_4_k1"), relu=True)
    p24 = cops.conv_bn_act(torch.as_tensor(c31).cuda(), d["conv3_1_sub2_proj.kernel"], bn=bn("conv3_1_sub2_proj"), relu=False)
    sub24 = cops.conv_bn_act(f1, d["conv_sub4.kernel"], dilation=2, bn=bn("conv_sub4"), residual=p24, relu=True, upsample2x=True)
    proj = cops.conv_bn_act(torch.as_tensor(c3).cuda(), d["conv3_sub1_proj.kernel"], bn=bn("conv3_sub1_proj"), relu=False)
    sub12 = cops.conv_bn_act(sub24, d["conv_sub2.kernel"], dilation=2, bn=bn("conv_sub2"), residual=proj, relu=True,
                             upsample2x=True)
    lq = cops.conv_bn_act(sub12, d["conv6_cls.kernel"], bias=d["conv6_cls.bias"], relu=False, upsample2x=True)
    return c53, s53, f1, sub24, sub12, inference.resize_bilinear(lq, (4 * lq.shape[1], 4 * lq.shape[2]))


def _pack(gd):
    return np.concatenate([gd[n].cpu().numpy().reshape(-1) for n in po.NAMES])


_ORACLE = {}


def _oracle(key, net, a, c52, c31, c3, d, labels, mask, weight, ls, acts):
    """the float64 gradient, its magnitude sums and the loss: they do not depend on ``max_workgroups``, so the cases that
    differ in it alone share one evaluation (``acts``, the fp32 forward values, do not depend on it either)"""
    if key not in _ORACLE:
        _ORACLE[key] = po.grad_and_bound(a, c52, c31, c3, po.pack(d), _stats(net), labels, mask, weight, ls,
                                         tuple(t.cpu().numpy() for t in acts))
    return _ORACLE[key]


def _check_gradient(net, k, a, c52, c31, c3, d, labels, mask, weight, ls, mw, tag, key):
    n, h, w, _ = a.shape
    tr = ICNetPoolingTrainer(net, 1e-3, loginverse_scaling=weight, label_smoothing=ls)
    dev = [torch.as_tensor(t).cuda() for t in (a, c52, c31, c3)]
    loss, gd = tr.gradient_features(*dev, labels, mask, params=d, max_workgroups=mw)
    loss2, gd2 = tr.gradient_features(*dev, labels, mask, params=d, max_workgroups=mw)
    acts = _forward(net, a, c52, c31, c3, d)
    pyr = ICNetPyramidTrainer(net, 1e-3, loginverse_scaling=weight, label_smoothing=ls)
    ploss, pgd = pyr.gradient_features(acts[1], dev[2], dev[3], labels, mask, params={n_: d[n_] for n_ in ipo.NAMES},
                                       max_workgroups=mw)
    torch.cuda.synchronize()
    g = _pack(gd)
    assert np.array_equal(g, _pack(gd2)) and torch.equal(loss, loss2), "two calls differ"
    # the loss and the seventeen gradients of section 39: the bits of the pyramid trainer on the forward path's conv5_3_sum
    assert torch.equal(loss, ploss), "loss %.17g != pyramid trainer's %.17g" % (float(loss[0]), float(ploss[0]))
    for name in ipo.NAMES:
        assert torch.equal(gd[name], pgd[name]), name
    pre_sign = acts[0].cpu().numpy() > 0
    assert pre_sign.any() and not pre_sign.all(), "conv5_3's pre-activation must have both signs"
    g64, c, loss64 = _oracle(key, net, a, c52, c31, c3, d, labels, mask, weight, ls, acts)
    dlt = np.abs(g.astype(np.float64) - g64)
    bad = []
    for name, (lo, hi) in po.offsets(k).items():
        kap = po.kappa(name, n, h, w, k, weight, mw)
        bound = kap * 2.0 ** -24 * c[lo:hi]
        ratio = (dlt[lo:hi] / np.maximum(bound, 1e-300)).max()
        print("%s %s: kappa %.0f, max |g - g64| %.3e, max |g - g64| / bound %.3e, max |g64| %.3e"
              % (tag, name, kap, dlt[lo:hi].max(), ratio, np.abs(g64[lo:hi]).max()))
        if (dlt[lo:hi] > bound).any():
            bad.append((name, int((dlt[lo:hi] > bound).sum()), float(ratio)))
    assert not bad, "entries beyond kappa 2^-24 C: %r" % (bad,)
    assert abs(float(loss[0]) - loss64) <= 1e-5 * abs(loss64)
    return gd, g64, acts[0]


# N x h32 x w32
SHAPES = [(1, 1, 1),   # every bin of every level is the one pixel (36 coinciding bins at level 6, one of them read)
          (2, 2, 3),
          (1, 3, 2),   # b = 6 > h: coinciding bins, bins the resize never reads
          (1, 3, 5),   # 3 does not divide 5: overlapping bins
          (2, 5, 9)]   # overlap on both axes at b = 2, 3, 6; P = 90 is no multiple of the 32-pixel tile of the weight gradient
                       # (3 tiles, the last of 26 pixels) nor of the data gradient's 64 (2 tiles, the last of 26); at
                       # max_workgroups = 2 the split-K groups take 2 and 1 tiles (a ragged last group)
GROUPS = [(s, k, wl) for s in SHAPES for k in (2, 19) for wl in ((0.0, 0.0), (1.02, 0.1))]
CASES = [(s, mw, k, wl) for (s, k, wl) in GROUPS for mw in (0, 1, 2)]


@pytest.mark.parametrize("shape,mw,k,wl", CASES)
def test_gradients_bits_and_determinism(shape, mw, k, wl):
    """|g - g64| <= kappa 2^-24 C_j for every entry of all twenty gradients; the loss within 1e-5 of float64; the loss and
    section 39's seventeen gradients bit-identical to ICNetPyramidTrainer on the forward path's conv5_3_sum; two calls give the
    same bits"""
    n, h, w = shape
    key = GROUPS.index((shape, k, wl))
    a, c52, c31, c3, d, labels, mask = po.case(6000 + key, n, h, w, k)
    _check_gradient(_shared_net(k), k, a, c52, c31, c3, d, labels, mask, wl[0], wl[1], mw,
                    "K=%d w=%g ls=%g %s mw=%d" % (k, wl[0], wl[1], shape, mw), key)


# the sign-coherent inputs (icnet_pool_train_oracle.coherent_case): tests/test_train_icnet_pool_cpu.py shows on these very arrays
# that the wrong backward passes leave the bound on every tensor they corrupt
COHERENT_SEED = 7
COHERENT = [(s, mw, k, wl) for s in ((1, 3, 5), (2, 5, 9)) for k, wl in ((2, (0.0, 0.0)), (19, (1.02, 0.1))) for mw in (0, 1, 2)]
_COHERENT = {}


@pytest.mark.parametrize("shape,mw,k,wl", COHERENT)
def test_gradients_on_sign_coherent_inputs(shape, mw, k, wl):
    """the same checks where the bound is tight: the CPU discrimination test's arrays"""
    n, h, w = shape
    if (shape, k) not in _COHERENT:
        arrays = po.coherent_case(COHERENT_SEED, n, h, w, k)
        net = _net(k)
        _assign_stats(net, arrays[5])
        _COHERENT[(shape, k)] = (arrays, net)
    (a, c52, c31, c3, d, stats, labels, mask), net = _COHERENT[(shape, k)]
    assert np.array_equal(_stats(net), stats)
    _check_gradient(net, k, a, c52, c31, c3, d, labels, mask, wl[0], wl[1], mw,
                    "coherent K=%d w=%g %s mw=%d" % (k, wl[0], shape, mw), ("coherent", shape, k))


@pytest.mark.parametrize("mw", [0, 2])
def test_dead_channels(mw):
    """a beta of -1e4 on channels 0..4 makes conv5_3 exactly 0 there: relu'(0) = 0, so g53 is exactly 0 on those units and the
    three gradients along them are exactly 0, in the GPU result and in the oracle; a gamma of 0 passes no kernel gradient along
    its output and still gets its own"""
    k = 19
    a, c52, c31, c3, d, labels, mask = po.case(43, 2, 2, 3, k)
    d[po.BLOCK[2]][:5] = -1e4
    d[po.BLOCK[1]][7] = 0.0
    d[po.BLOCK[2]][7] = 0.2  # (alive: with a zero scale the unit is relu(beta + conv5_2) everywhere)
    net = _shared_net(k)
    gd, g64, c53 = _check_gradient(net, k, a, c52, c31, c3, d, labels, mask, 1.02, 0.1, mw, "dead channels mw=%d" % mw,
                                   ("dead", mw))
    assert not c53[..., :5].any() and c53[..., 5:].any()
    g64d = po.unpack(g64)
    for name in po.BLOCK:
        assert not gd[name][..., :5].any() and not g64d[name][..., :5].any(), name
    assert not gd[po.BLOCK[0]][..., 7].any() and float(gd[po.BLOCK[1]][7]) != 0.0
    assert not g64d[po.BLOCK[0]][..., 7].any() and float(g64d[po.BLOCK[1]][7]) != 0.0


def _host(net):
    return np.concatenate([_var(net, n).numpy().reshape(-1) for n in po.NAMES])


def test_adam_three_steps_bit_identical_to_float32_restatement():
    k = 19
    a, c52, c31, c3, d, labels, mask = po.case(12, 2, 2, 3, k)
    d[po.BLOCK[0]][0, 0, :3] = 0.0  # exact zeros: sign(0) = 0
    net = _net(k)
    _assign_stats(net, po.draw_stats(STAT_SEED))
    _assign(net, d)
    tr = ICNetPoolingTrainer(net, 5e-4, 0.9, 0.99, l1=1e-4, l2=2e-4, loginverse_scaling=1.02, learning_rate_decay=0.5,
                             decay_steps=4)
    dev = [torch.as_tensor(t).cuda() for t in (a, c52, c31, c3)]
    w = po.pack(d).astype(np.float32)
    m, v = np.zeros_like(w), np.zeros_like(w)
    b1p, b2p = np.float32(0.9), np.float32(0.99)
    for step in range(3):
        _, gd = tr.gradient_features(*dev, labels, mask)
        lr = tr.current_learning_rate()
        tr.step_features(*dev, labels, mask)
        w, m, v = po.adam_pool(w, m, v, _pack(gd), k, lr, 0.9, 0.99, 1e-8, b1p, b2p, l1=1e-4, l2=2e-4)
        b1p, b2p = np.float32(b1p * np.float32(0.9)), np.float32(b2p * np.float32(0.99))
        st = tr.state
        assert np.array_equal(po.pack(st["m"]), m), "m differs at step %d" % step
        assert np.array_equal(po.pack(st["v"]), v), "v differs at step %d" % step
        assert np.array_equal(_host(net), w), "weights differ at step %d" % step
    assert tr.state["t"] == 3
    # the regulariser reached the seven kernels only (the increase kernel among them)
    z = np.zeros_like(w)
    _, m1, _ = po.adam_pool(w, z, z, z, k, 5e-4, 0.9, 0.99, 1e-8, b1p, b2p, l1=1e-4, l2=2e-4)
    for name, (lo, hi) in po.offsets(k).items():
        assert bool(m1[lo:hi].any()) == (name in po.KERNELS), name
    assert po.BLOCK[0] in po.KERNELS and len(po.KERNELS) == 7


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
def test_entries_from_frames_equal_entries_from_features_and_the_model_sees_the_weights(icnet19, u8):
    from oracle import icnet_oracle as icor
    net = _net(19)
    net.assign_named({v.name: v.numpy() for v in icnet19.variables})
    start = {v.name: v.numpy().copy() for v in net.variables}
    x = syn.synth_frames_device(3, 2, 64, 128, 3, dtype=torch.uint8 if u8 else None)
    labels, mask = _targets()
    tr = ICNetPoolingTrainer(net, 5e-4, 0.9, 0.99, loginverse_scaling=1.02, label_smoothing=0.1, l2=2e-4)
    feats = tr.features(x)
    assert [tuple(t.shape) for t in feats] == [(2, 2, 4, 256), (2, 2, 4, 1024), (2, 4, 8, 256), (2, 8, 16, 64)]
    # gradient(images) == gradient_features(features(images)), bit for bit: the truncated schedule changes no bits
    tr.reinitialize(seed=4)
    li, gi = tr.gradient(x, labels, mask)
    lf, gf = tr.gradient_features(*feats, labels, mask)
    assert torch.equal(li, lf)
    for name in po.NAMES:
        assert torch.equal(gi[name], gf[name]), name
    head0 = {n: _var(net, n).numpy().copy() for n in po.NAMES}
    la = [float(tr.step(x, labels, mask)) for _ in range(2)]
    wa = _host(net)
    _assign(net, head0)
    tr.reinitialize(seed=4)
    _assign(net, {n: head0[n] for n in po.NAMES[-2:]})  # (reinitialize re-drew conv6_cls from the same seed: the same values)
    lb = [float(tr.step_features(*feats, labels, mask)) for _ in range(2)]
    wb = _host(net)
    assert la == lb, "step(images) losses %r != step_features losses %r" % (la, lb)
    assert np.array_equal(wa, wb)
    assert tr.state["t"] == 2
    # after three steps the model and its handle see the trained weights (ssal_icnet_update_pool): net.score and the logits
    # equal a fresh ICNet's with the same variables assigned, and the C oracle's forward
    tr.step(x, labels, mask)
    trained = {id(_var(net, n)) for n in po.NAMES}
    for name in po.KERNELS:
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
    assert np.array_equal(P[po.BLOCK[0]], _var(net, po.BLOCK[0]).numpy())
    assert np.array_equal(logits.cpu().numpy(), icor.icnet_forward(P, frames([3, 4], 64, 128, 3)))


@pytest.mark.parametrize("u8", [False, True])
def test_truncated_trunk_writes_the_bits_of_the_unfused_forward(icnet19, u8):
    """the images entry's trunk ends inside conv5_3; what it leaves in conv5_3_3x3 / conv5_2 / conv3_1 / conv3_sub1 are the bits
    of the unfused forward: a gradient from frames equals, bit for bit, the gradient from the forward call's endpoints, on a
    handle whose endpoints were overwritten in between"""
    net = _net(19)
    net.assign_named({v.name: v.numpy() for v in icnet19.variables})
    x = syn.synth_frames_device(5, 2, 64, 128, 3, dtype=torch.uint8 if u8 else None)
    other = syn.synth_frames_device(6, 2, 64, 128, 3, dtype=torch.uint8 if u8 else None)
    labels, mask = _targets(11)
    tr = ICNetPoolingTrainer(net, 5e-4, loginverse_scaling=1.02)
    feats = tr.features(x)
    net(x, training=False)
    for name, t in zip(tr._FEATURE_NAMES, feats):
        assert torch.equal(t, net.endpoint(name)), name
    net(other, training=False)  # other values in every endpoint
    li, gi = tr.gradient(x, labels, mask)
    for name, t in zip(tr._FEATURE_NAMES, feats):
        assert torch.equal(t, net.endpoint(name)), "the truncated trunk's %s differs from the unfused forward's" % name
    lf, gf = tr.gradient_features(*feats, labels, mask)
    assert torch.equal(li, lf)
    for name in po.NAMES:
        assert torch.equal(gi[name], gf[name]), name


def test_end_to_end_learns_as_its_float64_restatement(icnet19):
    """section 23's 50-step run (same seed, labels and hyper-parameters) on cached features: the loss falls, and final / first
    is within 0.01 of the same ratio of the float64 restatement of the loop (section 23's margin); the pyramid trainer's ratio
    on the same frames is printed next to it"""
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
    tr = ICNetPoolingTrainer.from_params(net, params)
    feats = tr.features(x)
    tr.reinitialize(seed=0)
    w0 = _host(net)
    got = [float(tr.step_features(*feats, labels, mask)) for _ in range(50)]
    want = po.train_float64(*(t.cpu().numpy() for t in feats), w0, _stats(net), labels.cpu().numpy(), mask.cpu().numpy(),
                            19, 50, 0.0005, 0.9, 0.99, 1e-8, 1.02, 0.0, 0.0002)
    pnet = _net(19)
    pnet.assign_named({v.name: v.numpy() for v in icnet19.variables})
    ptr = ICNetPyramidTrainer.from_params(pnet, params)
    pfeats = ptr.features(x)
    ptr.reinitialize(seed=0)
    pgot = [float(ptr.step_features(*pfeats, labels, mask)) for _ in range(50)]
    r, r64 = got[-1] / got[0], want[-1] / want[0]
    print("end to end: loss %.6g -> %.6g (x%.6f); float64 restatement %.6g -> %.6g (x%.6f); pyramid trainer %.6g -> %.6g (x%.6f)"
          % (got[0], got[-1], r, want[0], want[-1], r64, pgot[0], pgot[-1], pgot[-1] / pgot[0]))
    assert got[-1] < got[0]
    assert abs(r - r64) <= 0.01
