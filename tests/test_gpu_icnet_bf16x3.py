"""GPU gate of ICNet's opt-in ``arithmetic="bf16x3"`` mode.

Per operator, through ``ssal_conv_bn_act_arith``: ``|kernel - value| <= bound`` per element against the model of the kernel's own
arithmetic (tests/icnet_split_model.py), bit equality where the bound is 0; tests/test_icnet_bf16x3_cpu.py proves that a kernel
which loses one of the six products, or a K = 16 step, cannot pass the live-chunk and exact cases.  Whole network on the golden
fixture's frames: every layer the mode runs against the model on the exact path's input endpoint, and logits / scores against
the float64 evaluation of the network, at most 4 x the exact path's own distance from it (the 4 is derived in DESIGN.md)."""
import os

import numpy as np
import pytest
import torch

import icnet_split_model as ism
import semanticsegmentationactivelearning_amd as ssal
from helpers import frames
from oracle import torch_restatement as tr
from semanticsegmentationactivelearning_amd import _lib, inference as inf, synthetic as syn
from semanticsegmentationactivelearning_amd.models.util import conv_ops as cops

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    _lib.lib()
    yield
    torch.cuda.synchronize()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bn(rng, c):
    return (rng.normal(0, 0.1, c).astype(np.float32), rng.uniform(0.5, 1.5, c).astype(np.float32),
            rng.uniform(0.8, 1.2, c).astype(np.float32), rng.normal(0, 0.1, c).astype(np.float32))


def run(x, k, stride=1, dil=1, bn=None, bias=None, res=None, relu=False, arithmetic="bf16x3"):
    y = cops.conv_bn_act(dev(x), k, stride, dil, bn=bn, bias=bias, residual=None if res is None else dev(res), relu=relu,
                         arithmetic=arithmetic)
    return y.cpu().numpy()


def gate(tag, got, value, bound):
    """|kernel - value| <= bound per element; the same bits where the bound is 0"""
    assert got.shape == value.shape and got.dtype == np.float32, tag
    err = np.abs(got.astype(np.float64) - value.astype(np.float64))
    live = bound > 0
    worst = float((err[live] / bound[live]).max()) if live.any() else 0.0
    print("%s: max err %.3g, worst err / bound %.3g, exact elements %d of %d" % (tag, err.max(), worst, (~live).sum(), live.size))
    assert (err <= bound).all(), "%s: %d of %d elements beyond the bound (worst %.3g x)" % (tag, (err > bound).sum(), err.size, worst)
    exact = ~live
    assert np.array_equal(got[exact].view(np.uint32), value[exact].view(np.uint32)), "%s: bits differ where the bound is 0" % tag


def _case(rng, n, h, w, cin, cout, k, stride, dil, res, relu, bn):
    x = rng.normal(size=(n, h, w, cin)).astype(np.float32)
    kern = (rng.normal(size=(k, k, cin, cout)) / np.sqrt(k * k * cin)).astype(np.float32)
    ho, wo, _, _ = ism.same_geometry(h, w, k, k, stride, dil)
    r = rng.normal(size=(n, ho, wo, cout)).astype(np.float32) if res else None
    return x, kern, (_bn(rng, cout) if bn else None), (None if bn else rng.normal(size=cout).astype(np.float32)), r


# (n, h, w, cin, cout, k, stride, dil, res, relu, batch-norm): rows and padding, channels, epilogues -- all NT = 1
SMALL = [
    (1, 3, 5, 32, 32, 1, 1, 1, False, True, True),      # M = 15 < one tile
    (1, 9, 15, 64, 32, 1, 1, 1, True, True, True),      # M = 135: a full tile and a 7-row tail; two chunks per tap
    (2, 5, 7, 96, 32, 1, 1, 1, False, False, True),     # an image boundary inside a tile; an odd three chunks
    (2, 5, 7, 64, 19, 3, 2, 1, True, False, False),     # stride 2 on the odd map; padded column tile; bias-only + res, no ReLU
    (1, 3, 5, 32, 32, 3, 1, 2, False, True, True),      # dilation 2
    (1, 3, 5, 64, 32, 3, 1, 4, True, True, False),      # dilation 4: every non-centre tap is padding
    (1, 9, 15, 32, 160, 1, 1, 1, False, True, True),    # five column tiles
    (1, 9, 15, 96, 19, 3, 1, 1, False, True, False),    # 3 x 3, 27 chunks, 19 of 32 columns, bias + ReLU
    (2, 5, 7, 32, 160, 3, 2, 2, True, True, True),      # stride 2 and dilation 2 together, five column tiles, res
]


@pytest.mark.parametrize("case", SMALL, ids=lambda c: "n%dx%dx%d_c%d_%d_k%d_s%d_d%d%s%s%s" % (c[:8] + ("_res" if c[8] else "", "_relu" if c[9] else "", "_bn" if c[10] else "_bias")))
def test_operator_against_the_model(case):
    n, h, w, cin, cout, k, stride, dil, res, relu, bn = case
    assert _lib.icnet_conv_dispatch(n, h, w, cin, cout, k, stride, dil, False, res, "bf16x3") == ("k_igemm_bf16x3", 1)
    x, kern, bnv, bias, r = _case(np.random.default_rng(sum(case)), *case)
    value, bound = ism.conv(x, kern, stride, dil, bn=bnv, bias=bias, res=r, relu=relu)
    got = run(x, kern, stride, dil, bnv, bias, r, relu)
    gate(str(case), got, value, bound)
    assert np.array_equal(run(x, kern, stride, dil, bnv, bias, r, relu).view(np.uint32), got.view(np.uint32)), "two calls, two results"
    # f32 through the _arith hook is the plain entry
    plain = cops.conv_bn_act(dev(x), kern, stride, dil, bn=bnv, bias=bias, residual=None if r is None else dev(r), relu=relu)
    hook = cops.conv_bn_act(dev(x), kern, stride, dil, bn=bnv, bias=bias, residual=None if r is None else dev(r), relu=relu, arithmetic="f32")
    assert torch.equal(plain, hook)


@pytest.fixture(scope="module")
def large_input():
    """1 x 255 x 258: M = 65 790 = 514 row tiles, the last one two rows short -- enough tiles for NT = 2 and 4"""
    rng = np.random.default_rng(255)
    return {c: rng.normal(size=(1, 255, 258, c)).astype(np.float32) for c in (32, 64)}


@pytest.mark.parametrize("cin,cout,k,dil,nt", [(64, 64, 1, 1, 2), (64, 128, 1, 1, 4), (32, 64, 3, 2, 2), (32, 128, 3, 2, 4)])
def test_wide_column_tiles(large_input, cin, cout, k, dil, nt):
    x = large_input[cin]
    assert _lib.icnet_conv_dispatch(1, 255, 258, cin, cout, k, 1, dil, False, True, "bf16x3") == ("k_igemm_bf16x3", nt)
    rng = np.random.default_rng(cin + cout + k)
    kern = (rng.normal(size=(k, k, cin, cout)) / np.sqrt(k * k * cin)).astype(np.float32)
    bnv = _bn(rng, cout)
    r = rng.normal(size=(1, 255, 258, cout)).astype(np.float32)
    value, bound = ism.conv(x, kern, 1, dil, bn=bnv, res=r, relu=True)
    gate("NT = %d" % nt, run(x, kern, 1, dil, bnv, None, r, True), value, bound)


@pytest.mark.parametrize("k,cin,cout,step", ism.LIVE_CASES, ids=lambda v: str(v))
def test_live_chunk_cases(k, cin, cout, step):
    x, w = ism.live_case(k, cin, cout, step)
    bn = ism.identity_bn(cout)
    value, bound = ism.conv(x, w, bn=bn)
    gate("live step %d" % step, run(x, w, bn=bn), value, bound)


@pytest.mark.parametrize("k,cin,cout", ism.EXACT_CASES, ids=lambda v: str(v))
def test_exact_cases_bit_for_bit(k, cin, cout):
    x, w = ism.exact_case(k, cin, cout)
    bn = ism.identity_bn(cout)
    value, bound = ism.conv(x, w, bn=bn)
    assert not bound.any()
    got = run(x, w, bn=bn)
    gate("exact", got, value, bound)
    assert not np.array_equal(got, run(x, w, bn=bn, arithmetic="f32"))  # the six-product sum is not the fp32 product here


def test_zero_input_and_dead_channel_give_exact_zeros():
    rng = np.random.default_rng(11)
    kern = rng.normal(size=(3, 3, 64, 40)).astype(np.float32)
    kern[..., 7] = 0.0
    zeros = run(np.zeros((2, 5, 7, 64), np.float32), kern)
    assert not zeros.view(np.uint32).any()  # +0 everywhere: padding and data alike split to (0, 0, 0)
    x = rng.normal(size=(2, 5, 7, 64)).astype(np.float32)
    assert not run(x, kern, dil=2)[..., 7].view(np.uint32).any()
    assert run(x, kern, dil=2)[..., 6].any()


# ---- whole network on the golden fixture's frames ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_net():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "icnet_c3k19_64x128.npz"))
    net = ssal.ICNet(19)
    net.build((None, None, None, 3))
    syn.randomize_icnet(net, seed=0)
    x = frames(list(g["frame_ids"]), 64, 128, 3)
    assert x.shape == (2, 64, 128, 3)
    return net, syn.icnet_params_dict(net), x


def test_f32_keyword_is_the_plain_call(golden_net):
    net, _, x = golden_net
    xd = dev(x)
    assert torch.equal(net(xd, arithmetic="f32"), net(xd))
    for m in ("margin", "entropy", "confidence"):
        a, ea = net.score(xd, m, return_label=True, return_confidence=True, arithmetic="f32")
        b, eb = net.score(xd, m, return_label=True, return_confidence=True)
        assert torch.equal(a, b) and torch.equal(ea["label"], eb["label"]) and torch.equal(ea["confidence"], eb["confidence"])
    assert torch.equal(inf.predict(net, xd, arithmetic="f32"), inf.predict(net, xd))
    assert inf.predict(net, xd, arithmetic="bf16x3").shape == (2, 64, 128)


def test_every_layer_of_the_mode_against_the_model(golden_net):
    net, P, x = golden_net
    net(dev(x))  # exact path: every endpoint is a layer output
    ends = {}
    checked = 0
    for c in ism.icnet_convs():
        h, w = 64 // c["div"], 128 // c["div"]
        kernel = _lib.icnet_conv_dispatch(2, h, w, c["cin"], c["cout"], c["k"], c["stride"], c["dil"], c["up2"], c["res"] is not None, "bf16x3")[0]
        if kernel != "k_igemm_bf16x3":
            continue
        for e in (c["src"], c["res"]):
            if e is not None and e not in ends:
                ends[e] = net.endpoint(e).cpu().numpy()
        xin, r = ends[c["src"]], (ends[c["res"]] if c["res"] else None)
        kern = P[c["name"] + ".kernel"]
        bn = tuple(P[c["name"] + "." + a] for a in ("mean", "variance", "gamma", "beta"))
        value, bound = ism.conv(xin, kern, c["stride"], c["dil"], bn=bn, res=r, relu=c["relu"])
        gate(c["name"], run(xin, kern, c["stride"], c["dil"], bn, None, r, c["relu"]), value, bound)
        checked += 1
    assert checked == 64 - 10  # every convolution but the ten that stay exact (tests/test_icnet_bf16x3_cpu.py)
    # endpoint() after a call in the mode returns that call's layer outputs
    exact = net.endpoint("conv5_4_k1").cpu().numpy()
    net(dev(x), arithmetic="bf16x3")
    got = net.endpoint("conv5_4_k1").cpu().numpy()
    assert got.shape == exact.shape and not np.array_equal(got, exact)


def test_network_within_four_times_the_exact_paths_distance_from_float64(golden_net):
    """per product the mode drops x2w3 + x3w2 + x3w3 <= 2 u |xw| and rounds at most once per instruction
    where the fmaf chain rounds once per product: worst-case coefficient 3 against the exact path's 1, 4 with one unit of slack"""
    net, P, x = golden_net
    old = tr.DTYPE
    try:
        tr.DTYPE = torch.float64
        ref = np.asarray(tr.icnet_forward(P, x), np.float64)
        scores64 = {m: tr.score_logits(ref, m)[0] for m in ("margin", "entropy", "confidence")}  # float64 per pixel too
    finally:
        tr.DTYPE = old
    assert ref.dtype == np.float64 and ref.shape == (2, 64, 128, 19)
    xd = dev(x)
    d_exact = np.abs(net(xd).cpu().numpy().astype(np.float64) - ref).max()
    d_mode = np.abs(net(xd, arithmetic="bf16x3").cpu().numpy().astype(np.float64) - ref).max()
    print("logits: exact %.3g, bf16x3 %.3g from float64: ratio %.2f" % (d_exact, d_mode, d_mode / d_exact))
    assert d_exact > 0 and d_mode <= 4 * d_exact
    for m in ("margin", "entropy", "confidence"):
        want = scores64[m]
        se = np.abs(net.score(xd, m).cpu().numpy() - want).max()
        sm = np.abs(net.score(xd, m, arithmetic="bf16x3").cpu().numpy() - want).max()
        print("%s score: exact %.3g, bf16x3 %.3g from float64: ratio %.2f" % (m, se, sm, sm / se if se else float("inf")))
        assert sm <= 4 * se
