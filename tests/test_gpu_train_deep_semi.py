"""The semi-supervised step of the last-block and last-stage trainers on the MI355X: pseudo annotation,
training-pass confusion matrix and pseudo-pixel counts inside k_tb_head<K, true>, against the COMPOSITION of code the parent
pins to the oracles -- the model layers' logits, score_logits, training_targets, the parent class's plain gradient / step, the
stand-alone confusion op.  Sections 17 / 18 assert that the kernel's logits are the model layers' bit for bit and pixel_score is
one device function in both routes, so the condition is derived, not measured: loss and all 13 / 26 gradients bit-identical,
confusion matrix and pseudo-pixel counts equal."""
import numpy as np
import pytest
import torch

import semanticsegmentationactivelearning_amd as ssal
from semanticsegmentationactivelearning_amd import _lib
from semanticsegmentationactivelearning_amd import active_learning as al
from semanticsegmentationactivelearning_amd import synthetic as syn
from semanticsegmentationactivelearning_amd.tensortools import metrics
from semanticsegmentationactivelearning_amd.training import (LastBlockTrainer, LastStageTrainer, SemiSupervisedBlockTrainer,
                                                             SemiSupervisedStageTrainer)

import last_block_train_oracle as lbo
import last_stage_train_oracle as lso
from helpers import make_model

pytestmark = pytest.mark.gpu

MEASURES = ("entropy", "margin", "confidence")
LOSSES = ((0.0, 0.0), (1.02, 0.0), (0.0, 0.1), (1.02, 0.1))  # (weight, label smoothing)
_NETS = {}


def _net(k, seed=4321):
    """an ENet(k) with random variables and statistics in its last two blocks (the trunk is not used)"""
    if k not in _NETS:
        params, stats = lso.random_params(seed + k, k)
        net = ssal.ENet(k)
        net.build((None, None, None, 3))
        net.Final.kernel.assign(params["Final.kernel"])
        for blk, names in ((lbo.BLOCK, lbo.BLOCK_VARS), (lso.STAGE, lso.STAGE_VARS)):
            for a in names:
                getattr(getattr(net, blk), a).assign(params["%s.%s" % (blk, a)])
            for a in lso.STATS:
                getattr(getattr(net, blk), a).assign(stats[blk][a])
        _NETS[k] = net
    return _NETS[k]


class _Side:
    """one trainer family: how its inputs are drawn and how the model layers turn them into logits"""

    def __init__(self, stage):
        self.stage = stage
        self.fused_cls = SemiSupervisedStageTrainer if stage else SemiSupervisedBlockTrainer
        self.parent_cls = LastStageTrainer if stage else LastBlockTrainer
        self.up = 4 if stage else 2

    def inputs(self, rng, n, h, w):
        if self.stage:
            x = (rng.standard_normal((n, h, w, 64)) * 0.7).astype(np.float32)
            return (torch.as_tensor(x).cuda(), torch.as_tensor(lso.random_argmax(rng, n, h, w)).cuda())
        return (torch.as_tensor((rng.standard_normal((n, h, w, 16)) * 0.7).astype(np.float32)).cuda(),)

    def logits(self, net, inputs):
        a5 = net.Bottleneck5_0(inputs[0], inputs[1], training=False) if self.stage else inputs[0]
        return net.Final(net.Bottleneck5_1(a5, training=False), training=False)

    def raw_kw(self, raw):
        if raw is None:
            return {}
        return {"features_raw": raw[0], "argmax1_raw": raw[1]} if self.stage else {"features_raw": raw[0]}


BLOCK, STAGE = _Side(False), _Side(True)


def _annotation(rng, n, ho, wo, k, labelled):
    """label / mask planes on the device; the planes of unlabelled images hold 0xFF labels and NaN masks"""
    labels = rng.integers(0, k, (n, ho, wo)).astype(np.uint8)
    mask = (rng.uniform(size=(n, ho, wo)) > 0.25).astype(np.float32)
    labels[rng.uniform(size=labels.shape) < 0.05] = 255  # ignored pixels under both mask values
    for i, l in enumerate(labelled):
        if not l:
            labels[i] = 0xFF
            mask[i] = np.nan
    return torch.as_tensor(labels).cuda(), torch.as_tensor(mask).cuda()


def _yardstick_targets(side, net, k, inputs, raw, labels, mask, labelled, measure, threshold=None):
    """steps 2-4 and 6 of the composition: (target label, target mask, confusion, pseudo pixels, threshold).  threshold None:
    the median of the yardstick's confidence over the unlabelled pixels (0.5 where there are none)"""
    sel = torch.as_tensor(np.asarray(labelled, dtype=bool)).cuda()
    train_logits = side.logits(net, inputs)
    pseudo_logits = train_logits if raw is None else side.logits(net, raw)
    derived = threshold is None  # a threshold handed in (a training run's fixed one) is not held to the share condition
    if threshold is None:
        threshold = 0.5
        if not bool(sel.all()):
            _, p = al.score_logits(pseudo_logits, measure, 0.0, return_confidence=True)
            threshold = float(np.median(p["confidence"][~sel].float().cpu().numpy()))
    _, p = al.score_logits(pseudo_logits, measure, threshold, return_label=True, return_mask=True)
    pl, pm = p["label"], p["mask"].float()
    n_unl = int((~sel).sum())
    if n_unl:
        share = float(pm[~sel].mean())
        print("    threshold %.6g: %.3f of the unlabelled pixels pass" % (threshold, share))
        assert not derived or 0.3 <= share <= 0.7, "the threshold does not give a mixed pseudo mask (%.3f)" % share
    if n_unl < len(labelled):
        zero = float((mask[sel] == 0).float().mean())
        assert zero >= 0.05, "only %.3f of the labelled pixels carry mask 0" % zero
    if labels is None:
        lab, mk = pl, pm
    else:
        lab, mk = al.training_targets(sel, labels, mask, pl, pm)
    _, pt = al.score_logits(train_logits, "confidence", 0.0, return_label=True)  # the first maximum
    conf = metrics.confusion_mat(lab, pt["label"], k, weights=mk)
    pp = pm.to(torch.int64).sum(dim=(1, 2)) * (~sel).to(torch.int64)
    return lab, mk, conf, pp, threshold


def _assert_same(name, got, want):
    loss, grads, conf, pp = got
    wloss, wgrads, wconf, wpp = want
    print("    %s: loss %.17g / %.17g, confusion sum %d, pseudo pixels %s"
          % (name, float(loss.cpu()[0]), float(wloss.cpu()[0]), int(conf.sum()), pp.tolist()))
    assert loss.cpu().numpy().tobytes() == wloss.cpu().numpy().tobytes(), "%s: loss %r != %r" % (
        name, float(loss.cpu()[0]), float(wloss.cpu()[0]))
    assert set(grads) == set(wgrads)
    for nm in wgrads:
        g, w = grads[nm].contiguous().cpu().numpy(), wgrads[nm].contiguous().cpu().numpy()
        bad = int((g.view(np.uint32) != w.view(np.uint32)).sum())
        assert bad == 0, "%s: %s: %d of %d entries differ (max |d| %.3e)" % (name, nm, bad, g.size, np.abs(g - w).max())
    assert torch.equal(conf, wconf), "%s: confusion differs in %d entries" % (name, int((conf != wconf).sum()))
    assert torch.equal(pp, wpp), "%s: pseudo pixels %s != %s" % (name, pp.tolist(), wpp.tolist())


def _fused(side, tr, inputs, raw, labels, mask, labelled, measure, threshold, k, **kw):
    conf = torch.zeros((k, k), dtype=torch.int64, device="cuda")
    loss, grads, pp = tr.gradient_features(*inputs, labels, mask, labelled=labelled, measure=measure, threshold=threshold,
                                           confusion=conf, return_pseudo_pixels=True, **side.raw_kw(raw), **kw)
    return loss, grads, conf, pp


# (n, h, w, max_workgroups): block a5_0 3 x 20 x 17 (2 x 2 ragged tiles) and 1 x 33 x 65 (3 x 5 tiles with one-pixel edges:
# second-pass pixels cross every kind of tile border); stage a4_2 2 x 10 x 17 and 1 x 20 x 20 (9 tiles on 2 workgroups)
SHAPES = {False: ((3, 20, 17, 0), (1, 33, 65, 0)), True: ((2, 10, 17, 0), (1, 20, 20, 2))}
# None: `labelled` not given; "unl": every image unlabelled, labels = mask = None
PATTERNS = {1: {"none": None, "all": [1], "unl": [0]}, 2: {"none": None, "all": [1, 1], "mixed": [1, 0], "unl": [0, 0]},
            3: {"none": None, "all": [1, 1, 1], "mixed": [1, 0, 1], "unl": [0, 0, 0]}}


@pytest.mark.parametrize("stage", (False, True), ids=("block", "stage"))
@pytest.mark.parametrize("k", (2, 6, 19, 32))
@pytest.mark.parametrize("measure", MEASURES)
def test_feature_entry_matches_composition(stage, k, measure):
    """the main sweep: bitwise loss and gradients, exact confusion matrix and pseudo-pixel counts"""
    side = STAGE if stage else BLOCK
    net = _net(k)
    seed = 100000 * int(stage) + 1000 * k + 10 * MEASURES.index(measure)
    for n, h, w, mw in SHAPES[stage]:
        kw = {"max_workgroups": mw} if stage else {}
        for pname, pat in PATTERNS[n].items():
            seed += 1
            rng = np.random.default_rng(seed)
            inputs = side.inputs(rng, n, h, w)
            flags = [1] * n if pat is None else pat
            labels, mask = _annotation(rng, n, side.up * h, side.up * w, k, flags)
            if pname == "unl":
                labels = mask = None
            print("K=%d %s %dx%dx%d labelled=%s" % (k, measure, n, h, w, pname))
            lab, mk, wconf, wpp, thr = _yardstick_targets(side, net, k, inputs, None, labels, mask, flags, measure)
            for weight, ls in LOSSES:
                parent = side.parent_cls(net, 1e-3, loginverse_scaling=weight, label_smoothing=ls)
                fused = side.fused_cls(net, 1e-3, loginverse_scaling=weight, label_smoothing=ls)
                wloss, wgrads = parent.gradient_features(*inputs, lab, mk, **kw)
                got = _fused(side, fused, inputs, None, labels, mask, None if pat is None else np.asarray(pat, np.uint8),
                             measure, thr, k, **kw)
                _assert_same("w=%g ls=%g" % (weight, ls), got, (wloss, wgrads, wconf, wpp))


@pytest.mark.parametrize("stage", (False, True), ids=("block", "stage"))
@pytest.mark.parametrize("measure", MEASURES)
def test_raw_features_differ_from_training_features(stage, measure):
    """the pseudo annotation comes from features_raw (the stage's with its own argmax1_raw), the gradient from the training
    features; features_raw is features == no raw side; a copy goes through the target-only launch and gives the same"""
    side = STAGE if stage else BLOCK
    k, labelled = 19, ([0, 1] if stage else [0, 1, 0])
    n, h, w, _ = SHAPES[stage][0]
    net = _net(k)
    rng = np.random.default_rng(31 + MEASURES.index(measure) + 10 * int(stage))
    raw = side.inputs(rng, n, h, w)
    scale = torch.linspace(0.8, 1.25, raw[0].shape[-1], device="cuda")
    inputs = ((raw[0] * scale).contiguous(),) + ((torch.as_tensor(lso.random_argmax(rng, n, h, w)).cuda(),) if stage else ())
    if stage:
        assert not torch.equal(inputs[1], raw[1])
    labels, mask = _annotation(rng, n, side.up * h, side.up * w, k, labelled)
    parent = side.parent_cls(net, 1e-3, loginverse_scaling=1.02)
    fused = side.fused_cls(net, 1e-3, loginverse_scaling=1.02)
    lab, mk, wconf, wpp, thr = _yardstick_targets(side, net, k, inputs, raw, labels, mask, labelled, measure)
    wloss, wgrads = parent.gradient_features(*inputs, lab, mk)
    got = _fused(side, fused, inputs, raw, labels, mask, labelled, measure, thr, k)
    _assert_same("features_raw " + measure, got, (wloss, wgrads, wconf, wpp))
    one_pass = _fused(side, fused, inputs, None, labels, mask, labelled, measure, thr, k)
    assert not torch.equal(one_pass[1]["Final.kernel"], got[1]["Final.kernel"]), "the raw side made no difference"
    same = _fused(side, fused, inputs, inputs, labels, mask, labelled, measure, thr, k)
    _assert_same("features_raw is features", same, one_pass)
    clone = _fused(side, fused, inputs, tuple(t.clone() for t in inputs), labels, mask, labelled, measure, thr, k)
    _assert_same("features_raw == features (a copy: the target-only launch)", clone, one_pass)


@pytest.mark.parametrize("stage", (False, True), ids=("block", "stage"))
def test_determinism_accumulation_and_labelled_counts(stage):
    """two calls give the same bits; two calls into one matrix give twice one call; pseudo_pixels is 0 for labelled images;
    all-labelled without extras is the parent's plain gradient"""
    side = STAGE if stage else BLOCK
    k, labelled = 19, ([0, 1] if stage else [0, 1, 0])
    n, h, w, _ = SHAPES[stage][0]
    net = _net(k)
    rng = np.random.default_rng(55 + int(stage))
    inputs = side.inputs(rng, n, h, w)
    raw = tuple((t * 1.1).contiguous() if t.is_floating_point() else t.clone() for t in inputs)
    labels, mask = _annotation(rng, n, side.up * h, side.up * w, k, labelled)
    fused = side.fused_cls(net, 1e-3, loginverse_scaling=1.02, label_smoothing=0.1)
    a = _fused(side, fused, inputs, raw, labels, mask, labelled, "entropy", 0.2, k)
    b = _fused(side, fused, inputs, raw, labels, mask, labelled, "entropy", 0.2, k)
    _assert_same("second call", b, a)
    assert all(a[3][i].item() == 0 for i, l in enumerate(labelled) if l) and int(a[3].sum()) > 0
    conf = a[2].clone()
    fused.gradient_features(*inputs, labels, mask, labelled=labelled, threshold=0.2, confusion=conf, **side.raw_kw(raw))
    assert torch.equal(conf, 2 * a[2]) and int(a[2].sum()) > 0
    # all labelled: the parent's bits through the plain entry (no keyword) and through the semi entry (labelled all ones)
    labels1, mask1 = _annotation(rng, n, side.up * h, side.up * w, k, [1] * n)
    parent = side.parent_cls(net, 1e-3, loginverse_scaling=1.02, label_smoothing=0.1)
    l0, g0 = parent.gradient_features(*inputs, labels1, mask1)
    l1, g1 = fused.gradient_features(*inputs, labels1, mask1)
    l2, g2 = fused.gradient_features(*inputs, labels1, mask1, labelled=torch.ones(n, dtype=torch.bool))
    assert torch.equal(l0, l1) and torch.equal(l0, l2)
    assert all(torch.equal(g0[nm], g1[nm]) and torch.equal(g0[nm], g2[nm]) for nm in g0)
    # labels / mask None with a threshold that lets every pixel through
    out = fused.gradient_features(*inputs, None, None, labelled=[0] * n, threshold=-1.0, return_pseudo_pixels=True)
    assert out[2].tolist() == [side.up * side.up * h * w] * n and bool(torch.isfinite(out[1]["Final.kernel"]).all())


HYPER = dict(learning_rate=5e-4, beta1=0.9, beta2=0.99, loginverse_scaling=1.02, l2=2e-4)


def _frames_case():
    x = syn.synth_frames_device(0, 2, 64, 128, 3)
    rng = np.random.default_rng(21)
    labels = rng.integers(0, 19, (2, 64, 128)).astype(np.uint8)
    mask = (rng.uniform(size=(2, 64, 128)) > 0.2).astype(np.float32)
    labels[1], mask[1] = 0xFF, np.nan  # image 1 is unlabelled
    return x, torch.as_tensor(labels).cuda(), torch.as_tensor(mask).cuda(), torch.tensor([True, False]).cuda()


def _composed_step(side, net, tr, x, x_raw, labels, mask, sel, measure, thr, conf):
    """features(images), the model layers, score_logits, training_targets, the parent's plain step, the confusion op"""
    f = tr.features(x)
    f = f if isinstance(f, tuple) else (f,)
    fr = None
    if x_raw is not None:
        fr = tr.features(x_raw)
        fr = fr if isinstance(fr, tuple) else (fr,)
    lab, mk, c, pp, _ = _yardstick_targets(side, net, net.classes, f, fr, labels, mask, sel.cpu().numpy(), measure, thr)
    conf += c
    return tr.step(x, lab, mk), pp


def _packed_equal(tr_a, tr_b, step):
    for (nm, va, _, _), (_, vb, _, _) in zip(tr_a._named(), tr_b._named()):
        assert np.array_equal(va.numpy(), vb.numpy()), "%s differs at step %d" % (nm, step)
    sa, sb = tr_a.state, tr_b.state
    assert sa["t"] == sb["t"] and set(sa["m"]) == set(sb["m"])
    for nm in sa["m"]:
        assert np.array_equal(sa["m"][nm], sb["m"][nm]) and np.array_equal(sa["v"][nm], sb["v"][nm]), \
            "Adam slots of %s differ at step %d" % (nm, step)


@pytest.mark.parametrize("stage", (False, True), ids=("block", "stage"))
def test_image_entry_end_to_end_ten_steps(stage):
    """10 fused steps on one ENet(19), 10 composed steps on its twin at 2 x 64 x 128: variables, m, v, loss, confusion and
    pseudo pixels equal after every step; net.score equal afterwards; the moving statistics untouched"""
    side = STAGE if stage else BLOCK
    net_a, _ = make_model(19, 3, seed=0)
    net_b, _ = make_model(19, 3, seed=0)
    x, labels, mask, sel = _frames_case()
    tr_a, tr_b = side.fused_cls(net_a, **HYPER), side.parent_cls(net_b, **HYPER)
    tr_a.reinitialize(seed=5)
    tr_b.reinitialize(seed=5)
    stats = {(blk, a): getattr(getattr(net_a, blk), a).numpy().copy() for blk in (lbo.BLOCK, lso.STAGE) for a in lso.STATS}
    _, p = net_b.score(x, "entropy", 0.0, return_confidence=True)
    thr = float(np.median(p["confidence"][1].float().cpu().numpy()))
    conf_a = torch.zeros((19, 19), dtype=torch.int64, device="cuda")
    conf_b = torch.zeros_like(conf_a)
    for step in range(10):
        la, ppa = tr_a.step(x, labels, mask, labelled=sel, measure="entropy", threshold=thr, confusion=conf_a,
                            return_pseudo_pixels=True)
        lb, ppb = _composed_step(side, net_b, tr_b, x, None, labels, mask, sel, "entropy", thr, conf_b)
        print("step %2d: loss %.12g / %.12g, pseudo pixels %s" % (step, float(la), float(lb), ppa.tolist()))
        assert float(la).hex() == float(lb).hex(), "loss differs at step %d" % step
        _packed_equal(tr_a, tr_b, step)
        assert torch.equal(ppa, ppb) and ppa[0].item() == 0
        assert torch.equal(conf_a, conf_b), "confusion differs at step %d" % step
    assert 0 < ppa[1].item() < 64 * 128
    s_a, e_a = net_a.score(x, return_label=True)
    s_b, e_b = net_b.score(x, return_label=True)
    assert torch.equal(s_a, s_b) and torch.equal(e_a["label"], e_b["label"])
    for (blk, a), v in stats.items():
        assert np.array_equal(getattr(getattr(net_a, blk), a).numpy(), v), "%s.%s was written" % (blk, a)
    # the state is the parent class's: it loads into it and back
    tr_c = side.parent_cls(net_b, **HYPER)
    tr_c.load_state(tr_a.state)
    tr_a.load_state(tr_c.state)
    _packed_equal(tr_a, tr_c, 10)


@pytest.mark.parametrize("stage", (False, True), ids=("block", "stage"))
def test_images_raw_against_composition(stage):
    """images_raw differing from the training frames (a channel-scaled copy, as InputStage's image_dist); images_raw is
    images == images_raw=None; with_raw grows the image entries' workspace"""
    side = STAGE if stage else BLOCK
    net_a, _ = make_model(19, 3, seed=0)
    net_b, _ = make_model(19, 3, seed=0)
    x_raw, labels, mask, sel = _frames_case()
    x = (x_raw * torch.tensor([0.9, 1.1, 0.8], device="cuda")).contiguous()
    tr_a, tr_b = side.fused_cls(net_a, **HYPER), side.parent_cls(net_b, **HYPER)
    _, p = net_b.score(x_raw, "margin", 0.0, return_confidence=True)
    thr = float(np.median(p["confidence"][1].float().cpu().numpy()))
    conf_a = torch.zeros((19, 19), dtype=torch.int64, device="cuda")
    conf_b = torch.zeros_like(conf_a)
    for step in range(3):
        la, ppa = tr_a.step(x, labels, mask, labelled=sel, measure="margin", threshold=thr, images_raw=x_raw,
                            confusion=conf_a, return_pseudo_pixels=True)
        lb, ppb = _composed_step(side, net_b, tr_b, x, x_raw, labels, mask, sel, "margin", thr, conf_b)
        assert float(la).hex() == float(lb).hex(), "loss differs at step %d" % step
        _packed_equal(tr_a, tr_b, step)
        assert torch.equal(ppa, ppb) and torch.equal(conf_a, conf_b)
    net_c, _ = make_model(19, 3, seed=0)
    net_d, _ = make_model(19, 3, seed=0)
    tr_c, tr_d = side.fused_cls(net_c, **HYPER), side.fused_cls(net_d, **HYPER)
    lc = tr_c.step(x, labels, mask, labelled=sel, threshold=0.3, images_raw=x)
    ld = tr_d.step(x, labels, mask, labelled=sel, threshold=0.3)
    assert float(lc).hex() == float(ld).hex()
    _packed_equal(tr_c, tr_d, 0)
    L = _lib.lib()
    h_ = tr_c._trunk_handle()
    q = L.ssal_enet_train_stage_semi_workspace_bytes if stage else L.ssal_enet_train_block_semi_workspace_bytes
    plain = L.ssal_enet_train_stage_workspace_bytes if stage else L.ssal_enet_train_block_workspace_bytes
    assert q(h_, 2, 64, 128, 1) - q(h_, 2, 64, 128, 0) >= 2 * 64 * 128  # one byte per output pixel
    assert q(h_, 2, 64, 128, 0) >= plain(h_, 2, 64, 128)


@pytest.mark.parametrize("stage", (False, True), ids=("block", "stage"))
def test_full_size_batch_matches_composition(stage):
    """one batch whose half-resolution map is 8 x 256 x 512 (1024 tiles), K = 19, entropy, four images unlabelled"""
    side = STAGE if stage else BLOCK
    k, labelled = 19, [1, 0, 1, 0, 0, 1, 0, 1]
    n, h, w = (8, 128, 256) if stage else (8, 256, 512)
    net = _net(k)
    rng = np.random.default_rng(7 + int(stage))
    inputs = side.inputs(rng, n, h, w)
    labels, mask = _annotation(rng, n, side.up * h, side.up * w, k, labelled)
    lab, mk, wconf, wpp, thr = _yardstick_targets(side, net, k, inputs, None, labels, mask, labelled, "entropy")
    parent = side.parent_cls(net, 1e-3, loginverse_scaling=1.02)
    fused = side.fused_cls(net, 1e-3, loginverse_scaling=1.02)
    wloss, wgrads = parent.gradient_features(*inputs, lab, mk)
    got = _fused(side, fused, inputs, None, labels, mask, labelled, "entropy", thr, k)
    _assert_same("full size", got, (wloss, wgrads, wconf, wpp))


def test_c_statuses_on_device():
    """the C entries: OK, NULL planes with no labelled image, unknown measure, short workspace, raw features without indices"""
    k = 19
    L = _lib.lib()
    x = torch.as_tensor((np.random.default_rng(3).standard_normal((2, 8, 8, 16)) * 0.7).astype(np.float32)).cuda()
    lab = torch.zeros((2, 16, 16), dtype=torch.uint8, device="cuda")
    msk = torch.ones((2, 16, 16), device="cuda")
    params = torch.as_tensor(SemiSupervisedBlockTrainer(_net(k), 1e-3)._pack()).cuda()
    loss = torch.zeros(1, dtype=torch.float64, device="cuda")
    grad = torch.zeros(params.numel(), device="cuda")
    ws = torch.zeros(int(L.ssal_train_block_grad_semi_workspace_bytes(2, 8, 8, k, 1)), dtype=torch.uint8, device="cuda")
    lbd = torch.zeros(2, dtype=torch.uint8, device="cuda")
    pp = torch.zeros(2, dtype=torch.int64, device="cuda")

    # threshold -1: every pixel of the (all unlabelled) batch passes, so sum(mask) > 0 and the gradient is finite; at
    # threshold 2 none passes, the counts are 0 and the gradient is 0 * (1 / 0), as in the plain entry under an all-zero mask
    def call(classes=k, measure=0, labels=_lib.dev_ptr(lab), labelled=_lib.dev_ptr(lbd), raw=None, ws_bytes=ws.numel(),
             threshold=-1.0):
        return L.ssal_train_block_grad_semi_nhwc(_lib.dev_ptr(x), raw, 2, 8, 8, classes, _lib.dev_ptr(params), labels,
                                                 _lib.dev_ptr(msk) if labels else None, labelled, measure, threshold, 0.0, 0.0,
                                                 _lib.dev_ptr(loss), _lib.dev_ptr(grad), None, _lib.dev_ptr(pp),
                                                 _lib.dev_ptr(ws), ws_bytes, _lib.stream_ptr())

    assert call(threshold=2.0) == _lib.SSAL_OK
    assert pp.tolist() == [0, 0]
    assert call() == _lib.SSAL_OK
    assert call(labels=None) == _lib.SSAL_OK
    assert pp.tolist() == [256, 256] and bool(torch.isfinite(grad).all())
    grad.fill_(float("nan"))
    assert call(raw=_lib.dev_ptr(x)) == _lib.SSAL_OK
    assert call(classes=33) == _lib.SSAL_EINVAL and b"classes must be in [2,32]" in L.ssal_last_error()
    assert call(measure=3) == _lib.SSAL_ENOTIMPL and b"Uncertainty function not implemented" in L.ssal_last_error()
    assert call(labels=None, labelled=None) == _lib.SSAL_EINVAL and b"may be NULL only" in L.ssal_last_error()
    assert call(ws_bytes=15) == _lib.SSAL_ENOMEM and b"workspace too small" in L.ssal_last_error()
    torch.cuda.synchronize()
    assert pp.tolist() == [256, 256] and bool(torch.isfinite(grad).all())  # the refused calls wrote nothing


def test_semi_entries_with_nothing_semi_equal_the_plain_entries():
    """the six semi C entries called with labelled = confusion = pseudo_pixels = NULL and no raw input give the loss and the
    gradient of their plain siblings bit for bit: ENet(6), 2 frames of 32 x 48 (feature maps 16 x 24 and 8 x 12: two
    16 x 16 tiles with a ragged edge on the stage's map), about 10 % of the mask zero"""
    k, n, h, w = 6, 2, 32, 48
    L = _lib.lib()
    net, _ = make_model(k, 3, seed=0)
    x = syn.synth_frames_device(0, n, h, w, 3)
    rng = np.random.default_rng(12)
    labels = torch.as_tensor(rng.integers(0, k, (n, h, w)).astype(np.uint8)).cuda()
    mask = torch.as_tensor((rng.uniform(size=(n, h, w)) > 0.1).astype(np.float32)).cuda()
    assert 0.05 <= float((mask == 0).float().mean()) <= 0.15
    net(x, training=False)
    f51 = net.endpoint_outputs[0][1].clone()
    block, stage = LastBlockTrainer(net, 1e-3), LastStageTrainer(net, 1e-3)
    f50 = block.features(x)
    f42, am = stage.features(x)
    assert tuple(f51.shape) == tuple(f50.shape) == (n, 16, 24, 16) and tuple(f42.shape) == (n, 8, 12, 64)
    kern = torch.as_tensor(net.Final.kernel.numpy()).cuda().contiguous()
    pb, ps = torch.as_tensor(block._pack()).cuda(), torch.as_tensor(stage._pack()).cuda()
    handle = net._sync_handle()
    p, u8 = _lib.dev_ptr, 0
    semi = (None, 0, 0.5)  # labelled, measure, threshold
    wl = (1.02, 0.1)  # loss weight, label smoothing
    # depth -> (gradient floats,
    #           features side: plain entry, its leading arguments, semi entry, its leading arguments, dims, parameters,
    #                          max_workgroups or nothing, workspace query, semi workspace query,
    #           images side: plain entry, semi entry, parameters, max_workgroups or nothing, the two workspace queries)
    depths = {
        "final": (kern.numel(),
                  (L.ssal_final_grad_nhwc, (p(f51),), L.ssal_final_grad_semi_nhwc, (p(f51), None), (n, 16, 24, k), p(kern), (),
                   L.ssal_final_grad_workspace_bytes, lambda *a: L.ssal_final_grad_semi_workspace_bytes(*a)),
                  (L.ssal_enet_train_final_nhwc, L.ssal_enet_train_final_semi_nhwc, p(kern), (),
                   L.ssal_enet_train_final_workspace_bytes, L.ssal_enet_train_final_semi_workspace_bytes)),
        "block": (pb.numel(),
                  (L.ssal_train_block_grad_nhwc, (p(f50),), L.ssal_train_block_grad_semi_nhwc, (p(f50), None), (n, 16, 24, k),
                   p(pb), (), L.ssal_train_block_grad_workspace_bytes,
                   lambda *a: L.ssal_train_block_grad_semi_workspace_bytes(*a, 0)),
                  (L.ssal_enet_train_block_nhwc, L.ssal_enet_train_block_semi_nhwc, p(pb), (),
                   L.ssal_enet_train_block_workspace_bytes, L.ssal_enet_train_block_semi_workspace_bytes)),
        "stage": (ps.numel(),
                  (L.ssal_train_stage_grad_nhwc, (p(f42), p(am)), L.ssal_train_stage_grad_semi_nhwc,
                   (p(f42), p(am), None, None), (n, 8, 12, k), p(ps), (0,), L.ssal_train_stage_grad_workspace_bytes,
                   lambda *a: L.ssal_train_stage_grad_semi_workspace_bytes(*a, 0)),
                  (L.ssal_enet_train_stage_nhwc, L.ssal_enet_train_stage_semi_nhwc, p(ps), (0,),
                   L.ssal_enet_train_stage_workspace_bytes, L.ssal_enet_train_stage_semi_workspace_bytes)),
    }

    def run(entry, nbytes, args):
        """args(loss, grad, ws) -> the entry's argument tuple; fresh NaN-filled outputs and workspace per call"""
        assert nbytes > 0
        ws = torch.zeros(int(nbytes), dtype=torch.uint8, device="cuda")
        loss = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
        grad = torch.full((floats,), float("nan"), device="cuda")
        assert entry(*args(loss, grad, ws)) == _lib.SSAL_OK, L.ssal_last_error()
        torch.cuda.synchronize()
        return loss, grad

    for name, (floats, feat, img) in depths.items():
        plain, head, semi_entry, semi_head, dims, params, extra, query, semi_query = feat
        tail = lambda loss, grad, ws: (p(ws), ws.numel(), _lib.stream_ptr())
        l0, g0 = run(plain, query(*dims), lambda loss, grad, ws: head + dims + (params, p(labels), p(mask)) + wl
                     + extra + (p(loss), p(grad)) + tail(loss, grad, ws))
        l1, g1 = run(semi_entry, semi_query(*dims), lambda loss, grad, ws: semi_head + dims + (params, p(labels), p(mask))
                     + semi + wl + extra + (p(loss), p(grad), None, None) + tail(loss, grad, ws))
        print("%s features: loss %.17g / %.17g" % (name, float(l0.cpu()[0]), float(l1.cpu()[0])))
        assert bool(torch.isfinite(l0).all()) and bool(torch.isfinite(g0).all())
        assert torch.equal(l0, l1) and torch.equal(g0, g1), "%s: features entries differ" % name
        plain, semi_entry, params, extra, query, semi_query = img
        l2, g2 = run(plain, query(handle, n, h, w), lambda loss, grad, ws: (handle, p(x), u8, n, h, w, p(labels), p(mask),
                     params) + wl + extra + (p(loss), p(grad)) + tail(loss, grad, ws))
        l3, g3 = run(semi_entry, semi_query(handle, n, h, w, 0), lambda loss, grad, ws: (handle, p(x), None, u8, n, h, w,
                     p(labels), p(mask)) + semi + (params,) + wl + extra + (p(loss), p(grad), None, None)
                     + tail(loss, grad, ws))
        print("%s images:   loss %.17g / %.17g" % (name, float(l2.cpu()[0]), float(l3.cpu()[0])))
        assert bool(torch.isfinite(l2).all()) and bool(torch.isfinite(g2).all())
        assert torch.equal(l2, l3) and torch.equal(g2, g3), "%s: images entries differ" % name
