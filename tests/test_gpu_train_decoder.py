"""Decoder training on the MI355X: the 63 gradients of Bottleneck4_0, Bottleneck4_1, Bottleneck4_2,
Bottleneck5_0, Bottleneck5_1 and Final.kernel against the float64 oracle with the tolerance measured from the reference
arithmetic's own error; the loss against the forward op and the deep tail's 50 gradients against DeepTailTrainer, bit for bit;
determinism; Adam bit for bit against the float32 restatement; the weights of record after three steps; the semi-supervised
step against the composed one; a short end-to-end run; the C entries' statuses."""
import numpy as np
import pytest
import torch

import semanticsegmentationactivelearning_amd as ssal
from semanticsegmentationactivelearning_amd import _lib
from semanticsegmentationactivelearning_amd import active_learning as al
from semanticsegmentationactivelearning_amd import synthetic as syn
from semanticsegmentationactivelearning_amd.tensortools import losses, metrics
from semanticsegmentationactivelearning_amd.training import DecoderTrainer, DeepTailTrainer, SemiSupervisedDecoderTrainer

import decoder_tail_train_oracle as dto
import decoder_train_oracle as dco
import deep_tail_train_oracle as ddo
import final_train_oracle as fto
import last_block_train_oracle as lbo
import last_stage_train_oracle as lso
from helpers import frames, make_model

pytestmark = pytest.mark.gpu

AL_PARAMS = {"hyperparams": {"learning_rate": 0.0005, "learning_rate_decay": 0.0,
                             "optimizer": {"type": "Adam", "kwargs": {"beta1": 0.9, "beta2": 0.99}},
                             "weight_reg": {"L2": 0.0002, "L1": 0.0},
                             "softmax": {"label_smoothing": 0.0, "loginverse_scaling": 1.02, "multiscale": False}}}
BLOCKS = ((lbo.BLOCK, lbo.BLOCK_VARS), (lso.STAGE, lso.STAGE_VARS), (dto.TAIL, dto.TAIL_VARS), (ddo.DEEP, ddo.DEEP_VARS),
          (dco.LOW, dco.LOW_VARS))

CASES = [(k, weight, ls) for k in (2, 19, 32) for weight in (0.0, 1.02) for ls in (0.0, 0.1)]
# seeds for which the ORACLE ALONE (float64 against float32 torch on the CPU) meets the condition on the inputs: the smallest
# |PReLU input| of the float64 forward, over all 15 PReLUs, exceeds 16 x the largest |fp32 - float64| deviation there
# (decoder_train_oracle: prelu_inputs / prelu_margin on _case's x, pooling indices and parameters; the forward does not depend
# on the loss' weight or smoothing; the GPU's results play no part).  Recipe: try 300, 301, ... and keep the first seed whose
# ratio exceeds 24; if there is none below 40 000, the first whose ratio exceeds 19; if there is none either, a smaller shape.
# (A seed whose smallest float64 |input| is below 4.5e-5 was not run in float32: it would need a deviation below 2.4e-6 to
# reach 19, and the smallest deviation seen at any of these shapes is 2.6e-6.)  Ratios on the search host / the MI355X host:
#   1 x 5 x 6     K = 2 / 19 / 32: 1798, 4151, 3000 (29.0 / 25.7, 24.5 / 19.7, 24.9 / 20.0), each the first above 24
#   2 x 5 x 9     no seed in [300, 40 000) reaches 19 for any K: the best are 8.9 / 15.7 / 10.4.  Shrunk to
#   2 x 3 x 9     two images, two tiles of Bottleneck4_0's kernels, three rows, ragged both ways.  K = 32: 19494, the first above
#                 24 (24.3 / 27.6).  K = 19: none above 24 below 40 000; 18910 is the first above 19 (21.2 / 20.1).
#                 K = 2: none above 19 below 40 000 (best 18.5); shrunk again to
#   2 x 1 x 9     K = 2: 303, the first above 24 (45.7 / 50.4); the kernels of Bottleneck4_0 do not depend on K
#   1 x 5 x 17    (max_workgroups = 2) no seed in [300, 40 000) reaches 19: the best is 15.9.  Shrunk to
#   1 x 3 x 17    three tiles of Bottleneck4_0's kernels, ten of the tail's, on two workgroups: 29726, the first above 24
#                 (27.6 / 21.8)
#   1 x 9 x 3     an extra case, nine rows: a tile boundary in the vertical direction.  328, the first above 24 (28.1 / 22.4)
# The fp32 deviation is the host CPU's (torch's float32 kernels differ between instruction sets), and the ratio of one seed
# moves by up to a third between hosts.
SEEDS = {((1, 5, 6), 2): 1798, ((1, 5, 6), 19): 4151, ((1, 5, 6), 32): 3000, ((2, 1, 9), 2): 303, ((2, 3, 9), 19): 18910,
         ((2, 3, 9), 32): 19494, ((1, 3, 17), 19): 29726, ((1, 9, 3), 19): 328}


def _shape(idx, k):
    return (1, 5, 6) if (idx // 2 + idx) % 2 == 0 else ((2, 1, 9) if k == 2 else (2, 3, 9))


def _case(seed, n, h, w, k):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, h, w, 128)) * 0.7).astype(np.float32)
    am2 = dco.random_argmax(rng, n, h, w, 64)
    am1 = dco.random_argmax(rng, n, 2 * h, 2 * w, 16)
    labels = rng.integers(0, k, (n, 8 * h, 8 * w)).astype(np.uint8)
    mask = (rng.uniform(size=(n, 8 * h, 8 * w)) > 0.25).astype(np.float32)
    labels[rng.uniform(size=labels.shape) < 0.05] = 255  # label 255 under both mask values
    params, stats = dco.random_params(seed + 1000, k)
    return x, am2, am1, labels, mask, params, stats


def _net_with(k, params, stats):
    net = ssal.ENet(k)
    net.build((None, None, None, 3))
    net.Final.kernel.assign(params["Final.kernel"])
    for blk, names in BLOCKS:
        for a in names:
            getattr(getattr(net, blk), a).assign(params["%s.%s" % (blk, a)])
        for a in dco.STATS:
            getattr(getattr(net, blk), a).assign(stats[blk][a])
    return net


def _check_case(name, n, h, w, k, weight, ls, max_workgroups=0):
    x, am2, am1, labels, mask, params, stats = _case(SEEDS[((n, h, w), k)], n, h, w, k)
    net = _net_with(k, params, stats)
    tr = DecoderTrainer(net, 1e-3, loginverse_scaling=weight, label_smoothing=ls)
    xd, a2d, a1d = torch.as_tensor(x).cuda(), torch.as_tensor(am2).cuda(), torch.as_tensor(am1).cuda()
    loss, g = tr.gradient_features(xd, a2d, a1d, labels, mask, max_workgroups=max_workgroups)
    loss2, g2 = tr.gradient_features(xd, a2d, a1d, labels, mask, max_workgroups=max_workgroups)
    torch.cuda.synchronize()
    assert set(g) == set(dco.NAMES)
    assert torch.equal(loss, loss2) and all(torch.equal(g[nm], g2[nm]) for nm in g), "two calls differ"
    # the forward the scoring path computes: the six layers of the model
    a40 = net.Bottleneck4_0(xd, a2d, training=False)
    a42 = net.Bottleneck4_2(net.Bottleneck4_1(a40, training=False), training=False)
    logits = net.Final(net.Bottleneck5_1(net.Bottleneck5_0(a42, a1d, training=False), training=False), training=False)
    want = losses.masked_softmax_cross_entropy(torch.as_tensor(labels).cuda(), logits, torch.as_tensor(mask).cuda(), k,
                                               weight, ls)
    got_loss, want_loss = float(loss.cpu()[0]), float(want)
    print("%s: loss %.17g, forward op %.17g" % (name, got_loss, want_loss))
    assert got_loss == want_loss, "loss %r != forward op %r" % (got_loss, want_loss)
    # the prefix is the deep tail: the other 50 gradients are DeepTailTrainer's on the model's own a4_0, bit for bit
    lt, gt = DeepTailTrainer(net, 1e-3, loginverse_scaling=weight, label_smoothing=ls).gradient_features(
        a40, a1d, labels, mask, max_workgroups=max_workgroups)
    assert torch.equal(lt, loss)
    for nm in ddo.NAMES:
        assert torch.equal(gt[nm], g[nm]), "%s differs from DeepTailTrainer's" % nm
    logits32 = logits.cpu().numpy()
    _, g64, _ = dco.loss_and_grads(x, am2, am1, params, stats, labels, mask, weight, ls, logits32=logits32)
    _, _, pre64 = dco.loss_and_grads(x, am2, am1, params, stats, labels, mask, weight, ls)
    _, g32, pre32 = dco.loss_and_grads(x, am2, am1, params, stats, labels, mask, weight, ls, dtype=torch.float32)
    margin = dco.prelu_margin(pre64, pre32)
    print("%s: smallest |PReLU input| %.3e = %.1f x the largest fp32 deviation" % (name, np.abs(pre64).min(), margin))
    assert margin > 16.0, "the chosen data does not meet the condition on the PReLU inputs"
    tol = dco.tolerance(g32, g64)
    worst = {}
    for nm in dco.NAMES:
        d = float(np.abs(g[nm].cpu().numpy().astype(np.float64) - g64[nm]).max())
        worst[nm] = d / tol[nm]
        print("%s: %-32s max |g - g64| %.3e, tolerance %.3e, ratio %.3f, max |g64| %.3e"
              % (name, nm, d, tol[nm], worst[nm], np.abs(g64[nm]).max()))
    bad = [nm for nm in dco.NAMES if not worst[nm] <= 1.0]
    assert not bad, "%s: beyond max(8 e_ref, 2^-22 max |g64|): %s" % (name, bad)


@pytest.mark.parametrize("k,weight,ls", CASES)
def test_gradients_match_float64_oracle(k, weight, ls):
    """max |g_gpu - g64| <= max(8 e_ref, 2^-22 max |g64|) per tensor, e_ref = max |g32 - g64| of float32 torch autograd of the
    same restatement; a3_8 1 x 5 x 6 and 2 x 3 x 9 (2 x 1 x 9 at K = 2; odd: the maps are ragged against the 8 x 8 tiles at both
    resolutions, and the second shape puts two tiles of Bottleneck4_0's kernels under the loop over the images), alternated so that, for every
    K, each shape meets both weights and both smoothing values"""
    idx = CASES.index((k, weight, ls))
    n, h, w = _shape(idx, k)
    _check_case("K=%d w=%g ls=%g %dx%dx%d" % (k, weight, ls, n, h, w), n, h, w, k, weight, ls)


def test_gradients_more_tiles_than_workgroups():
    """a3_8 1 x 3 x 17: three 8 x 8 tiles of Bottleneck4_0's kernels (and ten of the tail's) on 2 workgroups"""
    _check_case("3x17 on 2 workgroups", 1, 3, 17, 19, 1.02, 0.0, max_workgroups=2)


def test_gradients_across_a_vertical_tile_boundary():
    """a3_8 1 x 9 x 3: two tiles of Bottleneck4_0's kernels one above the other, so the halo row above a tile, the taps that
    reach into it and the row below a tile meet the oracle with data in them"""
    _check_case("9x3", 1, 9, 3, 19, 1.02, 0.1)


def test_adam_bit_identical_and_regulariser_ranges():
    """three step_features calls: every w, m, v of the 63 trained variables equals final_train_oracle.adam_step fed with the
    GPU's own gradient; l1 / l2 only on the variables the reference regularises; the 30 statistics and every other variable
    of the model are unchanged"""
    k = 19
    x, am2, am1, labels, mask, params, stats = _case(31, 2, 6, 10, k)
    params["Final.kernel"][0, 0, :3, :] = 0.0  # exact zeros: sign(0) = 0
    params["Bottleneck4_0.res_kernel"][0, 0, :4, :] = 0.0
    net = _net_with(k, params, stats)
    before = {v.name: v.numpy().copy() for v in net.variables}
    tr = DecoderTrainer(net, 5e-4, 0.9, 0.99, l1=1e-4, l2=2e-4, loginverse_scaling=1.02)
    xd, a2d, a1d = torch.as_tensor(x).cuda(), torch.as_tensor(am2).cuda(), torch.as_tensor(am1).cuda()
    w = {nm: np.array(params[nm]) for nm in dco.NAMES}
    m = {nm: np.zeros_like(w[nm]) for nm in dco.NAMES}
    v = {nm: np.zeros_like(w[nm]) for nm in dco.NAMES}
    b1p, b2p = np.float32(0.9), np.float32(0.99)
    var_of = lambda nm: net.Final.kernel if nm == "Final.kernel" else getattr(getattr(net, nm.split(".")[0]), nm.split(".")[1])
    for step in range(3):
        _, g = tr.gradient_features(xd, a2d, a1d, labels, mask)
        tr.step_features(xd, a2d, a1d, labels, mask)
        st = tr.state
        for nm in dco.NAMES:
            reg = nm in dco.REGULARISED
            w[nm], m[nm], v[nm] = fto.adam_step(w[nm], m[nm], v[nm], g[nm].cpu().numpy(), np.float32(5e-4), 0.9, 0.99, 1e-8,
                                                b1p, b2p, l1=1e-4 if reg else 0.0, l2=2e-4 if reg else 0.0)
            assert np.array_equal(st["m"][nm], m[nm]), "m of %s differs at step %d" % (nm, step)
            assert np.array_equal(st["v"][nm], v[nm]), "v of %s differs at step %d" % (nm, step)
            assert np.array_equal(var_of(nm).numpy(), w[nm]), "%s differs at step %d" % (nm, step)
        b1p, b2p = np.float32(b1p * np.float32(0.9)), np.float32(b2p * np.float32(0.99))
    assert tr.state["t"] == 3
    for blk, _ in BLOCKS:
        for a in dco.STATS:
            assert np.array_equal(getattr(getattr(net, blk), a).numpy(), stats[blk][a])
    trained = {var_of(nm).name for nm in dco.NAMES}
    changed = {vv.name for vv in net.variables if not np.array_equal(vv.numpy(), before[vv.name])}
    assert changed == trained, "changed %s, trained %s" % (sorted(changed ^ trained), len(trained))


def _frames_case():
    x = syn.synth_frames_device(0, 2, 64, 128, 3)
    rng = np.random.default_rng(9)
    labels = rng.integers(0, 19, (2, 64, 128)).astype(np.uint8)
    mask = (rng.uniform(size=(2, 64, 128)) > 0.2).astype(np.float32)
    return x, labels, mask


def test_image_entry_matches_features_and_weights_of_record():
    """step(images) == step_features(*features(images)); after three steps net(x) and net.score(x) use the new weights
    (bit-identical to the C oracle with the host variables); everything outside the trained variables is unchanged"""
    from oracle import enet_oracle as orc
    net, _ = make_model(19, 3, seed=0)
    twin, _ = make_model(19, 3, seed=0)
    x, labels, mask = _frames_case()
    before = {v.name: v.numpy().copy() for v in net.variables}
    trained = {"Final/Kernel"} | {getattr(getattr(net, blk), a).name for blk, names in BLOCKS for a in names}
    tr = DecoderTrainer.from_params(net, AL_PARAMS)
    tw = DecoderTrainer.from_params(twin, AL_PARAMS)
    feats, am2, am1 = tw.features(x)
    assert tuple(feats.shape) == (2, 8, 16, 128) and tuple(am2.shape) == (2, 8, 16, 64) and tuple(am1.shape) == (2, 16, 32, 16)
    assert am2.dtype == torch.int64 and am1.dtype == torch.int64
    # Bottleneck3_8's output: the model's own Bottleneck4_0 turns it into the deep-tail trainer's features, bit for bit
    f40, am40 = DeepTailTrainer.from_params(twin, AL_PARAMS).features(x)
    assert torch.equal(twin.Bottleneck4_0(feats, am2, training=False), f40) and torch.equal(am1, am40)
    for step in range(3):
        la = tr.step(x, labels, mask)
        lb = tw.step_features(feats, am2, am1, labels, mask)
        assert float(la) == float(lb), "step %d: step(images) loss %r != step_features loss %r" % (step, float(la), float(lb))
    for nm, var, _, _ in tr._named():
        blk, a = nm.split(".")
        other = twin.Final.kernel if nm == "Final.kernel" else getattr(getattr(twin, blk), a)
        assert np.array_equal(var.numpy(), other.numpy()), nm
    changed = {v.name for v in net.variables if not np.array_equal(v.numpy(), before[v.name])}
    assert changed == trained, "written outside the trained variables: %s" % sorted(changed ^ trained)
    P = syn.enet_params_dict(net)
    want_mean, _, want_label, want_logits = orc.score_images(P, frames([0, 1], 64, 128, 3), "entropy")
    scores, ex = net.score(x, return_label=True)
    logits = net(x, training=False)
    torch.cuda.synchronize()
    assert np.array_equal(logits.cpu().numpy(), want_logits)
    assert np.array_equal(ex["label"].cpu().numpy(), want_label)
    assert np.abs(scores.cpu().numpy() - want_mean).max() <= 1e-6
    want = float(losses.masked_softmax_cross_entropy(torch.as_tensor(labels).cuda(), logits, torch.as_tensor(mask).cuda(), 19,
                                                     1.02, 0.0))
    assert float(tr.step(x, labels, mask)) == want
    # the images entry leaves Bottleneck3_8's output where ssal_enet_train_decoder_features_offset says
    off = _lib.lib().ssal_enet_train_decoder_features_offset(net._handle, 2, 64, 128)
    left = net._ws[off:off + 4 * feats.numel()].view(torch.float32).view(feats.shape)
    assert torch.equal(left, feats)


@pytest.mark.parametrize("with_raw", (False, True), ids=("training-logits", "images_raw"))
def test_semi_supervised_step_matches_composition(with_raw):
    """SemiSupervisedDecoderTrainer.step on 2 x 64 x 128 with image 1 unlabelled (0xFF labels and NaN masks in its planes)
    against the composed step on a twin: net.score's label / mask planes -> training_targets -> the plain step; the loss, the
    packed gradient (every variable's), the confusion matrix and the pseudo-pixel counts, bit for bit, over two steps"""
    net_a, _ = make_model(19, 3, seed=0)
    net_b, _ = make_model(19, 3, seed=0)
    x_raw, labels, mask = _frames_case()
    labels[1], mask[1] = 0xFF, np.nan
    labels, mask = torch.as_tensor(labels).cuda(), torch.as_tensor(mask).cuda()
    sel = torch.tensor([True, False]).cuda()
    x = (x_raw * torch.tensor([0.9, 1.1, 0.8], device="cuda")).contiguous() if with_raw else x_raw
    tr_a, tr_b = SemiSupervisedDecoderTrainer.from_params(net_a, AL_PARAMS), DecoderTrainer.from_params(net_b, AL_PARAMS)
    _, p = net_b.score(x_raw, "entropy", 0.0, return_confidence=True)
    thr = float(np.median(p["confidence"][1].float().cpu().numpy()))
    conf_a = torch.zeros((19, 19), dtype=torch.int64, device="cuda")
    conf_b = torch.zeros_like(conf_a)
    for step in range(2):
        la, ppa = tr_a.step(x, labels, mask, labelled=sel, measure="entropy", threshold=thr, confusion=conf_a,
                            return_pseudo_pixels=True, **({"images_raw": x_raw} if with_raw else {}))
        _, p = net_b.score(x_raw, "entropy", thr, return_label=True, return_mask=True)
        pl, pm = p["label"], p["mask"].float()
        lab, mk = al.training_targets(sel, labels, mask, pl, pm)
        _, pt = al.score_logits(net_b(x, training=False), "confidence", 0.0, return_label=True)  # the first maximum
        conf_b += metrics.confusion_mat(lab, pt["label"], 19, weights=mk)
        ppb = pm.to(torch.int64).sum(dim=(1, 2)) * (~sel).to(torch.int64)
        lb = tr_b.step(x, lab, mk)
        print("step %d: loss %.17g / %.17g, pseudo pixels %s" % (step, float(la), float(lb), ppa.tolist()))
        assert float(la).hex() == float(lb).hex(), "loss differs at step %d" % step
        ga, gb = tr_a._dev["grad"].cpu().numpy(), tr_b._dev["grad"].cpu().numpy()
        assert ga.shape == gb.shape and np.array_equal(ga.view(np.uint32), gb.view(np.uint32)), "gradients differ at step %d" % step
        assert torch.equal(ppa, ppb) and ppa[0].item() == 0 and 0 < ppa[1].item() < 64 * 128
        assert torch.equal(conf_a, conf_b), "confusion differs at step %d" % step
    for (nm, va, _, _), (_, vb, _, _) in zip(tr_a._named(), tr_b._named()):
        assert np.array_equal(va.numpy(), vb.numpy()), nm


def test_semi_features_entry_and_launch_table():
    """the semi-supervised features entry with the undistorted frame's own features and pooling indices against the images
    entry, bit for bit; with no semi keyword SemiSupervisedDecoderTrainer issues exactly DecoderTrainer's launches"""
    net_a, _ = make_model(19, 3, seed=0)
    net_b, _ = make_model(19, 3, seed=0)
    x_raw, labels, mask = _frames_case()
    x = (x_raw * torch.tensor([0.9, 1.1, 0.8], device="cuda")).contiguous()
    sel = torch.tensor([True, False]).cuda()
    tr_a, tr_b = SemiSupervisedDecoderTrainer.from_params(net_a, AL_PARAMS), SemiSupervisedDecoderTrainer.from_params(net_b, AL_PARAMS)
    f, a2, a1 = tr_a.features(x)
    fr, a2r, a1r = tr_a.features(x_raw)
    conf_a = torch.zeros((19, 19), dtype=torch.int64, device="cuda")
    conf_b = torch.zeros_like(conf_a)
    la, ppa = tr_a.step_features(f, a2, a1, labels, mask, labelled=sel, measure="entropy", threshold=0.5, features_raw=fr,
                                 argmax2_raw=a2r, argmax1_raw=a1r, confusion=conf_a, return_pseudo_pixels=True)
    lb, ppb = tr_b.step(x, labels, mask, labelled=sel, measure="entropy", threshold=0.5, images_raw=x_raw, confusion=conf_b,
                        return_pseudo_pixels=True)
    assert float(la).hex() == float(lb).hex() and torch.equal(ppa, ppb) and torch.equal(conf_a, conf_b)
    for (nm, va, _, _), (_, vb, _, _) in zip(tr_a._named(), tr_b._named()):  # the same gradient: the same step
        assert np.array_equal(va.numpy(), vb.numpy()), nm
    plain = DecoderTrainer.from_params(make_model(19, 3, seed=0)[0], AL_PARAMS)
    semi = SemiSupervisedDecoderTrainer.from_params(make_model(19, 3, seed=0)[0], AL_PARAMS)
    tables = []
    for tr in (plain, semi):
        tr.step_features(f, a2, a1, labels, mask)  # (the first call uploads the state)
        torch.cuda.synchronize()
        _lib.profile_collect()
        _lib.profile_enable(True)
        try:
            tr.step_features(f, a2, a1, labels, mask)
            torch.cuda.synchronize()
            prof = _lib.profile_collect()
        finally:
            _lib.profile_enable(False)
        tables.append({nm: r["launches"] for nm, r in prof.items()})
    print("launch table: %s" % tables[0])
    assert tables[0] == tables[1]
    assert tables[0]["k_td_block"] == 1 and tables[0]["k_td_res"] == 1 and tables[0]["k_td_finish"] == 1
    assert tables[0]["k_tt_block<dx>"] == 2 and "k_tt_block" not in tables[0]  # the lowest regular block writes dL/d a4_0


def test_end_to_end_decoder_learns():
    """section 15's setup: labels from the original head's argmax, reinitialize(0), 50 steps at the reference's settings: the
    final loss is at most 0.9 x the initial one (the project's condition); DeepTailTrainer's run on the same data and start is
    printed next to it"""
    out = {}
    for cls in (DeepTailTrainer, DecoderTrainer):
        net, _ = make_model(19, 3, seed=0)
        x = syn.synth_frames_device(0, 2, 64, 128, 3)
        _, extra = net.score(x, return_label=True)
        labels = extra["label"].clone()
        mask = torch.ones((2, 64, 128), dtype=torch.float32, device=x.device)
        tr = cls.from_params(net, AL_PARAMS)
        tr.reinitialize(seed=0)
        ls_ = [float(tr.step(x, labels, mask)) for _ in range(50)]
        out[cls.__name__] = ls_
        print("end to end, %s: loss %.6g -> %.6g (x%.3f)" % (cls.__name__, ls_[0], ls_[-1], ls_[-1] / ls_[0]))
    assert out["DecoderTrainer"][-1] <= 0.9 * out["DecoderTrainer"][0]


def test_invalid_arguments_on_device():
    """the statuses of the ten entries: classes 1 and 33, a too-small workspace (the deep tail's), NULL pointers, a bad
    measure, a lone raw pointer, a NULL net: refused without a launch (the outputs keep their bytes); the same arguments,
    valid, succeed"""
    L = _lib.lib()
    n, h, w, k = 1, 4, 4, 19
    rng = np.random.default_rng(0)
    x = torch.zeros((n, h, w, 128), device="cuda")
    am2 = torch.as_tensor(dco.random_argmax(rng, n, h, w, 64)).cuda()
    am1 = torch.as_tensor(dco.random_argmax(rng, n, 2 * h, 2 * w, 16)).cuda()
    lab = torch.zeros((n, 8 * h, 8 * w), dtype=torch.uint8, device="cuda")
    mk = torch.ones((n, 8 * h, 8 * w), device="cuda")
    params = torch.zeros((L.ssal_train_decoder_param_floats(32),), device="cuda")
    nbytes = L.ssal_train_decoder_grad_semi_workspace_bytes(n, h, w, 32, 1)
    ws = torch.zeros((nbytes,), dtype=torch.uint8, device="cuda")
    loss = torch.full((1,), 7.0, dtype=torch.float64, device="cuda")
    grad = torch.full_like(params, 7.0)
    lbd = torch.ones((n,), dtype=torch.uint8, device="cuda")
    P = _lib.dev_ptr

    def call(classes=k, ws_bytes=nbytes, xp=x, mw=0):
        return L.ssal_train_decoder_grad_nhwc(P(xp), P(am2), P(am1), n, h, w, classes, P(params), P(lab), P(mk), 0.0, 0.0, mw,
                                              P(loss), P(grad), P(ws), ws_bytes, _lib.stream_ptr())

    def semi_call(measure=0, raw=(None, None, None), ws_bytes=nbytes, classes=k):
        return L.ssal_train_decoder_grad_semi_nhwc(P(x), P(am2), P(am1), P(raw[0]), P(raw[1]), P(raw[2]), n, h, w, classes,
                                                   P(params), P(lab), P(mk), P(lbd), measure, 0.5, 0.0, 0.0, 0, P(loss), P(grad),
                                                   None, None, P(ws), ws_bytes, _lib.stream_ptr())
    assert call(classes=1) == _lib.SSAL_EINVAL and call(classes=33) == _lib.SSAL_EINVAL
    assert call(xp=None) == _lib.SSAL_EINVAL and call(mw=-1) == _lib.SSAL_EINVAL
    assert call(ws_bytes=L.ssal_train_decoder_grad_workspace_bytes(n, h, w, k) - 1) in (_lib.SSAL_EINVAL, _lib.SSAL_ENOMEM)
    assert call(ws_bytes=L.ssal_train_tail2_grad_workspace_bytes(n, 2 * h, 2 * w, k)) == _lib.SSAL_ENOMEM
    assert semi_call(classes=33) == _lib.SSAL_EINVAL
    assert semi_call(measure=3) == _lib.SSAL_ENOTIMPL
    assert semi_call(raw=(x, am2, None)) == _lib.SSAL_EINVAL and semi_call(raw=(None, am2, am1)) == _lib.SSAL_EINVAL
    assert semi_call(ws_bytes=16) == _lib.SSAL_ENOMEM
    args_img = (None, P(x), 0, 1, 64, 64, P(lab), P(mk), P(params), 0.0, 0.0, 0, P(loss), P(grad), P(ws), nbytes, None)
    assert L.ssal_enet_train_decoder_nhwc(*args_img) == _lib.SSAL_EINVAL
    assert L.ssal_enet_train_decoder_semi_nhwc(None, P(x), None, 0, 1, 64, 64, P(lab), P(mk), P(lbd), 0, 0.5, P(params), 0.0,
                                               0.0, 0, P(loss), P(grad), None, None, P(ws), nbytes, None) == _lib.SSAL_EINVAL
    net, _ = make_model(19, 3, seed=0)
    net(syn.synth_frames_device(0, 1, 64, 64, 3), training=False)  # commits the handle
    assert L.ssal_enet_train_decoder_workspace_bytes(net._handle, 1, 64, 60) == -1
    assert L.ssal_enet_train_decoder_semi_workspace_bytes(net._handle, 0, 64, 64, 0) == -1
    assert L.ssal_enet_train_decoder_features_offset(net._handle, 1, 60, 64) == -1
    assert 0 < L.ssal_enet_train_decoder_workspace_bytes(net._handle, 1, 64, 64) \
        < L.ssal_enet_train_decoder_semi_workspace_bytes(net._handle, 1, 64, 64, 1)
    assert L.ssal_enet_train_decoder_features_offset(net._handle, 1, 64, 64) > 0
    assert L.ssal_enet_train_decoder_nhwc(net._handle, P(x), 0, 1, 64, 60, P(lab), P(mk), P(params), 0.0, 0.0, 0, P(loss),
                                          P(grad), P(ws), nbytes, None) == _lib.SSAL_EINVAL
    torch.cuda.synchronize()
    assert float(loss[0]) == 7.0 and bool((grad == 7.0).all()) and not bool(ws.any())
    tr = DecoderTrainer(net, 1e-3)
    labn, mkn = np.zeros((1, 32, 32), np.uint8), np.ones((1, 32, 32), np.float32)
    with pytest.raises(ValueError):
        tr.gradient_features(x, am2[:, :, :2], am1, labn, mkn)  # argmax2 of another shape
    with pytest.raises(ValueError):
        tr.gradient_features(x, am2 + 64, am1, labn, mkn)  # a device tensor of indices outside their windows
    with pytest.raises(ValueError):
        tr.gradient_features(x, am2, am1, labn[:, :8], mkn)
    assert call() == _lib.SSAL_OK  # the same arguments, valid
    assert semi_call() == _lib.SSAL_OK
    torch.cuda.synchronize()
    assert bool((grad[:L.ssal_train_decoder_param_floats(k)] != 7.0).all())
