"""The reference side of the class-count sweep (test_gpu_class_counts.py) checked on the host at every K, so that a failure on
the MI355X points at the kernel: the C oracle's score against the independent torch restatement for K = 2 .. 32 on the sweep's
own logits; the block head's seed against the condition on its PReLU inputs; the float64 restatement of the output-layer step
(final_train_oracle) against plain torch autograd at class counts that are not multiples of 4."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import enet_oracle as orc
from oracle import torch_restatement as tr

import class_count_cases as cc
import final_train_oracle as fto
from helpers import report_diff


@pytest.mark.parametrize("k", cc.CLASS_COUNTS)
def test_oracle_score_matches_torch_restatement_at_every_class_count(k):
    """orc.score_logits (C, the sweep's yardstick) against active_learning.py:239-263 restated on stock torch ops, on the
    sweep's logits: labels equal (the all-tie pixel included: the first maximum); confidences within 1e-5, the bound
    test_score_matches_literal_numpy holds the oracle to (two fp32 evaluations of a softmax over <= 32 terms and of a log per
    term: a few 2^-24 each); the float64 means within 1e-6"""
    lg = cc.sweep_logits(k)
    assert lg.shape == (2, 3, 5, k)
    for measure in cc.MEASURES:
        mean, conf, label = orc.score_logits(lg, measure)
        wmean, wconf, wlabel = tr.score_logits(lg, measure)
        report_diff("K=%d %s label" % (k, measure), label, wlabel)
        assert label[0, 0, 0] == 0
        report_diff("K=%d %s confidence" % (k, measure), conf, wconf, exact=False, atol=1e-5)
        report_diff("K=%d %s mean" % (k, measure), mean, wmean, exact=False, atol=1e-6)


def test_block_head_seed_meets_the_prelu_condition():
    """BLOCK_SEED: the smallest |PReLU input| of Bottleneck5_1's float64 forward exceeds 16 x the largest |fp32 - float64|
    deviation there.  The block's forward does not depend on K: one evaluation covers the 31 cases"""
    x, params, stats = cc.block_inputs()
    assert x.shape == (2, 3, 17, 16)
    margin = cc.block_margin(x, params, stats)
    print("block head seed %d: margin %.1f" % (cc.BLOCK_SEED, margin))
    assert margin > 16.0
    for k in (2, 32):  # only Final.kernel, the labels and the mask change with K
        xk, _, _, pk, sk = cc.block_case(k)
        assert np.array_equal(xk, x) and all(np.array_equal(pk[nm], params[nm]) for nm in params)
        assert all(np.array_equal(sk[a], stats[a]) for a in stats) and pk["Final.kernel"].shape == (3, 3, k, 16)


def _plain_autograd(x, kern, labels, mask, weight, ls):
    """float64 (loss, dL/dW) from stock torch ops alone: conv_transpose2d, log_softmax, softmax.  Holds where every label
    under mask 1 is a class (sum(y) = 1), where TensorFlow's softmax - y is the derivative of the value"""
    k = kern.shape[2]
    on, off, w32, c_w = fto.xent_constants(k, weight, ls)
    w = torch.as_tensor(kern.astype(np.float64)).requires_grad_(True)
    xt = torch.as_tensor(x.astype(np.float64)).permute(0, 3, 1, 2)
    n, h, ww = x.shape[:3]
    # [kh, kw, K, C] -> torch's [C_in, K_out, kh, kw]; SAME at stride 2 keeps the first 2h x 2w of the full output
    lg = F.conv_transpose2d(xt, w.permute(3, 2, 0, 1), stride=2)[:, :, :2 * h, :2 * ww].permute(0, 2, 3, 1)
    lab = torch.as_tensor(labels.astype(np.int64))
    y = torch.full(lg.shape, off, dtype=torch.float64)
    y.scatter_(-1, lab.clamp(max=k - 1)[..., None], on)
    mk = torch.as_tensor(mask.astype(np.float64))
    ce = -(y * F.log_softmax(lg, -1)).sum(-1) * mk
    if w32 > 1.0:
        ce = ce / torch.log(w32 + c_w * (F.softmax(lg, -1) * y).sum(-1))
    loss = ce.sum() / float(np.float32(mask.astype(np.float64).sum()))
    loss.backward()
    return float(loss.detach()), w.grad.numpy()


@pytest.mark.parametrize("k", (5, 29, 30, 31))
@pytest.mark.parametrize("weight,ls", cc.LOSSES)
def test_final_oracle_matches_plain_autograd(k, weight, ls):
    """fto.loss_and_grad (einsum transposed convolution, logsumexp, TensorFlow's gradient written out) against stock torch
    ops in float64.  Both are float64 sums of fewer than 10^4 terms of magnitude <= 1: they agree to 10^4 x 2^-53 ~ 1e-12 of
    the largest entry.  Pixels whose label is no class carry mask 0 here (there TensorFlow's gradient is not the value's).
    With label smoothing the fp32 constants give sum(y) = 1 + eps, |eps| ~ 1e-8, and TensorFlow's softmax - y differs from the
    value's derivative sum(y) softmax - y by eps s mask w softmax_k per pixel: at most |eps| C_j after the contraction, C the
    magnitude bound of fto.grad_and_bound (its A_{p,k} >= s mask w softmax_k).  Without smoothing eps is exactly 0."""
    x, kern, labels, mask = cc.final_case(k)
    mask = np.where(labels >= k, np.float32(0.0), mask)
    assert (labels >= k).any() and mask.sum() > 100
    loss, g = fto.loss_and_grad(x, kern, labels, mask, weight, ls)
    wloss, wg = _plain_autograd(x, kern, labels, mask, weight, ls)
    d = float(np.abs(g - wg).max())
    print("K=%d w=%g ls=%g: loss %.17g / %.17g, max |dg| %.3e of %.3e" % (k, weight, ls, loss, wloss, d, np.abs(wg).max()))
    assert g.shape == wg.shape == (3, 3, k, 16)
    assert abs(loss - wloss) <= 1e-12 * abs(wloss)
    on, off, w32, c_w = fto.xent_constants(k, weight, ls)
    eps = abs(on + (k - 1) * off - 1.0)
    assert (eps == 0.0) == (ls == 0.0) and eps < 1e-7
    lg = fto.conv2d_transpose_3x3_s2(torch.as_tensor(x.astype(np.float64)), torch.as_tensor(kern.astype(np.float64)))
    g2, c, _ = fto.grad_and_bound(x, kern, labels, mask, weight, ls, lg.numpy())
    assert np.abs(g2 - g).max() <= 1e-12 * float(np.abs(wg).max())  # one image at a time: the same gradient
    bad = np.abs(g - wg) > 1e-12 * float(np.abs(wg).max()) + eps * c
    assert not bad.any(), "%d entries beyond 1e-12 max |g| + |sum(y) - 1| C" % int(bad.sum())
    # and the loss is pixel_loss / mask_scale, the pair the loss op's sweep is compared with
    pl = fto.pixel_loss(lg, fto.one_hot(labels, k, on, off), torch.as_tensor(mask.astype(np.float64)), w32, c_w)
    assert abs(float(pl.sum()) * fto.mask_scale(mask) - wloss) <= 1e-12 * abs(wloss)


@pytest.mark.parametrize("k", cc.CLASS_COUNTS)
def test_loss_case_holds_the_labels_the_sweep_names(k):
    """label 255 under both mask values, exactly one label == K and that under mask 1, a mixed mask"""
    lg, labels, mask = cc.loss_case(k)
    assert lg.shape == (2, 6, 10, k)
    assert ((labels == 255) & (mask == 1)).any() and ((labels == 255) & (mask == 0)).any()
    assert int((labels == k).sum()) == 1 and mask[labels == k].tolist() == [1.0]
    assert 0.1 < float((mask == 0).mean()) < 0.5
