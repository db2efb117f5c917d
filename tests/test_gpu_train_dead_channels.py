"""Dead channels on the MI355X: the derivative of PReLU at exactly 0 as the four training kernel files use it (dprelu of
csrc/ssal_train_common.h, inlined into each block kernel).  A trained network's dead channels -- batch-norm gamma = beta = 0 -- put +0 into
their PReLU at every pixel; the reference's PReLU, relu(x) - alpha relu(-x), has derivative 0 there, so every gradient entry that
belongs to such a channel is exactly 0.0.  A rule that said ``v >= 0 ? 1 : a`` would push a spurious d beta into Adam.  The
float64 oracle's half is test_train_dead_channels_cpu.py; the data is class_count_cases.dead_decoder_case (K = 19, a3_8
1 x 3 x 9, projection channel 1 and convolution channel 2 dead in all five trained blocks, the moving statistics random).

The last block alone is also compared with float64 under lbo.tolerance: class_count_cases.DEAD_BLOCK_SEED = 300, the first seed
>= 300 by the recipe of test_gpu_train_decoder.py whose margin over the PReLU inputs of the live channels exceeds 24 (133.6 on
the search host, float64 against float32 torch on the CPU; asserted > 16)."""
import numpy as np
import pytest
import torch

from semanticsegmentationactivelearning_amd.tensortools import losses
from semanticsegmentationactivelearning_amd.training import (DecoderTailTrainer, DecoderTrainer, DeepTailTrainer, LastBlockTrainer,
                                                             LastStageTrainer)

import class_count_cases as cc
import decoder_tail_train_oracle as dto
import decoder_train_oracle as dco
import deep_tail_train_oracle as ddo
import last_block_train_oracle as lbo
import last_stage_train_oracle as lso
import test_gpu_train_block as train_block
import test_gpu_train_decoder as train_decoder

pytestmark = pytest.mark.gpu

K, WEIGHT, SMOOTHING = 19, 1.02, 0.1


def _check_trainer(who, loss, g, names, blocks, want_loss, shared=None):
    """the loss bit for bit, the dead entries of every block the trainer trains exactly 0, every entry finite, the gradients
    shared with the longer trainer bit-identical"""
    assert set(g) == set(names), who
    got = float(loss.cpu()[0])
    assert got == want_loss, "%s: loss %r != forward op %r" % (who, got, want_loss)
    host = {nm: g[nm].cpu().numpy() for nm in names}
    entries = cc.dead_decoder_entries(blocks)
    assert len(entries) == 9 * len(blocks)
    count = cc.assert_dead_entries_zero(who, host, entries)
    for nm in names:
        assert np.isfinite(host[nm]).all(), "%s: %s is not finite" % (who, nm)
        assert (host[nm] != 0).any(), "%s: %s is zero everywhere" % (who, nm)
    if shared is not None:
        for nm in names:
            assert torch.equal(g[nm], shared[nm]), "%s: %s differs from DecoderTrainer's" % (who, nm)
    print("%-20s %2d blocks, %5d entries exactly 0, loss %.17g" % (who, len(blocks), count, got))
    return host


def test_dead_channels_give_exactly_zero_gradients_in_every_trainer():
    """DecoderTrainer on a3_8, then DeepTailTrainer, DecoderTailTrainer, LastStageTrainer and LastBlockTrainer on the model's own
    intermediate activations (the <false> instantiations of the chained kernels)"""
    x, am2, am1, labels, mask, params, stats = cc.dead_decoder_case(K)
    net = train_decoder._net_with(K, params, stats)
    xd, a2d, a1d = torch.as_tensor(x).cuda(), torch.as_tensor(am2).cuda(), torch.as_tensor(am1).cuda()
    a40 = net.Bottleneck4_0(xd, a2d, training=False)
    a41 = net.Bottleneck4_1(a40, training=False)
    a42 = net.Bottleneck4_2(a41, training=False)
    a50 = net.Bottleneck5_0(a42, a1d, training=False)
    logits = net.Final(net.Bottleneck5_1(a50, training=False), training=False)
    want_loss = float(losses.masked_softmax_cross_entropy(torch.as_tensor(labels).cuda(), logits, torch.as_tensor(mask).cuda(), K,
                                                          WEIGHT, SMOOTHING))
    kw = dict(loginverse_scaling=WEIGHT, label_smoothing=SMOOTHING)
    order = [b for b, _, _ in cc.decoder_blocks()]  # the last block first
    loss, g = DecoderTrainer(net, 1e-3, **kw).gradient_features(xd, a2d, a1d, labels, mask)
    _check_trainer("DecoderTrainer", loss, g, dco.NAMES, order, want_loss)
    runs = ((DeepTailTrainer, (a40, a1d), ddo.NAMES, order[:4]), (DecoderTailTrainer, (a41, a1d), dto.NAMES, order[:3]),
            (LastStageTrainer, (a42, a1d), lso.NAMES, order[:2]), (LastBlockTrainer, (a50,), lbo.NAMES, order[:1]))
    for cls, inputs, names, blocks in runs:
        ls_, gs = cls(net, 1e-3, **kw).gradient_features(*inputs, labels, mask)
        _check_trainer(cls.__name__, ls_, gs, names, blocks, want_loss, shared=g)
    torch.cuda.synchronize()
    # the oracle at the GPU's logits agrees on the zeros (asserted on the host without a GPU, too)
    _, g64, _ = dco.loss_and_grads(x, am2, am1, params, stats, labels, mask, WEIGHT, SMOOTHING, logits32=logits.cpu().numpy())
    cc.assert_dead_entries_zero("float64 oracle", g64, cc.dead_decoder_entries())


def test_last_block_with_dead_channels_matches_float64():
    """LastBlockTrainer on a5_0 1 x 12 x 36 with dead channels in Bottleneck5_1: all 13 gradients within lbo.tolerance of
    float64 (the dead entries are 0 on both sides), the loss equal to the forward op's bit for bit"""
    x, labels, mask, params, stats = cc.dead_block_case(K)
    margin = cc.block_margin(x, params, stats, dead=True)
    assert margin > 16.0, "the chosen data does not meet the condition on the live PReLU inputs (margin %.1f)" % margin
    net = train_block._net_with(K, params, stats)
    xd = torch.as_tensor(x).cuda()
    logits = net.Final(net.Bottleneck5_1(xd, training=False), training=False)
    want_loss = float(losses.masked_softmax_cross_entropy(torch.as_tensor(labels).cuda(), logits, torch.as_tensor(mask).cuda(), K,
                                                          WEIGHT, SMOOTHING))
    loss, g = LastBlockTrainer(net, 1e-3, loginverse_scaling=WEIGHT, label_smoothing=SMOOTHING).gradient_features(xd, labels, mask)
    torch.cuda.synchronize()
    host = _check_trainer("LastBlockTrainer", loss, g, lbo.NAMES, [lbo.BLOCK], want_loss)
    _, g64, smallest = lbo.loss_and_grads(x, params, stats, labels, mask, WEIGHT, SMOOTHING, logits32=logits.cpu().numpy())
    assert smallest == 0.0
    _, g32, _ = lbo.loss_and_grads(x, params, stats, labels, mask, WEIGHT, SMOOTHING, dtype=torch.float32)
    tol = lbo.tolerance(g32, g64)
    ratios = {nm: float(np.abs(host[nm].astype(np.float64) - g64[nm]).max()) / tol[nm] for nm in lbo.NAMES}
    for nm in lbo.NAMES:
        print("%-32s ratio %.3f, max |g64| %.3e" % (nm, ratios[nm], np.abs(g64[nm]).max()))
    print("margin over the live PReLU inputs %.1f, worst ratio %.3f" % (margin, max(ratios.values())))
    bad = [nm for nm in lbo.NAMES if not ratios[nm] <= 1.0]
    assert not bad, "beyond max(8 e_ref, 2^-22 max |g64|): %s" % bad
