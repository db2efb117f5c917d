"""Dead channels on the host: the float64 oracles give exactly 0.0 at every gradient entry that belongs to a channel whose
batch-norm has gamma = beta = 0, because the reference's PReLU, relu(x) - alpha relu(-x) (models/util/extra_ops.py:9-26), has
derivative 0 at 0.  test_gpu_train_dead_channels.py asserts the same of the four kernel files' own copies of that rule; this
file is the reference's half, and shows that the data would expose a copy that said ``v >= 0 ? 1 : a``."""
import numpy as np
import torch

import class_count_cases as cc
import decoder_train_oracle as dco
import last_block_train_oracle as lbo

WEIGHT, SMOOTHING = 1.02, 0.1


def _decoder_grads():
    x, am2, am1, labels, mask, params, stats = cc.dead_decoder_case()
    return dco.loss_and_grads(x, am2, am1, params, stats, labels, mask, WEIGHT, SMOOTHING)


def test_decoder_oracle_is_exactly_zero_at_the_dead_entries():
    """all five trained blocks at K = 19, a3_8 1 x 3 x 9: the listed entries == 0, every entry finite, and the dead channels
    are a strict part of each tensor (the rest carries a gradient)"""
    loss, g, pre = _decoder_grads()
    entries = cc.dead_decoder_entries()
    assert len(entries) == 5 * 9
    count = cc.assert_dead_entries_zero("float64 oracle", g, entries)
    print("loss %.12g: %d gradient entries exactly 0, %d PReLU inputs exactly 0 of %d" % (loss, count, int((pre == 0).sum()), pre.size))
    assert np.isfinite(loss) and all(np.isfinite(g[nm]).all() for nm in dco.NAMES)
    assert (pre == 0).any()
    for nm in entries:
        assert (g[nm] != 0).any(), "%s is zero everywhere: the case shows nothing" % nm
    # the convolution kernel's two index sets are the right way round: an entry outside both carries a gradient
    for blk, shapes, up in cc.decoder_blocks():
        gk = g["%s.conv_kernel" % blk]
        assert gk.shape == shapes["conv_kernel"]
        live = np.ones(gk.shape, bool)
        for idx in entries["%s.conv_kernel" % blk]:
            live[idx] = False
        assert (gk[live] != 0).all() or (gk[live] != 0).mean() > 0.99, blk


def test_a_derivative_of_one_at_zero_would_show(monkeypatch):
    """the same data under PReLU restated with derivative 1 at 0 (x >= 0 ? x : alpha x): the dead projection channel's beta
    gets a gradient in every block.  So the exact-zero assertions tell the two rules apart"""
    monkeypatch.setattr(lbo, "prelu", lambda x, alpha: torch.where(x >= 0, x, alpha * x))
    _, g, _ = _decoder_grads()
    for blk, _, _ in cc.decoder_blocks():
        assert g["%s.proj_beta" % blk][cc.DEAD_PROJ] != 0, blk
        assert g["%s.conv_beta" % blk][cc.DEAD_CONV] != 0, blk


def test_dead_block_seed_meets_the_prelu_condition_and_oracle_zeros():
    """DEAD_BLOCK_SEED: over the PReLU inputs of the channels that are not dead, the smallest float64 |input| exceeds 16 x the
    largest |fp32 - float64| deviation; the last block's oracle is exactly 0 at the dead entries"""
    x, labels, mask, params, stats = cc.dead_block_case()
    assert x.shape == (1, 12, 36, 16)
    margin = cc.block_margin(x, params, stats, dead=True)
    print("dead block seed %d: margin over the live channels %.1f" % (cc.DEAD_BLOCK_SEED, margin))
    assert margin > 16.0
    _, g, smallest = lbo.loss_and_grads(x, params, stats, labels, mask, WEIGHT, SMOOTHING)
    assert smallest == 0.0
    cc.assert_dead_entries_zero("float64 oracle", g, cc.dead_entries(lbo.BLOCK, lbo.SHAPES, False))
    assert all(np.isfinite(g[nm]).all() for nm in lbo.NAMES)
