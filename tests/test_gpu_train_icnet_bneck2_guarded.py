"""ICNet's deep bottleneck trainer on poisoned workspaces and guarded outputs (tests/guarded_alloc.py under its three byte
patterns; DESIGN.md sections 31 and 43): the gradient and step entries, from features and from frames, give the bits of a clean
run and leave every guard intact."""
import numpy as np
import pytest
import torch

import semanticsegmentationactivelearning_amd as ssal
from semanticsegmentationactivelearning_amd import synthetic as syn, training

import icnet_bneck2_train_oracle as b2
import test_gpu_train_icnet_bneck2 as t2
from guarded_alloc import same_bits
from helpers import frames
from test_gpu_guarded import AL_PARAMS, _train_planes, _trained, guarded

pytestmark = pytest.mark.gpu


def test_features_entries_on_the_ragged_case():
    """``gradient_features`` and one ``step_features`` at the gradient test's ragged shape (2, 5, 9): the last 64-pixel tile of the
    new kernel and the last tiles of the link's matrix-core kernels are ragged, as is the last split-K group of the three weight
    gradients, and conv5_2's backward runs in the pieces conv5_3's left behind.  The features entries allocate their workspace
    themselves, so the loss and the gradients are interiors of guarded slabs"""
    k = 19
    x, c31, c3, d, labels, mask = b2.case(8000 + 14, 2, 5, 9, k)

    def make():
        net = t2._net(k)
        t2._assign(net, d)
        t2._assign_stats(net, b2.draw_stats(t2.STAT_SEED))
        return net

    def body(put):
        net = put.adopt(make())
        tr = training.ICNetDeepBottleneckTrainer(net, 1e-3, loginverse_scaling=1.02, label_smoothing=0.1)
        put.fresh()
        loss, grads = tr.gradient_features(put(x), put(c31), put(c3), put(labels), put(mask), max_workgroups=2)
        out = {"loss": loss}
        out.update({"g:" + n: v for n, v in grads.items()})
        put.fresh()
        out["~step_loss"] = tr.step_features(put(x), put(c31), put(c3), put(labels), put(mask), max_workgroups=2)
        torch.cuda.synchronize()
        out.update(_trained(tr))
        return out
    got = guarded(body, clean=True, tag="ICNetDeepBottleneckTrainer ragged")
    assert np.isfinite(got["loss"]).all() and same_bits(got["loss"].ravel()[:1], got["step_loss"].ravel()[:1])
    assert all(np.abs(got["g:" + n]).max() > 0 for n in b2.BLOCK)
    assert all(np.isfinite(v).all() for n, v in got.items() if n.startswith("g:") or n.startswith("w:"))


def test_images_entries_from_frames():
    """``gradient(images)`` and one ``step(images)`` on 2 x 64 x 128 frames, a fresh model per run: the trunk's workspace, which
    also holds the call's pieces behind the forward workspace, must come from the patch"""
    x = frames([0, 1], 64, 128, 3)
    labels, mask = _train_planes(2, 64, 128)

    def body(put):
        net = ssal.ICNet(19)
        net.build((None, None, None, 3))
        syn.randomize_icnet(net, seed=0)
        net = put.adopt(net)
        tr = training.ICNetDeepBottleneckTrainer.from_params(net, AL_PARAMS)
        put.fresh()
        loss, grads = tr.gradient(put(x), put(labels), put(mask))
        assert put.g is None or put.g.is_guarded(net._ws), "the trunk's workspace did not come from the patch"
        out = {"loss": loss}
        out.update({"g:" + n: v for n, v in grads.items()})
        put.fresh()
        out["~step_loss"] = tr.step(put(x), put(labels), put(mask))
        torch.cuda.synchronize()
        out.update(_trained(tr))
        return out
    got = guarded(body, clean=True, tag="ICNetDeepBottleneckTrainer images")
    assert np.isfinite(got["loss"]).all() and same_bits(got["loss"].ravel()[:1], got["step_loss"].ravel()[:1])
    assert all(np.abs(got["g:" + n]).max() > 0 for n in b2.BLOCK)
