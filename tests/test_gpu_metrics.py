"""Validation metrics on the MI355X: the stand-alone confusion op (ssal_confusion_matrix) against numpy's bincount, the
fused evaluation pass (ENet.evaluate: argmax + confusion inside the Final kernel) against the C oracle's argmax and
against score(return_label=True) in every kernel form, ICNet.evaluate, and active_learning.evaluate over TFRecords."""
import numpy as np
import pytest
import torch

import semanticsegmentationactivelearning_amd as ssal
from semanticsegmentationactivelearning_amd import _lib
from semanticsegmentationactivelearning_amd import active_learning as al
from semanticsegmentationactivelearning_amd import synthetic as syn
from semanticsegmentationactivelearning_amd.tensortools import metrics as M

pytestmark = pytest.mark.gpu


def bincount(labels, pred, k, weights=None):
    """tf.math.bincount(k * label + pred, weights, minlength = maxlength = k * k), keys >= k * k dropped"""
    key = k * np.asarray(labels, dtype=np.int64).ravel() + np.asarray(pred, dtype=np.int64).ravel()
    w = None if weights is None else np.asarray(weights, dtype=np.int64).ravel()
    keep = key < k * k
    return np.bincount(key[keep], None if w is None else w[keep], minlength=k * k)[:k * k].astype(np.int64).reshape(k, k)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("k", [2, 3, 6, 19, 32])
@pytest.mark.parametrize("pixels", [1, 255, 257, (1 << 21) + 3])
def test_confusion_mat_equals_bincount(k, pixels):
    rng = np.random.default_rng(k * 1000 + pixels % 997)
    pred = rng.integers(0, k, size=pixels, dtype=np.uint8)
    lab = rng.integers(0, k, size=pixels, dtype=np.uint8)
    lab[rng.random(pixels) < 0.1] = 255           # void label with mask 1: dropped (key >= K*K)
    lab[rng.random(pixels) < 0.05] = min(k + 3, 254)  # labels >= K
    if pixels > 1000:
        lab[: pixels // 3] = pred[: pixels // 3]  # long runs on the diagonal (wave-level aggregation)
    w = rng.choice(np.array([0, 1, 7, 255], dtype=np.uint8), size=pixels)
    got = M.confusion_mat(_dev(lab), _dev(pred), k, weights=_dev(w))
    np.testing.assert_array_equal(got.cpu().numpy(), bincount(lab, pred, k, w))
    got1 = M.confusion_mat(_dev(lab), _dev(pred), k)  # NULL mask = weight 1
    np.testing.assert_array_equal(got1.cpu().numpy(), bincount(lab, pred, k))


def test_confusion_mat_accumulates_and_reps_are_invisible():
    k, n = 19, 100003
    rng = np.random.default_rng(5)
    pred, lab = rng.integers(0, k, size=n, dtype=np.uint8), rng.integers(0, k, size=n, dtype=np.uint8)
    start = rng.integers(0, 1 << 40, size=(k, k))
    out = _dev(start.astype(np.int64))
    M.confusion_mat(_dev(lab), _dev(pred), k, out=out)
    want = start + bincount(lab, pred, k)
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    assert _lib.get_knobs()["conf_reps"] == 8
    try:
        for reps in (1, 3, 64):
            _lib.set_knob("conf_reps", reps)
            got = M.confusion_mat(_dev(lab), _dev(pred), k)
            np.testing.assert_array_equal(got.cpu().numpy(), bincount(lab, pred, k))
    finally:
        _lib.set_knob("conf_reps", 8)
    acc = M.Metrics(k)
    acc.update(_dev(pred), _dev(lab))
    acc.update(_dev(pred), _dev(lab), _dev(np.ones(n, np.uint8)))
    np.testing.assert_array_equal(acc.confusion, 2 * bincount(lab, pred, k))


@pytest.fixture(scope="module")
def enet19():
    from helpers import make_model
    return make_model(19, 3, seed=0)


@pytest.fixture(scope="module")
def enet6():
    from helpers import make_model
    return make_model(6, 4, seed=1)


def _labels(n, h, w, k, seed):
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, k, size=(n, h, w), dtype=np.uint8)
    lab[rng.random((n, h, w)) < 0.1] = 255
    mask = (lab != 255).astype(np.uint8)
    return lab, mask


@pytest.mark.parametrize("which", ["k19c3", "k6c4"])
def test_enet_evaluate_equals_oracle_argmax(which, enet19, enet6):
    from oracle import enet_oracle as orc
    net, P = enet19 if which == "k19c3" else enet6
    k, c = (19, 3) if which == "k19c3" else (6, 4)
    h, w = 256, 512
    x_u8 = np.stack([syn.synth_frame_u8(f, h, w, c) for f in (3, 4)])
    x_f32 = syn.u8_to_f32(x_u8)
    want_label = orc.score_images(P, x_f32, "confidence")[2]
    lab, mask = _labels(2, h, w, k, seed=k)
    lab[0, :64] = want_label[0, :64]  # a band on the diagonal
    want = bincount(lab, want_label, k, mask)
    for x in (_dev(x_u8), _dev(x_f32)):
        got = net.evaluate(x, _dev(lab), _dev(mask))
        np.testing.assert_array_equal(got.cpu().numpy(), want)
    got = net.evaluate(_dev(x_f32), _dev(lab))  # mask None = weight 1 (label 255 dropped by its key)
    np.testing.assert_array_equal(got.cpu().numpy(), bincount(lab, want_label, k))


def _big_batch(net):
    n, h, w = 8, 1024, 2048
    x = syn.synth_frames_device(0, n, h, w, 3, dtype=torch.uint8)
    return x, n, h, w


def _check_schedule_equalities(net, x, n, h, w, k):
    """evaluate over the batch == bincount of score()'s labels == two halves == single frames, for labels equal to the
    predictions (worst contention) and for random labels"""
    _, extra = net.score(x, measure="entropy", return_label=True)
    pred = extra["label"].cpu().numpy()
    rng = np.random.default_rng(11)
    rand = rng.integers(0, k, size=pred.shape, dtype=np.uint8)
    rand[rng.random(pred.shape) < 0.1] = 255
    for lab in (pred, rand):
        mask = (lab != 255).astype(np.uint8)
        want = bincount(lab, pred, k, mask)
        lab_d, mask_d = _dev(lab), _dev(mask)
        np.testing.assert_array_equal(net.evaluate(x, lab_d, mask_d).cpu().numpy(), want)
        acc = torch.zeros((k, k), dtype=torch.int64, device="cuda")
        half = n // 2
        net.evaluate(x[:half], lab_d[:half], mask_d[:half], confusion=acc)
        net.evaluate(x[half:], lab_d[half:], mask_d[half:], confusion=acc)
        np.testing.assert_array_equal(acc.cpu().numpy(), want)
        acc.zero_()
        for i in range(n):
            net.evaluate(x[i:i + 1], lab_d[i:i + 1], mask_d[i:i + 1], confusion=acc)
        np.testing.assert_array_equal(acc.cpu().numpy(), want)
    return pred


def test_enet_evaluate_shipping_schedule_and_kernel_forms(enet19):
    net, _ = enet19
    x, n, h, w = _big_batch(net)
    assert _lib.get_knobs()["defaults"] == 1
    pred = _check_schedule_equalities(net, x, n, h, w, 19)
    try:
        _lib.set_knob("fuse_ends", 0)  # plain Final kernel (no Bottleneck5_1 inside)
        np.testing.assert_array_equal(_check_schedule_equalities(net, x, n, h, w, 19), pred)
    finally:
        _lib.set_knob("fuse_ends", 3)
    try:
        _lib.set_kernel_family(False)  # generic kernels everywhere
        np.testing.assert_array_equal(_check_schedule_equalities(net, x[:2], 2, h, w, 19), pred[:2])
    finally:
        _lib.set_kernel_family(True)
    assert _lib.get_knobs()["defaults"] == 1


def test_enet_evaluate_bf16x3_and_score_after_evaluate(enet19):
    net, _ = enet19
    n, h, w = 2, 512, 1024
    x = syn.synth_frames_device(20, n, h, w, 3, dtype=torch.uint8)
    before = net.score(x, measure="entropy").cpu().numpy()
    _, extra = net.score(x, measure="entropy", return_label=True, arithmetic="bf16x3")
    pred = extra["label"].cpu().numpy()
    lab, mask = _labels(n, h, w, 19, seed=2)
    lab[1] = pred[1]
    got = net.evaluate(x, _dev(lab), _dev(mask), arithmetic="bf16x3")
    np.testing.assert_array_equal(got.cpu().numpy(), bincount(lab, pred, 19, mask))
    after = net.score(x, measure="entropy").cpu().numpy()
    assert np.array_equal(before.view(np.uint64), after.view(np.uint64))


def test_icnet_evaluate_equals_score_labels():
    net = ssal.ICNet(19)
    net.build((None, None, None, 3))
    syn.randomize_icnet(net, seed=0)
    n, h, w = 2, 256, 512
    x = syn.synth_frames_device(0, n, h, w, 3)
    _, extra = net.score(x, measure="margin", return_label=True)
    pred = extra["label"].cpu().numpy()
    lab, mask = _labels(n, h, w, 19, seed=4)
    lab[0] = pred[0]
    got = net.evaluate(x, _dev(lab), _dev(mask))
    np.testing.assert_array_equal(got.cpu().numpy(), bincount(lab, pred, 19, mask))
    acc = _dev(np.ones((19, 19), np.int64))
    net.evaluate(x, _dev(lab), None, confusion=acc)
    np.testing.assert_array_equal(acc.cpu().numpy(), 1 + bincount(lab, pred, 19))


def test_active_learning_evaluate_over_tfrecords(tmp_path, enet19):
    from test_input_cpu import write_pool
    from semanticsegmentationactivelearning_amd.tensortools import InputStage
    net, _ = enet19
    write_pool(str(tmp_path), 5, 72, 136)
    stage = InputStage(input_shape=[64, 128], image_dtype=np.uint8)
    stage.add_dataset("val", str(tmp_path), batch_size=2)
    stage.init_iterator("val")
    batches = list(stage)
    got = al.evaluate(net, iter(batches), 19)
    want = np.zeros((19, 19), dtype=np.int64)
    for img, lab, mask in batches:
        _, extra = net.score(_dev(np.asarray(img)), measure="entropy", return_label=True)
        want += bincount(lab, extra["label"].cpu().numpy(), 19, mask)
    ref = M.create_metrics(want)
    assert set(got) == set(ref)
    for key in ref:
        np.testing.assert_array_equal(np.asarray(got[key]), np.asarray(ref[key]), err_msg=key)
