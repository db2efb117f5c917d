"""Validation metrics on the host (no GPU): tensortools.metrics.create_metrics against an independent restatement of the
reference's Metrics._create_metrics (tensortools/metrics.py:155-224), the accumulate / reset semantics of Metrics, and a
world-size-2 gloo run of active_learning.all_reduce_confusion (one collective per pass, every rank gets the sum)."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from semanticsegmentationactivelearning_amd import tensortools as tt
from semanticsegmentationactivelearning_amd.tensortools import metrics as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("TruePositive", "TrueNegative", "FalsePositive", "FalseNegative", "ClassAccuracy", "ClassPrecission",
        "ClassRecall", "ClassMeanIoU", "PixelAccuracy", "MeanIoU", "ConfusionMat")


def _restated(cm):
    """metrics.py:155-224 restated element by element (explicit loops, float64)"""
    cm = np.asarray(cm, dtype=np.int64)
    k = cm.shape[0]
    tot = int(cm.sum())
    out = {key: [] for key in KEYS[:8]}
    for c in range(k):
        tp = int(cm[c, c])
        fp = int(sum(cm[r, c] for r in range(k) if r != c))
        fn = int(sum(cm[c, q] for q in range(k) if q != c))
        tn = tot - (tp + fp + fn)
        out["TruePositive"].append(tp)
        out["TrueNegative"].append(tn)
        out["FalsePositive"].append(fp)
        out["FalseNegative"].append(fn)
        out["ClassAccuracy"].append((tp + tn) / tot if tot else float("nan"))
        out["ClassPrecission"].append(tp / max(tp + fp, 1))
        out["ClassRecall"].append(tp / max(tp + fn, 1))
        out["ClassMeanIoU"].append(tp / max(tp + fp + fn, 1))
    out = {key: np.array(v) for key, v in out.items()}
    out["PixelAccuracy"] = (int(np.trace(cm)) / tot) if tot else float("nan")
    out["MeanIoU"] = float(np.sum(out["ClassMeanIoU"]) / k)
    return out


def _matrices():
    rng = np.random.default_rng(7)
    for k in (2, 3, 19, 32):
        yield k, rng.integers(0, 1000, size=(k, k))
        m = rng.integers(0, 50, size=(k, k))
        m[0, :] = 0
        m[:, 0] = 0  # class 0 absent: TP + FP + FN = 0
        if k > 2:
            m[1, 1] = 0  # class 1 never right
        yield k, m
        yield k, np.diag(rng.integers(0, 10 ** 9, size=k))
    yield 5, np.zeros((5, 5), dtype=np.int64)


@pytest.mark.parametrize("k,cm", list(_matrices()))
def test_create_metrics_matches_restatement(k, cm):
    got = M.create_metrics(cm)
    want = _restated(cm)
    assert set(got) == set(KEYS)
    np.testing.assert_array_equal(got["ConfusionMat"], cm)
    for key in ("TruePositive", "TrueNegative", "FalsePositive", "FalseNegative"):
        assert got[key].dtype == np.int64
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    for key in ("ClassAccuracy", "ClassPrecission", "ClassRecall", "ClassMeanIoU", "PixelAccuracy", "MeanIoU"):
        np.testing.assert_allclose(got[key], want[key], rtol=1e-15, atol=0, equal_nan=True, err_msg=key)


def test_create_metrics_quirks():
    cm = np.array([[5, 1, 0], [0, 0, 0], [2, 0, 3]])
    m = M.create_metrics(torch.as_tensor(cm))
    # class 1 never labelled and never right: IoU 0, and MeanIoU still averages over all three classes
    assert m["ClassMeanIoU"][1] == 0.0
    assert m["MeanIoU"] == pytest.approx((5 / 8 + 0 + 3 / 5) / 3, rel=1e-15)
    assert m["PixelAccuracy"] == pytest.approx(8 / 11, rel=1e-15)
    empty = M.create_metrics(np.zeros((2, 2), dtype=np.int64))
    assert np.isnan(empty["PixelAccuracy"]) and empty["MeanIoU"] == 0.0


def test_metrics_accumulate_and_reset():
    rng = np.random.default_rng(3)
    a, b = rng.integers(0, 100, size=(4, 4)), rng.integers(0, 100, size=(4, 4))
    acc = tt.Metrics(4)
    np.testing.assert_array_equal(acc.confusion, np.zeros((4, 4)))
    acc.add(a)
    acc.add(torch.as_tensor(b, dtype=torch.int32))
    np.testing.assert_array_equal(acc.confusion, a + b)
    np.testing.assert_array_equal(acc.metrics["ConfusionMat"], a + b)
    np.testing.assert_array_equal(acc.batch_metrics["ConfusionMat"], b)
    assert acc.metrics["MeanIoU"] == pytest.approx(_restated(a + b)["MeanIoU"], rel=1e-15)
    acc.reset()
    np.testing.assert_array_equal(acc.confusion, np.zeros((4, 4)))
    np.testing.assert_array_equal(acc.batch_metrics["ConfusionMat"], np.zeros((4, 4)))
    acc.add(b)
    np.testing.assert_array_equal(acc.confusion, b)
    with pytest.raises(ValueError):
        acc.add(np.zeros((3, 3), dtype=np.int64))
    with pytest.raises(ValueError):
        acc.add(np.zeros((4, 4), dtype=np.float32))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_matrix(rank, k):
    return np.random.default_rng(100 + rank).integers(0, 1 << 40, size=(k, k))


def _worker(rank, world, port, k, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    from semanticsegmentationactivelearning_amd import active_learning as al
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        calls = []
        orig = dist.all_reduce

        def counting(*a, **kw):
            calls.append("all_reduce")
            return orig(*a, **kw)
        names = ("all_gather_into_tensor", "all_gather", "broadcast", "reduce", "barrier")
        saved = {nm: getattr(dist, nm) for nm in names}
        for nm in names:
            setattr(dist, nm, lambda *a, _nm=nm, **kw: (calls.append(_nm), saved[_nm](*a, **kw))[1])
        dist.all_reduce = counting
        try:
            mine = torch.as_tensor(_rank_matrix(rank, k))
            total = al.all_reduce_confusion(mine)
        finally:
            dist.all_reduce = orig
            for nm in names:
                setattr(dist, nm, saved[nm])
        np.testing.assert_array_equal(mine.numpy(), _rank_matrix(rank, k))  # the caller's matrix is left alone
        np.save(os.path.join(out_dir, "r%d.npy" % rank), total.numpy())
        with open(os.path.join(out_dir, "calls%d.txt" % rank), "w") as f:
            f.write(",".join(calls))
    finally:
        dist.destroy_process_group()


def test_all_reduce_confusion_gloo_world2(tmp_path):
    k, world = 19, 2
    mp.spawn(_worker, args=(world, _free_port(), k, str(tmp_path)), nprocs=world, join=True)
    want = sum(_rank_matrix(r, k) for r in range(world))
    for r in range(world):
        np.testing.assert_array_equal(np.load(tmp_path / ("r%d.npy" % r)), want)
        assert (tmp_path / ("calls%d.txt" % r)).read_text() == "all_reduce"


def test_all_reduce_confusion_without_group_is_identity():
    from semanticsegmentationactivelearning_amd import active_learning as al
    c = torch.arange(9, dtype=torch.int64).view(3, 3)
    assert al.all_reduce_confusion(c) is c
