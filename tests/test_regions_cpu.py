"""Region-level acquisition, host side (no GPU): the shared reduction core behind the two region kernels run on the CPU
(``ssal_region_reduce_host``), the region grid and the error paths of the C ABI, ``select_regions`` against a brute-force
sort, the world-2 gloo merge of ``rank_regions`` and ``region_boxes``."""
import ctypes
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from semanticsegmentationactivelearning_amd import _lib
from semanticsegmentationactivelearning_amd import active_learning as al
from semanticsegmentationactivelearning_amd import inference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Both sides are float64 sums of at most 2^21 values in [0, 1] taken in different orders: they differ by at most
# n * 2^-53 relative = 2.4e-10; the bound asserted is 1e-9.
TOL = 1e-9


def _plane(n, h, w, seed):
    return np.random.default_rng(seed).random((n, h, w), dtype=np.float32)


def _block_means(plane, rh, rw):
    """numpy reference: float64 mean of every clipped rh x rw block, and the clipped pixel counts"""
    n, h, w = plane.shape
    ry, rx = -(-h // rh), -(-w // rw)
    mean = np.empty((n, ry, rx), dtype=np.float64)
    count = np.empty((ry, rx), dtype=np.int64)
    p64 = plane.astype(np.float64)
    for y in range(ry):
        for x in range(rx):
            blk = p64[:, y * rh:(y + 1) * rh, x * rw:(x + 1) * rw]
            count[y, x] = blk.shape[1] * blk.shape[2]
            mean[:, y, x] = blk.reshape(n, -1).sum(axis=1) / count[y, x]
    return mean, count


def _tile_sums(plane):
    """float64 sums of the 32 x 32 tiles of a plane (what the fused score pass keeps per workgroup)"""
    n, h, w = plane.shape
    ty, tx = -(-h // 32), -(-w // 32)
    out = np.zeros((n, ty, tx), dtype=np.float64)
    p64 = plane.astype(np.float64)
    for y in range(ty):
        for x in range(tx):
            out[:, y, x] = p64[:, 32 * y:32 * y + 32, 32 * x:32 * x + 32].reshape(n, -1).sum(axis=1)
    return out


@pytest.mark.parametrize("h,w,region", [
    (64, 128, (32, 32)),       # divides the frame
    (136, 264, (32, 32)),      # clipped last row and column
    (136, 264, (48, 20)),      # rh != rw, neither divides, rw a multiple of 4
    (70, 90, (7, 13)),         # odd sizes, rows not 16-byte aligned
    (24, 40, (1, 1)),          # 1 x 1 regions
    (40, 72, (64, 128)),       # a region larger than the frame
    (40, 72, (40, 72)),        # exactly the frame
    (16, 1100, (16, 600)),     # rows wider than one pass of the 64 lanes
    (1024, 2048, (1024, 2048)),  # 2^21 pixels in one region: the case the tolerance is derived for
])
def test_plane_form_matches_numpy(h, w, region):
    plane = _plane(1 if h * w > 100000 else 3, h, w, seed=h * 7 + w)
    got, counts = _lib.region_reduce_host(plane, h, w, region, form="plane")
    want, want_counts = _block_means(plane, *region)
    assert got.shape == want.shape
    assert np.array_equal(counts, want_counts)  # clipped pixel counts: exact
    d = np.abs(got - want).max()
    print("plane form %dx%d region %s: max |d| = %.3e" % (h, w, region, d))
    assert d <= TOL


@pytest.mark.parametrize("h,w,region", [
    (128, 256, (32, 32)),
    (128, 256, (64, 64)),
    (136, 264, (32, 32)),      # h / 2 = 68 is not a multiple of 16: the last tile row holds 8 pixel rows
    (136, 264, (64, 128)),
    (136, 264, (32, 128)),
    (1024, 2048, (1024, 2048)),
])
def test_tile_form_matches_numpy(h, w, region):
    plane = _plane(1 if h * w > 100000 else 2, h, w, seed=h + 3 * w)
    got, counts = _lib.region_reduce_host(_tile_sums(plane), h, w, region, form="tiles")
    want, want_counts = _block_means(plane, *region)
    assert np.array_equal(counts, want_counts)
    d = np.abs(got - want).max()
    print("tile form %dx%d region %s: max |d| = %.3e" % (h, w, region, d))
    assert d <= TOL


def test_tile_form_of_one_tile_is_the_tile_sum_over_the_count():
    """region 32: the mean is exactly tile / clipped count (no second summation)"""
    plane = _plane(1, 136, 264, seed=5)
    tiles = _tile_sums(plane)
    got, counts = _lib.region_reduce_host(tiles, 136, 264, 32, form="tiles")
    assert np.array_equal(got, tiles / counts[None].astype(np.float64))


def test_region_grid():
    assert _lib.region_grid(1024, 2048, 128) == (8, 16)
    assert _lib.region_grid(136, 264, (32, 128)) == (5, 3)
    assert _lib.region_grid(136, 264, (1, 1)) == (136, 264)
    assert _lib.region_grid(64, 64, (1000, 1000)) == (1, 1)
    for bad in ((0, 32), (32, 0), (-32, 32)):
        with pytest.raises(ValueError, match="region size must be positive"):
            _lib.region_grid(64, 64, bad)
    with pytest.raises(ValueError, match="bad dims"):
        _lib.region_grid(0, 64, 32)
    L = _lib.lib()
    ry = ctypes.c_int(0)
    assert L.ssal_region_grid(64, 64, 32, 32, ctypes.byref(ry), None) == _lib.SSAL_EINVAL


def _fused_entry(rh, rw, region_out):
    """the fused ENet entry with a NULL handle: the region arguments are judged before anything needs a device"""
    L = _lib.lib()
    return L.ssal_enet_score_regions_nhwc_arith(None, None, 0, 1, 128, 256, 0, 0.0, 0, rh, rw, None, region_out,
                                                None, None, None, None, 0, None)


def test_error_paths():
    L = _lib.lib()
    out = np.zeros(64, dtype=np.float64)
    out_p = out.ctypes.data_as(ctypes.c_void_p)
    # a region that is not a whole number of tiles on the fused ENet entry: the message names the rule
    for rh, rw in ((48, 32), (32, 100), (16, 16)):
        assert _fused_entry(rh, rw, out_p) == _lib.SSAL_EINVAL
        assert "multiples of 32" in L.ssal_last_error().decode()
        with pytest.raises(ValueError, match="multiples of 32"):
            _lib.check(_fused_entry(rh, rw, out_p))
    # rh <= 0
    for rh, rw in ((0, 32), (32, -32)):
        assert _fused_entry(rh, rw, out_p) == _lib.SSAL_EINVAL
        assert "must be positive" in L.ssal_last_error().decode()
    # a null region output
    assert _fused_entry(32, 32, None) == _lib.SSAL_EINVAL
    assert "region_scores_dev is NULL" in L.ssal_last_error().decode()
    # and with valid region arguments the entry goes on to the handle check
    assert _fused_entry(32, 32, out_p) == _lib.SSAL_EINVAL
    assert "net is NULL" in L.ssal_last_error().decode()
    # the other entries: size <= 0, null pointers, the tile rule of the host twin
    assert L.ssal_region_means_plane(None, 1, 64, 64, 0, 8, out_p, None) == _lib.SSAL_EINVAL
    assert L.ssal_region_means_plane(None, 1, 64, 64, 8, 8, out_p, None) == _lib.SSAL_EINVAL
    assert "NULL" in L.ssal_last_error().decode()
    assert L.ssal_icnet_score_regions_nhwc(None, None, 0, 1, 64, 64, 1, 0.0, 8, -1, None, out_p, None, None, None, None, 0,
                                           None) == _lib.SSAL_EINVAL
    assert L.ssal_icnet_score_regions_nhwc(None, None, 0, 1, 64, 64, 1, 0.0, 8, 8, None, None, None, None, None, None, 0,
                                           None) == _lib.SSAL_EINVAL
    assert "region_scores_dev is NULL" in L.ssal_last_error().decode()
    assert L.ssal_score_logits_regions_nhwc(None, 1, 64, 64, 19, 0, 0.0, 0, 0, None, out_p, None, None, None, None, 0,
                                            None) == _lib.SSAL_EINVAL
    assert L.ssal_score_regions_workspace_bytes(0, 64, 64) == -1
    assert L.ssal_score_regions_workspace_bytes(2, 64, 64) >= L.ssal_score_workspace_bytes(2, 64, 64) + 2 * 64 * 64 * 4
    plane = _plane(1, 64, 64, seed=1)
    with pytest.raises(ValueError, match="multiples of 32"):
        _lib.region_reduce_host(_tile_sums(plane), 64, 64, 48, form="tiles")
    assert L.ssal_region_reduce_host(1, None, 1, 64, 64, 8, 8, out_p, None) == _lib.SSAL_EINVAL
    assert L.ssal_region_reduce_host(7, plane.ctypes.data_as(ctypes.c_void_p), 1, 64, 64, 8, 8, out_p, None) == _lib.SSAL_EINVAL


# ---- select_regions -------------------------------------------------------------------------------------------------------
def _brute_force(conf, examples, k, max_per_image, annotated):
    """the specification, written as a plain sort + walk"""
    conf = np.asarray(conf, dtype=np.float32)
    cand = []
    for e in range(conf.shape[0]):
        for y in range(conf.shape[1]):
            for x in range(conf.shape[2]):
                if annotated is None or not annotated[e, y, x]:
                    cand.append((float(conf[e, y, x]), int(examples[e]), y, x))
    cand.sort()
    taken, per = [], {}
    for _, ex, y, x in cand:
        if len(taken) >= k:
            break
        if max_per_image is not None and per.get(ex, 0) >= max_per_image:
            continue
        per[ex] = per.get(ex, 0) + 1
        taken.append((ex, y, x))
    return np.asarray(taken, dtype=np.int64).reshape(-1, 3)


@pytest.mark.parametrize("max_per_image", [None, 1, 2, 5])
@pytest.mark.parametrize("with_annotated", [False, True])
def test_select_regions_matches_brute_force(max_per_image, with_annotated):
    rng = np.random.default_rng(11)
    e, ry, rx = 9, 4, 6
    # few distinct values: ties everywhere, so the (example id, ry, rx) tie-break decides most of the order
    conf = (rng.integers(0, 7, size=(e, ry, rx)) / 7.0).astype(np.float32)
    examples = rng.permutation(40)[:e]  # unsorted example ids
    annotated = rng.random((e, ry, rx)) < 0.3 if with_annotated else None
    for k in (0, 1, 10, 37, e * ry * rx, 10 * e * ry * rx):
        got = al.select_regions(conf, examples, k, max_per_image, annotated)
        want = _brute_force(conf, examples, k, max_per_image, annotated)
        assert got.dtype == np.int64 and got.shape == want.shape, (k, got.shape, want.shape)
        assert np.array_equal(got, want), k
        if annotated is not None and len(got):
            rows = {int(x): i for i, x in enumerate(examples)}
            assert not any(annotated[rows[a], b, c] for a, b, c in got)
    # selection_size beyond the candidates: every candidate (or m per example), once
    n_free = e * ry * rx - (int(annotated.sum()) if annotated is not None else 0)
    full = al.select_regions(conf, examples, 10 ** 6, max_per_image, annotated)
    if max_per_image is None:
        assert len(full) == n_free
    assert len({tuple(r) for r in full.tolist()}) == len(full)


def test_select_regions_rounds_to_float32_first():
    """two float64 scores that differ below float32 resolution are a TIE: the example id decides, not the float64 value"""
    conf64 = np.zeros((2, 1, 2), dtype=np.float64)
    conf64[0, 0, 0] = 0.5 + 1e-12   # example 7: larger in float64, equal in float32
    conf64[1, 0, 0] = 0.5           # example 9
    conf64[:, 0, 1] = 0.9
    got = al.select_regions(conf64, [7, 9], 1)
    assert got.tolist() == [[7, 0, 0]]
    assert _brute_force(conf64, [7, 9], 1, None, None).tolist() == [[7, 0, 0]]
    sel, conf32 = al.finish_region_ranking(np.array([1, 0]), conf64[::-1], 2, [0, 1], 4)
    assert conf32.dtype == np.float32 and np.array_equal(conf32, conf64.astype(np.float32))
    assert sel.tolist() == [[0, 0, 0], [1, 0, 0], [0, 0, 1], [1, 0, 1]]


def test_select_regions_rejects_bad_arguments():
    conf = np.zeros((2, 2, 2), dtype=np.float32)
    with pytest.raises(ValueError):
        al.select_regions(conf[0], [0, 1], 1)
    with pytest.raises(ValueError):
        al.select_regions(conf, [0], 1)
    with pytest.raises(ValueError):
        al.select_regions(conf, [0, 1], 1, annotated=np.zeros((2, 2), dtype=bool))
    with pytest.raises(ValueError):
        al.select_regions(conf, [0, 1], 1, max_per_image=0)


# ---- the merge of rank_regions under a world-2 gloo group ------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _fake_region_scores(num, ry, rx):
    rng = np.random.default_rng(77)
    return rng.random((num, ry, rx)) * 0.5 + (rng.integers(0, 3, size=(num, ry, rx)) / 4.0)


class _CollectiveCounter:
    NAMES = ("all_gather_into_tensor", "all_gather", "all_reduce", "broadcast", "reduce", "all_to_all",
             "gather", "scatter", "reduce_scatter", "barrier", "all_gather_object")

    def __enter__(self):
        self.calls, self._orig = [], {}
        for nm in self.NAMES:
            if hasattr(dist, nm):
                self._orig[nm] = getattr(dist, nm)
                setattr(dist, nm, self._wrap(nm, self._orig[nm]))
        return self

    def _wrap(self, nm, fn):
        def inner(*a, **kw):
            self.calls.append(nm)
            return fn(*a, **kw)
        return inner

    def __exit__(self, *exc):
        for nm, fn in self._orig.items():
            setattr(dist, nm, fn)


NUM, RY, RX, K, CAP = 203, 4, 8, 60, 2


def _unlabelled():
    return np.arange(NUM)[np.arange(NUM) % 4 != 1]


def _annotated():
    return np.random.default_rng(5).random((len(_unlabelled()), RY, RX)) < 0.2


def _worker(rank, world, port, out_dir, overflow):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    from semanticsegmentationactivelearning_amd import active_learning as al_
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        scores = _fake_region_scores(NUM, RY, RX)
        pos = al_.shard_positions(NUM, rank, world)
        mine = pos[pos >= 0]
        if rank == 1:
            mine = mine[::-1].copy()  # scored in another order
        if overflow and rank == 1:
            mine = np.concatenate([mine, mine[:3]])  # longer than ceil(num / world)
        idx, sc = torch.from_numpy(mine), torch.from_numpy(scores[mine])
        with _CollectiveCounter() as cc:
            try:
                sel, conf = al_.merge_and_rank_regions(idx, sc, NUM, _unlabelled(), K, CAP, _annotated())
                raised = ""
            except ValueError as e:
                sel, conf, raised = np.zeros((0, 3), np.int64), np.zeros((0,), np.float32), str(e)
        assert cc.calls == ["all_gather_into_tensor"], cc.calls  # exactly ONE collective, also on the failing pass
        np.save(os.path.join(out_dir, "sel_%d.npy" % rank), sel)
        np.save(os.path.join(out_dir, "conf_%d.npy" % rank), conf)
        with open(os.path.join(out_dir, "raised_%d.txt" % rank), "w") as f:
            f.write(raised)
    finally:
        dist.destroy_process_group()


def test_two_rank_region_merge_matches_single_process(tmp_path):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), False), nprocs=world, join=True)
    sels = [np.load(tmp_path / ("sel_%d.npy" % r)) for r in range(world)]
    confs = [np.load(tmp_path / ("conf_%d.npy" % r)) for r in range(world)]
    assert all(open(tmp_path / ("raised_%d.txt" % r)).read() == "" for r in range(world))
    assert np.array_equal(sels[0], sels[1]) and np.array_equal(confs[0], confs[1])  # identical, ORDER included
    scores = _fake_region_scores(NUM, RY, RX)
    want_sel, want_conf = al.finish_region_ranking(np.arange(NUM), scores, NUM, _unlabelled(), K, CAP, _annotated())
    assert np.array_equal(sels[0], want_sel) and np.array_equal(confs[0], want_conf)
    assert confs[0].dtype == np.float32 and confs[0].shape == (len(_unlabelled()), RY, RX)
    assert np.array_equal(want_sel, _brute_force(scores[_unlabelled()], _unlabelled(), K, CAP, _annotated()))
    assert len(want_sel) == K and np.bincount(want_sel[:, 0]).max() <= CAP
    assert set(want_sel[:, 0].tolist()) <= set(_unlabelled().tolist())


def test_two_rank_region_merge_raises_on_every_rank_for_a_long_shard(tmp_path):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), True), nprocs=world, join=True)
    for r in range(world):
        msg = open(tmp_path / ("raised_%d.txt" % r)).read()
        assert "longer than ceil(num_examples / world)" in msg and "[1]" in msg, (r, msg)


def test_single_process_region_helpers():
    idx, sc = torch.arange(3), torch.rand(3, 2, 2, dtype=torch.float64)
    a, b = al.pad_to_length(idx, sc, 5)
    assert a.tolist() == [0, 1, 2, -1, -1] and b.shape == (5, 2, 2) and torch.isinf(b[3:]).all() and torch.equal(b[:3], sc)
    with pytest.raises(ValueError):
        al.pad_to_length(idx, sc, 2)
    sel, conf = al.merge_and_rank_regions(idx, sc, 3, [0, 2], 3)
    assert conf.shape == (2, 2, 2) and sel.shape == (3, 3)


# ---- region_boxes --------------------------------------------------------------------------------------------------------
def test_region_boxes_clip_to_the_frame():
    sel = np.array([[5, 0, 0], [5, 4, 2], [9, 1, 1], [9, 4, 0]], dtype=np.int64)
    got = inference.region_boxes(sel, (32, 128), (136, 264))
    assert got.dtype == np.int64
    assert got.tolist() == [[0, 0, 32, 128], [128, 256, 136, 264], [32, 128, 64, 256], [128, 0, 136, 128]]
    assert inference.region_boxes(sel[:1], 64, (64, 64)).tolist() == [[0, 0, 64, 64]]
    assert inference.region_boxes(sel[:1], 1000, (64, 96)).tolist() == [[0, 0, 64, 96]]
    assert inference.region_boxes(np.zeros((0, 3), np.int64), 32, (64, 64)).shape == (0, 4)
    # every box covers exactly the clipped pixel count the reduction divides by
    _, counts = _lib.region_reduce_host(np.zeros((1, 136, 264), np.float32), 136, 264, (32, 128))
    for (_, ry, rx), (y0, x0, y1, x1) in zip(sel.tolist(), got.tolist()):
        assert (y1 - y0) * (x1 - x0) == counts[ry, rx]
    with pytest.raises(ValueError):
        inference.region_boxes(np.array([[0, 5, 0]]), 32, (136, 264))  # ry = 5 is outside the 5-row grid
    with pytest.raises(ValueError):
        inference.region_boxes(sel, 0, (136, 264))
