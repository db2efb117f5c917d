"""GPU tests of region-level acquisition: the fused ENet route (tile partials of the Final + score kernel folded by
k_reduce_regions) and the plane route (k_region_means_plane) against the CPU oracle's per-pixel confidence block-averaged
in float64 here; bit-identity of the per-image score with ``score``; fused against plane route; invariance under batch
size, image chains and knobs; ``rank_regions`` end to end; ICNet; ``score_logits(region=...)``.

Bounds.  A mean cannot move further than its largest term and the project gates per-pixel confidence at 1e-4 (north_star;
ICNet's parity gate in tests/test_icnet_gpu.py uses the same 1e-4), so region means are asserted within 1e-4 of the
oracle's.  Two float64 summation orders of at most 2^21 values in [0, 1] differ by at most 2^21 * 2^-53 = 2.4e-10
relative, so the fused route and the plane route are asserted within 1e-9 of each other.  Every test prints the largest
difference it saw before it asserts."""
import numpy as np
import pytest
import torch

import semanticsegmentationactivelearning_amd as ssal
from helpers import frames, make_model
from oracle import enet_oracle as orc
from oracle import icnet_oracle as ico
from semanticsegmentationactivelearning_amd import _lib, active_learning as al, inference, synthetic as syn

pytestmark = pytest.mark.gpu

TOL = 1e-4        # region mean vs the oracle (see the module docstring)
TOL_ROUTES = 1e-9  # two float64 summation orders of the same fp32 values


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    _lib.lib()
    yield
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def icnet19():
    net = ssal.ICNet(19)
    net.build((None, None, None, 3))
    syn.randomize_icnet(net, seed=0)
    return net, syn.icnet_params_dict(net)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def block_means(conf, region):
    """float64 mean of every clipped region of per-pixel planes [N, H, W]"""
    rh, rw = _lib.region_size(region)
    n, h, w = conf.shape
    ry, rx = -(-h // rh), -(-w // rw)
    out = np.empty((n, ry, rx), dtype=np.float64)
    c64 = conf.astype(np.float64)
    for y in range(ry):
        for x in range(rx):
            out[:, y, x] = c64[:, y * rh:(y + 1) * rh, x * rw:(x + 1) * rw].reshape(n, -1).mean(axis=1)
    return out


def check(name, got, want, tol):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == want.shape, "%s: shape %s != %s" % (name, got.shape, want.shape)
    d = float(np.abs(got - want).max())
    print("%s: max |d| = %.3e (bound %.0e)" % (name, d, tol))
    assert d <= tol, "%s: max |d| = %.3e > %.0e" % (name, d, tol)
    return d


# ---- 6. ENet region means against the oracle ---------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(128, 256), (256, 512), (136, 264)])
@pytest.mark.parametrize("measure", ["entropy", "margin", "confidence"])
def test_enet_region_means_match_oracle(enet_c3k19, h, w, measure):
    net, P = enet_c3k19
    x = frames([3, 4], h, w, 3)
    want_mean, want_conf, _, _ = orc.score_images(P, x, measure)
    for region in (32, 64, (32, 128)):
        scores, regions = net.score_regions(dev(x), region=region, measure=measure)
        assert regions.dtype == torch.float64 and tuple(regions.shape) == (2,) + _lib.region_grid(h, w, region)
        check("ENet %dx%d %s region %s" % (h, w, measure, region), regions, block_means(want_conf, region), TOL)
        check("ENet %dx%d %s image score" % (h, w, measure), scores, want_mean, 1e-6)


def test_enet_region_means_match_oracle_c4k6(enet_c4k6):
    net, P = enet_c4k6
    x = frames([7, 8, 9], 136, 264, 4)
    _, want_conf, _, _ = orc.score_images(P, x, "entropy")
    for region in (32, 64, (32, 128)):
        _, regions = net.score_regions(dev(x), region=region, measure="entropy")
        check("ENet c_in=4 K=6 region %s" % (region,), regions, block_means(want_conf, region), TOL)


def test_enet_other_region_sizes_take_the_plane_route(enet_c3k19):
    """a size that is not a multiple of 32 (and an int, and a region larger than the frame) goes through the plane kernel"""
    net, P = enet_c3k19
    x = frames([3, 4], 136, 264, 3)
    _, want_conf, _, _ = orc.score_images(P, x, "entropy")
    for region in (48, (20, 50), (7, 13), 1, (1000, 1000), (136, 600)):
        out = net.score_regions(dev(x), region=region)
        assert len(out) == 2
        check("ENet plane route region %s" % (region,), out[1], block_means(want_conf, region), TOL)
    with pytest.raises(ValueError, match="must be positive"):
        net.score_regions(dev(x), region=0)
    with pytest.raises(NotImplementedError):
        net.score_regions(dev(x), measure="bald")


# ---- 7. per-image scores keep the bits of score() ----------------------------------------------------------------------
def test_image_scores_are_bit_identical_to_score(enet_c3k19):
    net, _ = enet_c3k19
    xf = syn.synth_frames_device(20, 5, 128, 256, 3)
    xu = syn.synth_frames_device(20, 5, 128, 256, 3, dtype=torch.uint8)
    for tag, x, kw in (("float", xf, {}), ("u8", xu, {}), ("bf16x3", xf, {"arithmetic": "bf16x3"})):
        for measure in ("entropy", "margin"):
            want = net.score(x, measure=measure, **kw)
            got, regions = net.score_regions(x, region=64, measure=measure, **kw)
            assert torch.equal(got, want), "%s %s: score_regions()[0] != score()" % (tag, measure)
            # and with maps requested (the OUT form of the Final kernel on both sides)
            want2, _ = net.score(x, measure=measure, return_label=True, **kw)
            got2, regions2, maps = net.score_regions(x, region=64, measure=measure, return_label=True, **kw)
            assert torch.equal(got2, want2) and maps["label"] is not None and maps["confidence"] is None
            assert torch.equal(regions2, regions), "%s %s: region scores depend on the optional outputs" % (tag, measure)


# ---- 8. fused route against plane route --------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(128, 256), (136, 264), (256, 512)])
def test_fused_route_matches_plane_route(enet_c3k19, h, w):
    net, _ = enet_c3k19
    x = syn.synth_frames_device(30, 3, h, w, 3)
    for region in (32, 64, (32, 128), (128, 64), (256, 512)):
        _, fused, maps = net.score_regions(x, region=region, return_confidence=True)
        plane = _lib.region_means_plane(maps["confidence"], region)
        check("fused vs plane %dx%d region %s" % (h, w, region), fused, plane.cpu().numpy(), TOL_ROUTES)
        # the device plane kernel and its host twin run the same source: the same bits
        host, _ = _lib.region_reduce_host(maps["confidence"].cpu().numpy(), h, w, region, form="plane")
        assert np.array_equal(plane.cpu().numpy(), host), "k_region_means_plane differs from its host twin (region %s)" % (region,)


def test_plane_kernel_alignment_and_odd_shapes():
    """16-byte path, scalar path (odd width / unaligned base) and the host twin give the same bits"""
    rng = np.random.default_rng(3)
    for h, w, region in ((70, 90, (7, 13)), (64, 1100, (16, 600)), (40, 72, (64, 128)), (24, 40, 1), (96, 256, (5, 256)),
                         (130, 516, (33, 68))):
        a = rng.random((2, h, w), dtype=np.float32)
        host, _ = _lib.region_reduce_host(a, h, w, region, form="plane")
        got = _lib.region_means_plane(dev(a), region).cpu().numpy()
        assert np.array_equal(got, host), (h, w, region)
        # the same planes 4 bytes off a 16-byte boundary: the scalar path
        buf = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
        shifted = buf[1:].view(2, h, w)
        shifted.copy_(dev(a))
        assert shifted.data_ptr() % 16 == 4
        assert np.array_equal(_lib.region_means_plane(shifted, region).cpu().numpy(), host), (h, w, region, "unaligned")


# ---- 9. invariance, bit for bit ----------------------------------------------------------------------------------------
def test_region_scores_do_not_depend_on_batch_chains_or_knobs(enet_c3k19):
    net, _ = enet_c3k19
    x = syn.synth_frames_device(40, 8, 128, 256, 3)
    ref = net.score_regions(x, region=64)[1]
    assert torch.equal(net.score_regions(x, region=64)[1], ref), "two runs differ"
    for i in range(8):  # frame i alone == frame i inside the batch of 8 (both chains covered)
        alone = net.score_regions(x[i:i + 1].contiguous(), region=64)[1]
        assert torch.equal(alone[0], ref[i]), "frame %d scored alone differs from the batch of 8" % i
    assert torch.equal(net.score_regions(x[:3].contiguous(), region=64)[1], ref[:3])
    try:
        for g, span in ((1, 4), (4, 4), (2, 0), (3, 3)):
            _lib.set_knob("img_groups", g)
            _lib.set_knob("img_span", span)
            assert torch.equal(net.score_regions(x, region=64)[1], ref), "img_groups=%d span=%d" % (g, span)
        _lib.set_knob("img_groups", 2)
        _lib.set_knob("img_span", 4)
        for fuse in (0, 1, 2):
            _lib.set_knob("fuse_ends", fuse)
            assert torch.equal(net.score_regions(x, region=64)[1], ref), "fuse_ends=%d" % fuse
        _lib.set_knob("fuse_ends", 3)
        _lib.set_knob("bnk_tw", 16)
        _lib.set_knob("bnk_xcd", 0)
        assert torch.equal(net.score_regions(x, region=64)[1], ref), "bnk_tw=16 bnk_xcd=0"
        _lib.set_knob("bnk_tw", 0)
        _lib.set_knob("bnk_xcd", 1)
        _lib.set_kernel_family(False)
        assert torch.equal(net.score_regions(x, region=64)[1], ref), "generic kernel family"
    finally:
        _lib.set_kernel_family(True)
        for name, v in (("img_groups", 2), ("img_span", 4), ("fuse_ends", 3), ("bnk_tw", 0), ("bnk_xcd", 1)):
            _lib.set_knob(name, v)
    assert _lib.get_knobs()["defaults"] == 1


# ---- 10. one full-size frame -------------------------------------------------------------------------------------------
def test_full_size_frame_matches_oracle(enet_c3k19):
    net, P = enet_c3k19
    x = frames([2], 1024, 2048, 3)
    want_mean, want_conf, _, _ = orc.score_images(P, x, "entropy")
    scores, regions = net.score_regions(dev(x), region=128)
    assert tuple(regions.shape) == (1, 8, 16)
    check("ENet 1024x2048 region 128", regions, block_means(want_conf, 128), TOL)
    check("ENet 1024x2048 image score", scores, want_mean, 1e-6)
    assert torch.equal(scores, net.score(dev(x)))


# ---- 11. rank_regions end to end ---------------------------------------------------------------------------------------
POOL_SEED, POOL_FRAMES, POOL_H, POOL_W, POOL_REGION, POOL_K, POOL_CAP = 6, 24, 128, 256, 32, 16, 2
GAP = 2e-4  # twice the bound of the region means: a selection boundary wider than this cannot flip


def pool_unlabelled():
    return np.arange(POOL_FRAMES)[np.arange(POOL_FRAMES) % 6 != 5]


def selection_gaps(conf32, examples, k, cap):
    """the smallest gap, in the given scores, at any decision that shapes ``select_regions(conf32, examples, k, cap)``:
    the boundary between the last region taken and the next one the walk would take, and -- for a capped walk -- for every
    example that reached its cap, the boundary between the last of its regions taken and its next one, whenever that next
    one would otherwise have come before the walk's next pick (+ GAP)"""
    sel = al.select_regions(conf32, examples, k + 1, cap)
    assert len(sel) == k + 1, "the pool is too small for this check"
    row = {int(e): i for i, e in enumerate(examples)}
    val = lambda r: float(conf32[row[int(r[0])], r[1], r[2]])
    gaps = [val(sel[k]) - val(sel[k - 1])]
    if cap is not None:
        taken = sel[:k]
        for e in np.unique(taken[:, 0]):
            mine = taken[taken[:, 0] == e]
            if len(mine) < cap:
                continue
            rest = np.sort(conf32[row[int(e)]].reshape(-1))
            nxt = float(rest[cap])  # the example's first region the cap shuts out
            if nxt < val(sel[k]) + GAP:
                gaps.append(nxt - max(val(r) for r in mine))
    return min(gaps)


@pytest.mark.parametrize("cap", [None, POOL_CAP])
def test_rank_regions_selects_what_the_oracle_selects(enet_c3k19, cap):
    """Pool: synthetic.py frames 0..23 of seed POOL_SEED at 128x256, region 32, selection_size 16, entropy; frames 5, 11, 17,
    23 count as labelled.  POOL_SEED = 6 was chosen with the CPU oracle among seeds 0..6 (the first one whose boundaries are
    wide in both walks): in the oracle's float32-rounded region means the smallest gap at a decision of the uncapped walk
    is 8.455e-04 and of the capped walk (max_per_image = 2, cap decisions included) 1.201e-03, both wider than 2e-4.  The
    precondition is asserted, not skipped: a pass cannot come from luck and a failure cannot come from a near-tie."""
    net, P = enet_c3k19
    ids = np.arange(POOL_FRAMES)
    x = syn.synth_frames_f32(ids, POOL_H, POOL_W, 3, seed=POOL_SEED)
    _, want_conf, _, _ = orc.score_images(P, x, "entropy")
    unl = pool_unlabelled()
    oracle32 = block_means(want_conf, POOL_REGION).astype(np.float32)[unl]
    gap = selection_gaps(oracle32, unl, POOL_K, cap)
    print("oracle gap at the selection boundary (cap=%s): %.3e" % (cap, gap))
    assert gap > GAP, "fixture: the oracle's selection boundary (%.3e) is not wider than %.0e" % (gap, GAP)
    want = al.select_regions(oracle32, unl, POOL_K, cap)

    batches = [(x[i:i + 8], ids[i:i + 8]) for i in range(0, POOL_FRAMES, 8)]
    sel, conf = al.rank_regions(net, batches, POOL_FRAMES, unl, POOL_K, region=POOL_REGION, measure="entropy",
                                max_per_image=cap, prefetch=2)
    assert sel.dtype == np.int64 and sel.shape == (POOL_K, 3)
    assert conf.dtype == np.float32 and conf.shape == (len(unl), POOL_H // 32, POOL_W // 32)
    check("rank_regions region_confidence (cap=%s)" % cap, conf, oracle32, TOL)
    assert {tuple(r) for r in sel.tolist()} == {tuple(r) for r in want.tolist()}
    assert np.array_equal(sel, al.select_regions(conf, unl, POOL_K, cap))
    if cap is not None:
        assert np.bincount(sel[:, 0]).max() <= cap
    boxes = inference.region_boxes(sel, POOL_REGION, (POOL_H, POOL_W))
    assert boxes.shape == (POOL_K, 4) and (boxes[:, 2] - boxes[:, 0] == 32).all() and (boxes[:, 3] <= POOL_W).all()
    # uint8 frames and annotated regions: the regions taken before are never taken again
    annotated = np.zeros(conf.shape, dtype=bool)
    row = {int(e): i for i, e in enumerate(unl)}
    for e, ry, rx in sel.tolist():
        annotated[row[e], ry, rx] = True
    sel2, conf2 = al.rank_regions(net, batches, POOL_FRAMES, unl, POOL_K, region=POOL_REGION, max_per_image=cap,
                                  annotated=annotated)
    assert np.array_equal(conf2, conf)
    assert not ({tuple(r) for r in sel2.tolist()} & {tuple(r) for r in sel.tolist()})


# ---- 12. ICNet ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(64, 128), (128, 256)])
def test_icnet_region_means_match_oracle(icnet19, h, w):
    """ICNet's per-pixel parity gate (tests/test_icnet_gpu.py) is the same 1e-4, so the bound of the ENet tests holds"""
    net, P = icnet19
    x = frames([3, 4, 5], h, w, 3)
    for measure in ("margin", "entropy"):
        want_mean, want_conf, _, _ = ico.score_images(P, x, measure)
        for region in (32, (32, 128), (20, 50)):
            scores, regions = net.score_regions(dev(x), region=region, measure=measure)
            check("ICNet %dx%d %s region %s" % (h, w, measure, region), regions, block_means(want_conf, region), TOL)
            assert torch.equal(scores, net.score(dev(x), measure)), "ICNet image scores differ from score()"
        s3, r3, maps = net.score_regions(dev(x), region=32, measure=measure, return_confidence=True, return_label=True)
        assert torch.equal(s3, net.score(dev(x), measure))
        assert torch.equal(r3, _lib.region_means_plane(maps["confidence"], 32))
        assert torch.equal(r3, net.score_regions(dev(x), region=32, measure=measure)[1])
    xu = syn.synth_frames_device(3, 2, h, w, 3, dtype=torch.uint8)
    su, ru = net.score_regions(xu, region=32)
    assert torch.equal(su, net.score(xu)) and tuple(ru.shape) == (2, h // 32, w // 32)


# ---- 13. score_logits(region=...) --------------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", ["entropy", "margin", "confidence"])
def test_score_logits_regions(measure):
    rng = np.random.default_rng(9)
    logits = (rng.normal(size=(3, 72, 100, 19)) * 3).astype(np.float32)
    want_mean, want_conf, want_label = orc.score_logits(logits, measure)
    plain = al.score_logits(dev(logits), measure)
    for region in (32, (10, 30), (72, 100), 1):
        scores, regions = al.score_logits(dev(logits), measure, region=region)
        assert torch.equal(scores, plain)
        check("score_logits %s region %s" % (measure, region), regions, block_means(want_conf, region), TOL)
    scores, regions, maps = al.score_logits(dev(logits), measure, return_label=True, return_confidence=True, region=(10, 30))
    assert np.array_equal(maps["label"].cpu().numpy(), want_label)
    assert torch.equal(regions, _lib.region_means_plane(maps["confidence"], (10, 30)))
