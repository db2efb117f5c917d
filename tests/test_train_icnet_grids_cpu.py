"""The grid cases of tests/test_gpu_train_icnet_grids.py without a GPU: the oracle modules' grid
arithmetic against a literal restatement of the launch code's (``icnet_grid``, ``icnet_head_workgroups`` and the tile
expressions of the launchers, their constants read from the sources), the preconditions of the GPU cases, the tile numbering of
``icnet_grids.tile_mask``, and the discrimination of the bound at the caps: a second-round tile left out of a split-K sum, or
counted twice, leaves kappa 2^-24 C."""
import os
import re

import numpy as np
import pytest
import torch

import icnet_cascade_train_oracle as ico
import icnet_fusion_train_oracle as ifo
import icnet_grids as gr
import icnet_head_train_oracle as iho
import icnet_highres_train_oracle as iho3

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "semanticsegmentationactivelearning_amd", "csrc")
# the shapes of the GPU file (their literals are restated here: this file imports nothing that needs a GPU)
SMALL = {"head": (2, 5, 13), "fusion": (2, 3, 5), "cascade": (2, 3, 5), "highres": (1, 4, 5)}
CAPPED = {"head": (1, 129, 129), "fusion": (3, 11, 22), "cascade": (3, 9, 17), "highres": (3, 11, 5)}


# ---- the launch code, restated ------------------------------------------------------------------------------------------------
def _constant(source, name):
    """``name = <integer>`` of a ``constexpr int`` line of the source"""
    with open(os.path.join(CSRC, source)) as f:
        (m,) = re.findall(r"constexpr int [^;\n]*\b%s = (\d+)\b" % name, f.read())
    return int(m)


def _cdiv(a, b):
    return (a + b - 1) // b


def icnet_grid(tiles, cap, max_workgroups):
    """ssal_train_icnet_common.h"""
    g = tiles if tiles < cap else cap
    if max_workgroups > 0 and g > max_workgroups:
        g = max_workgroups
    return 1 if g < 1 else g


def icnet_head_workgroups(h8, w8, max_workgroups, IH_T, IH_MAX_WG):
    """ssal_train_icnet.hip"""
    g = ((2 * h8 + IH_T - 1) // IH_T) * ((2 * w8 + IH_T - 1) // IH_T)
    if g > IH_MAX_WG:
        g = IH_MAX_WG
    if max_workgroups > 0 and g > max_workgroups:
        g = max_workgroups
    return g


def launch_code(trainer, n, h, w, mw):
    """[(tiles, G)] of every split-K launch as the launchers compute them, in ``icnet_grids.launches``' order"""
    IH_T, IH_MAX_WG = _constant("ssal_train_icnet.h", "IH_T"), _constant("ssal_train_icnet.h", "IH_MAX_WG")
    FU_TH, FU_TW = _constant("ssal_train_icnet_fusion.h", "FU_TH"), _constant("ssal_train_icnet_fusion.h", "FU_TW")
    with open(os.path.join(CSRC, "ssal_train_icnet_common.h")) as f:
        (caps,) = re.findall(r"MAX_WG = CIN == 128 \? (\d+) : (\d+);", f.read())
    block_cap = {128: int(caps[0]), 256: int(caps[1])}

    def head(h8, w8):
        return [(_cdiv(2 * h8, IH_T) * _cdiv(2 * w8, IH_T), icnet_head_workgroups(h8, w8, mw, IH_T, IH_MAX_WG))]

    def block(cin, hl, wl):  # icnet_block_workgroups<CIN>(n, h, w, max_workgroups) on the low-resolution input
        tiles = n * _cdiv(2 * hl, FU_TH) * _cdiv(2 * wl, FU_TW)
        return [(tiles, icnet_grid(tiles, block_cap[cin], mw))]
    if trainer == "head":
        return head(h, w)
    if trainer == "fusion":
        return block(128, h, w) + head(2 * h, 2 * w)
    if trainer == "cascade":
        return block(256, h, w) + block(128, 2 * h, 2 * w) + head(4 * h, 4 * w)
    HW_TH, HW_TW = _constant("ssal_train_icnet_highres.hip", "HW_TH"), _constant("ssal_train_icnet_highres.hip", "HW_TW")
    HR_MAX_WG = _constant("ssal_train_icnet_highres.h", "HR_MAX_WG")
    H, W = 32 * h, 32 * w
    h2, w2, h4, w4, h8, w8 = H // 2, W // 2, H // 4, W // 4, H // 8, W // 8
    wt3 = n * _cdiv(h8, HW_TH) * _cdiv(w8, HW_TW)
    wt2 = n * _cdiv(h4, HW_TH) * _cdiv(w4, HW_TW)
    chunks = _cdiv(n * h2 * w2, 256)
    return ([(t, icnet_grid(t, HR_MAX_WG, mw)) for t in (wt3, wt2, chunks)]
            + block(256, h, w) + block(128, 2 * h, 2 * w) + head(4 * h, 4 * w))


def test_the_restated_constants_are_the_sources():
    assert (_constant("ssal_train_icnet.h", "IH_T"), _constant("ssal_train_icnet.h", "IH_MAX_WG")) == (iho.TILE, gr.HEAD_CAP)
    assert (_constant("ssal_train_icnet_fusion.h", "FU_TH"), _constant("ssal_train_icnet_fusion.h", "FU_TW")) == (ifo.TILE_H,
                                                                                                                   ifo.TILE_W)
    assert (_constant("ssal_train_icnet_highres.hip", "HW_TH"), _constant("ssal_train_icnet_highres.hip", "HW_TW")) == iho3.WG_TILE
    assert _constant("ssal_train_icnet_highres.h", "HR_MAX_WG") == iho3.MAX_WG == 64
    assert (ifo.MAX_WG, ico.MAX_WG, iho3.W1_CHUNK) == (96, 64, 256)
    assert icnet_grid(0, 64, 0) == 1 and icnet_grid(5, 64, 0) == 5 and icnet_grid(65, 64, 0) == 64 and icnet_grid(65, 64, 7) == 7


@pytest.mark.parametrize("trainer", ["head", "fusion", "cascade", "highres"])
def test_oracle_grid_arithmetic_is_the_launch_code(trainer):
    """``workgroups()`` of the four oracle modules (through ``icnet_grids.launches``) against the restated launch code, over a
    sweep of (n, h, w, max_workgroups) around every cap and at every shape of the GPU file"""
    lim = {"head": (1, 140, 140), "fusion": (3, 24, 24), "cascade": (3, 12, 18), "highres": (3, 12, 6)}[trainer]
    shapes = {SMALL[trainer], CAPPED[trainer], (1, 1, 1), (1, 3, 5), (1, 3, 9), (2, 2, 3), (1, 3, 2)}
    rng = np.random.default_rng(3)
    shapes |= {tuple(int(rng.integers(1, l + 1)) for l in lim) for _ in range(60)}
    shapes |= {(lim[0], lim[1] - i, lim[2] - j) for i in range(3) for j in range(3)}
    for n, h, w in sorted(shapes):
        for mw in (0, 1, 2, 3, 5, 7, 63, 64, 65, 95, 96, 97, 1023, 1024, 1025):
            got = [(l[1], l[2]) for l in gr.launches(trainer, n, h, w, mw)]
            assert got == launch_code(trainer, n, h, w, mw), (trainer, n, h, w, mw)


def test_preconditions_of_the_gpu_cases():
    """what the GPU file asserts case by case, once here: uneven strides at the small shapes, the caps at the capped ones"""
    for trainer, shape in SMALL.items():
        for mw in (3, 5, 7):
            own = gr.launches(trainer, *shape, mw)[:gr.OWN[trainer]]
            assert any(gr.uneven(l) for l in own) and any(gr.ragged(l) for l in own), (trainer, mw)
        assert all(l[1] == l[2] for l in gr.launches(trainer, *shape, 0))
    want = {"head": [1089], "fusion": [108], "cascade": [75, 243], "highres": [66, 198, 165]}
    for trainer, shape in CAPPED.items():
        must = gr.launches(trainer, *shape, 0)[:len(want[trainer])]
        assert [l[1] for l in must] == want[trainer]
        assert all(gr.capped(l) for l in must) and any(gr.ragged(l) for l in must), trainer
    assert gr.launches("highres", 3, 11, 5)[4][:4] == ("k_icnet_fusion_wgrad<128>", 99, 96, 96)


def test_tile_masks_partition_the_map():
    for trainer, i in (("fusion", 0), ("highres", 0), ("highres", 1), ("highres", 2)):
        n = CAPPED[trainer][0]
        launch = gr.launches(trainer, *CAPPED[trainer])[i]
        total = sum(gr.tile_mask(launch, n, t) for t in range(launch[1]))
        assert (total == 1.0).all()
    # image-major, then row-major over the image's tiles: tile 36 of 3 x 36 is the first of image 1, tile 107 the partial last
    launch = gr.launches("fusion", 3, 11, 22)[0]
    assert gr.tile_mask(launch, 3, 36)[1, :4, :8].all() and gr.tile_mask(launch, 3, 36).sum() == 32
    assert gr.tile_mask(launch, 3, 107)[2, 20:, 40:].all() and gr.tile_mask(launch, 3, 107).sum() == 8


# ---- a dropped or doubled second-round tile leaves the bound ----------------------------------------------------------------
K, WEIGHT, LS = 19, 1.02, 0.1
f32 = lambda a: np.asarray(a, dtype=np.float32)


def _second_round_tiles(launch):
    """the first tile of the second round (a whole one) and the last tile of the map (a partial one): both have index >= G"""
    _, tiles, g, _, _ = launch
    assert tiles > g
    return g, tiles - 1


def _report(tag, names, off, kappa_of, gv, g64, c):
    inside = []
    for name in names:
        lo, hi = off[name]
        bound = kappa_of(name) * 2.0 ** -24 * c[lo:hi]
        dlt = np.abs(gv[lo:hi] - g64[lo:hi])
        print("%s %s: %d of %d entries beyond, worst ratio %.3g, bound / max|g64| %.2e"
              % (tag, name, int((dlt > bound).sum()), hi - lo, (dlt / np.maximum(bound, 1e-300)).max(),
                 bound.max() / np.abs(g64[lo:hi]).max()))
        if not (dlt > bound).any():
            inside.append(name)
    return inside


@pytest.fixture(scope="module")
def fusion_case():
    n, h, w = CAPPED["fusion"]
    s24, c3, d, stats, labels, mask = gr.coherent_inputs("fusion", n, h, w, K)
    packed = ifo.pack(d)
    x24, x3, W = ifo._tensors(s24, c3, packed, grad=False)
    s12 = ifo.fusion_forward(x24, x3, W, stats)[0]
    _, lg = iho.head_logits(s12, W[ifo.NAMES[6]].reshape(128, K), W[ifo.NAMES[7]])
    args = (s24, c3, packed, stats, labels, mask, WEIGHT, LS, f32(s12.numpy()), f32(lg.numpy()))
    return args, ifo.grad_and_bound(*args)


@pytest.mark.parametrize("factor", [0.0, 2.0], ids=["dropped", "doubled"])
@pytest.mark.parametrize("which", [0, 1], ids=["first of round two", "last, partial"])
def test_fusion_bound_rejects_a_wrong_second_round_tile(fusion_case, which, factor):
    """k_icnet_fusion_wgrad at (3, 11, 22): 108 tiles over 96 groups.  One tile of index >= 96 left out of the contraction of
    the block's six parameter gradients (or counted twice) puts five of the six outside kappa 2^-24 C on the sign-coherent
    inputs of the GPU case, at that case's own kappa (max_workgroups = 0).
    The bound does NOT separate conv_sub2.gamma (worst ratio 0.92 for the whole tile, 0.28 for the partial one): its sum
    g (acc_a - mean) rstd runs over a pre-BN accumulator of both signs (conv_sub2's kernel keeps its random signs in the coherent
    inputs), so C lies 1.8e-2 of |g| there instead of 1.6e-3.  The device forms that gradient from the folded sums of
    conv_sub2.kernel (k_icnet_block_gamma), so a wrong tile shows in the kernel's own entries; it is asserted to stay inside,
    so that a change of the inputs that tightens it is noticed"""
    args, (g64, c, _) = fusion_case
    n, h, w = CAPPED["fusion"]
    launch = gr.launches("fusion", n, h, w)[0]
    assert gr.capped(launch)
    t = _second_round_tiles(launch)[which]
    wmask = 1.0 + (factor - 1.0) * gr.tile_mask(launch, n, t)
    _, gv = ifo.loss_and_grad(*args, wmask=wmask)
    inside = _report("fusion tile %d x%g" % (t, factor), ifo.NAMES[:6], ifo.offsets(K),
                     lambda name: ifo.kappa(name, n, h, w, K, WEIGHT, 0), gv, g64, c)
    assert inside == ["conv_sub2.gamma"], "stay inside the bound: %r" % (inside,)
    lo = ifo.offsets(K)[ifo.NAMES[6]][0]
    assert np.array_equal(gv[lo:], g64[lo:])  # the head's gradients do not pass through that sum
    assert np.array_equal(ifo.loss_and_grad(*args, wmask=np.ones_like(wmask))[1], g64)


@pytest.fixture(scope="module")
def highres_case():
    n, h, w = CAPPED["highres"]
    c54, c31, u8, d, stats, labels, mask = gr.coherent_inputs("highres", n, h, w, K)
    x, packed = iho3.unit(u8), iho3.pack(d)
    at32 = tuple(f32(t) for t in iho3.forward(c54, c31, x, packed, stats, K))
    args = (c54, c31, x, packed, stats, labels, mask, K, WEIGHT, LS, at32)
    return args, iho3.grad_and_bound(*args)


@pytest.mark.parametrize("factor", [0.0, 2.0], ids=["dropped", "doubled"])
@pytest.mark.parametrize("which", [0, 1], ids=["first of round two", "last, partial"])
def test_highres_bound_rejects_a_wrong_second_round_tile(highres_case, which, factor):
    """k_icnet_highres_wgrad<64>, <32> and k_icnet_highres_wgrad1 at (3, 11, 5): 66 / 198 tiles and 165 chunks over 64 groups.
    One tile (chunk) of index >= 64 of each launch left out of that layer's kernel, gamma and beta sums, or counted twice -- one
    pass corrupts the three launches at once, their tensors are disjoint -- puts each of the nine tensors outside the bound"""
    args, (g64, c, _) = highres_case
    n, h, w = CAPPED["highres"]
    own = gr.launches("highres", n, h, w)[:3]
    wmask = {}
    for launch, layer in zip(own, (2, 1, 0)):
        assert gr.capped(launch)
        t = _second_round_tiles(launch)[which]
        m = gr.tile_mask(launch, n, t)
        if layer == 0:
            m = m.reshape(n, 16 * h, 16 * w, 1)
        assert m.sum() > 0
        wmask[layer] = 1.0 + (factor - 1.0) * m
    _, gv = iho3.loss_and_grad(*args, wmask=wmask)
    inside = _report("highres which=%d x%g" % (which, factor), iho3.BRANCH, iho3.offsets(K),
                     lambda name: iho3.kappa(name, n, h, w, K, WEIGHT, 0), gv, g64, c)
    assert not inside, "stay inside the bound: %r" % (inside,)
    lo = iho3.offsets(K)[iho3.NAMES[9]][0]
    assert np.array_equal(gv[lo:], g64[lo:])  # the cascade head's fourteen do not pass through these sums
