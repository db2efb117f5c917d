"""ICNet's four trainers at the split-K grids the real workload runs and no other test reaches.

Every weight gradient of these trainers is a split-K sum: G = min(tiles, cap, max_workgroups) workgroups stride over the pixel
tiles (``t = blockIdx.x; t < tiles; t += gridDim.x``), each writes one partial, a finish kernel folds the G partials in a fixed
order.  The trainers' own tests stay at max_workgroups in {1, 2} or at shapes of a handful of tiles.  Here every case runs the
FULL check of the trainer's own test (its ``_check_gradient``, imported, not restated): all gradients elementwise within
kappa 2^-24 C of the float64 oracle with kappa at the case's own max_workgroups, the loss within 1e-5, two calls bit-identical,
the bit-identity chain to the next-shallower trainer at the same max_workgroups and, for the high-resolution trainer, uint8
frames against fp32 frames -- at

  (a) small shapes with max_workgroups in {3, 5, 7}: G >= 3 groups of which some run one round more than the others, and
      max_workgroups = 0 there: the default grid G = tiles, one tile per group, G partials in the fold;
  (b) max_workgroups = 0 at one shape per cap -- tiles > cap, tiles no multiple of the cap, a partial last tile;
  (c) the capped feature-entry cases of (b) and one ``step_features`` each on guarded, poisoned allocations: the partial buffers
      [cap][PART] are written up to their last slot there and nothing beyond them.

Each case asserts its preconditions from the oracle modules' own grid arithmetic (tests/icnet_grids.py); the CPU file
tests/test_train_icnet_grids_cpu.py checks that arithmetic against the launch code's and shows that a dropped or doubled
second-round tile leaves the bound.  Inputs: of random sign (each trainer's own ``_case``) and the sign-coherent ones of
``icnet_highres_train_oracle.case(..., coherent=True)`` (``icnet_grids.coherent_inputs``), where the bound is tight.

K = 19 with weight / smoothing (1.02, 0.1) everywhere, the head's cap shape included: its float64 oracle takes 3 s there (1 s at
K = 2), no longer than the cascade's, so nothing was dropped to K = 2.

The strided data-gradient launches (k_icnet_cascade_dx, k_icnet_cascade_g24, k_icnet_highres_dproj, k_icnet_highres_dx) take
their grid from the same ``icnet_grid(tiles, cap, max_workgroups)`` under caps of 2048 and 65536, which only a workload-size
input exceeds (2048 tiles of 8 x 16 pixels).  Part (a)'s max_workgroups put those launches on the same strided path with
several rounds per group; no full-size oracle case is built for the caps themselves."""
import functools

import numpy as np
import pytest
import torch

from semanticsegmentationactivelearning_amd import training

import icnet_cascade_train_oracle as ico
import icnet_fusion_train_oracle as ifo
import icnet_grids as gr
import icnet_highres_train_oracle as iho3
import test_gpu_train_icnet_cascade as tca
import test_gpu_train_icnet_fusion as tfu
import test_gpu_train_icnet_head as the
import test_gpu_train_icnet_highres as thr
from guarded_alloc import GuardedAlloc, same_bits

pytestmark = pytest.mark.gpu

K, WEIGHT, LS = 19, 1.02, 0.1
TRAINERS = ("head", "fusion", "cascade", "highres")

# (a) the largest shape of each trainer's own test, or the next ragged one up at which one of the trainer's OWN launches has
# tiles % G != 0 with G >= 3 for every max_workgroups of {3, 5, 7} (the own shapes (1, 3, 9) / (1, 3, 5) have 3, 4, 4 and
# 6 / 18 / 15 tiles: G = tiles at 5 and 7, or every count a multiple of 3).  Tiles of the own launches:
SMALL = {"head": (2, 5, 13),     # 8
         "fusion": (2, 3, 5),    # 8 (the head under it: 6)
         "cascade": (2, 3, 5),   # 8 (the fusion block under it: 18, the head: 15)
         "highres": (1, 4, 5)}   # 8, 24, 20 (the cascade block: 4, the fusion block: 12, the head: 20)
# (b) one shape per cap; tiles of every launch that must run capped (own launches first), as DESIGN.md section 34 lists them
CAPPED = {"head": ((1, 129, 129), [1089]),            # against 1024
          "fusion": ((3, 11, 22), [108]),             # against 96
          "cascade": ((3, 9, 17), [75, 243]),         # against 64; the fusion block under it against 96
          "highres": ((3, 11, 5), [66, 198, 165])}    # against 64 (and the fusion block under it: 99 against 96)


@functools.lru_cache(maxsize=None)
def _inputs(trainer, shape, coherent, seed, c_in=3):
    """one set of arrays per case, shared by (b) and (c) and never written to"""
    n, h, w = shape
    if coherent:
        return gr.coherent_inputs(trainer, n, h, w, K, c_in)
    if trainer == "highres":
        return thr._case(seed, n, h, w, K, c_in)
    return {"head": the, "fusion": tfu, "cascade": tca}[trainer]._case(seed, n, h, w, K)


_NETS = {}


def _net_with_stats(mod, stats):
    """this file's own model per trainer (the shared models of the trainers' own tests keep their statistics)"""
    if mod not in _NETS:
        _NETS[mod] = mod._net(K)
    for name, v in zip(mod.STAT_NAMES, np.split(np.asarray(stats, dtype=np.float32), len(mod.STAT_NAMES))):
        mod._var(_NETS[mod], name).assign(v)
    return _NETS[mod]


def _check(trainer, shape, mw, coherent, seed, c_in=3):
    tag = "%s %s %r mw=%d C_in=%d" % (trainer, "coherent" if coherent else "random", shape, mw, c_in)
    case = _inputs(trainer, shape, coherent, seed, c_in)
    if trainer == "head":
        return the._check_gradient(K, *case, WEIGHT, LS, mw)
    if trainer == "highres":
        return thr._check_gradient(thr._shared_net(K, c_in), K, *case, WEIGHT, LS, mw, tag)
    mod = tfu if trainer == "fusion" else tca
    if coherent:
        *feats, d, stats, labels, mask = case
        net = _net_with_stats(mod, stats)
    else:
        *feats, d, labels, mask = case
        net = mod._shared_net(K)
    return mod._check_gradient(net, K, *feats, d, labels, mask, WEIGHT, LS, mw, tag)


@pytest.mark.parametrize("coherent", [False, True], ids=["random", "coherent"])
@pytest.mark.parametrize("mw", [0, 3, 5, 7])
@pytest.mark.parametrize("trainer", TRAINERS)
def test_uneven_strides_at_small_shapes(trainer, mw, coherent):
    """(a): the full check where some groups run one round more than the others, and on the default grid G = tiles"""
    shape = SMALL[trainer]
    all_launches = gr.launches(trainer, *shape, mw)
    own = all_launches[:gr.OWN[trainer]]
    print("%s %r mw=%d: %s" % (trainer, shape, mw, ["%s %d tiles / %d groups" % l[:3] for l in all_launches]))
    assert any(gr.ragged(l) for l in own)
    if mw:
        # one launch or more of the trainer's own (not only of the shallower trainer it runs) has tiles % G != 0 with G >= 3
        assert any(gr.uneven(l) for l in own), own
        assert all(l[2] == min(l[1], mw) for l in all_launches)
    else:
        # max_workgroups = 0 below every cap is the default grid: one tile per group and three or more partials in every fold
        # of the trainer's own (tiles % G != 0 needs tiles > cap there: part (b))
        assert all(l[1] == l[2] < l[3] for l in all_launches) and all(l[2] >= 3 for l in own), all_launches
    _check(trainer, shape, mw, coherent, 7100 + 10 * TRAINERS.index(trainer) + mw)


@pytest.mark.parametrize("coherent", [False, True], ids=["random", "coherent"])
@pytest.mark.parametrize("trainer", TRAINERS)
def test_the_caps_themselves(trainer, coherent):
    """(b): max_workgroups = 0 at the smallest balanced shape found with tiles > cap, tiles % cap != 0 and a partial last tile
    for every own launch of the trainer: G = cap, the first tiles % cap groups run one round more, the fold takes cap partials
    and the partial buffer is written up to its last slot"""
    shape, want_tiles = CAPPED[trainer]
    all_launches = gr.launches(trainer, *shape, 0)
    must = all_launches[:len(want_tiles)]
    print("%s %r: %s" % (trainer, shape, ["%s %d tiles / %d groups (cap %d)" % l[:4] for l in all_launches]))
    assert [l[1] for l in must] == want_tiles
    for name, tiles, g, cap, _ in must:
        assert tiles > cap and tiles % cap != 0 and g == cap, (name, tiles, g, cap)
    assert all(gr.capped(l) for l in must) and any(gr.ragged(l) for l in must)
    if trainer == "highres":  # the fusion block inside it runs at its own cap too
        name, tiles, g, cap, _ = all_launches[4]
        assert (name, tiles, g, cap) == ("k_icnet_fusion_wgrad<128>", 99, 96, 96) and gr.ragged(all_launches[4])
    _check(trainer, shape, 0, coherent, 7200 + TRAINERS.index(trainer))


def test_the_caps_on_four_channel_uint8_frames():
    """k_icnet_highres_wgrad1<4, uint8_t> (and <4, float>: the check compares the two) at 165 chunks over 64 groups"""
    shape, want_tiles = CAPPED["highres"]
    own = gr.launches("highres", *shape, 0)[:3]
    assert [l[1] for l in own] == want_tiles and all(gr.capped(l) for l in own)
    _check("highres", shape, 0, True, 0, c_in=4)


# ---- (c) guards at the caps ------------------------------------------------------------------------------------------------
def _assign(net, values):
    for name, v in values.items():
        layer, attr = name.split(".")
        getattr(getattr(net, layer), attr).assign(v)


def _entries(trainer, put):
    """``gradient_features`` and one ``step_features`` of a fresh model at the trainer's cap shape, the workspaces dropped before
    each call -> host copies of the loss, every gradient, the step's loss and the updated weights"""
    case = _inputs(trainer, CAPPED[trainer][0], False, 7200 + TRAINERS.index(trainer))
    if trainer == "highres":
        c54, c31, u8, d, stats, labels, mask = case
        feats, mod, names = (c54, c31, u8), thr, iho3.NAMES
        net = thr._net(K)
        thr._set_stats(net, stats)
    else:
        mod, names = (tfu, ifo.NAMES) if trainer == "fusion" else (tca, ico.NAMES)
        *feats, d, labels, mask = case
        net = mod._net(K)
        _assign(net, dict(zip(mod.STAT_NAMES, np.split(mod._stats(mod._shared_net(K)), len(mod.STAT_NAMES)))))
    _assign(net, d)
    cls = {"fusion": training.ICNetFusionTrainer, "cascade": training.ICNetCascadeTrainer,
           "highres": training.ICNetHighResTrainer}[trainer]
    tr = cls(net, 1e-3, loginverse_scaling=WEIGHT, label_smoothing=LS)

    def fresh():
        net._workspaces.clear()
        net._tls.last = (None, None, None, None)
    fresh()
    loss, gd = tr.gradient_features(*[put(f) for f in feats], put(labels), put(mask))
    out = {"loss": loss.cpu().numpy()}
    out.update({"g:" + nm: gd[nm].cpu().numpy() for nm in names})
    fresh()
    out["step_loss"] = tr.step_features(*[put(f) for f in feats], put(labels), put(mask)).cpu().numpy()
    torch.cuda.synchronize()
    out.update({"w:" + nm: mod._var(net, nm).numpy().copy() for nm in names})
    return out


@pytest.mark.parametrize("trainer", ["fusion", "cascade", "highres"])
def test_guards_at_the_caps(trainer):
    """(c): no guard of any allocation changes while every partial slot up to the cap is written, and the bits are those of the
    run on plain allocations (pattern 0xFF: what no kernel wrote reads as NaN)"""
    assert all(gr.capped(l) for l in gr.launches(trainer, *CAPPED[trainer][0], 0)[:len(CAPPED[trainer][1])])
    want = _entries(trainer, lambda a: torch.as_tensor(a).cuda())
    with GuardedAlloc("cuda", 0xFF) as g:
        got = _entries(trainer, g.guarded_from_numpy)
        g.check()
        assert g.count > 0
    assert sorted(got) == sorted(want)
    for key in want:
        assert same_bits(got[key], want[key]), key
    assert np.isfinite(want["loss"]).all() and same_bits(want["loss"].ravel()[:1], want["step_loss"].ravel()[:1])
    assert all(np.isfinite(v).all() for v in want.values())
    assert any(np.abs(v).max() > 0 for key, v in want.items() if key.startswith("g:"))
