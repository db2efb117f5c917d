"""CPU check of the case table in bottleneck_phase_cases.py: the launcher's arithmetic (launch_bottleneck_mfma / decode_tile,
csrc/ssal_bottleneck_mfma.hip) restated in Python gives every case the property it is listed for -- unequal phases, empty
tiles, a phase <= 16 wide under a 32-wide tile, phases without rows, the side of the Wp = 16 / 17 boundary -- the expected
kernel per bnk_w8 setting, and, over the whole table, every kernel the default knobs can reach.  The dispatch lines the
restatement follows are pinned against the source, so an edit to the launcher fails here until the table follows it.
tests/test_gpu_bottleneck_phases.py runs the table on the device."""
import os
import re

import pytest

import bottleneck_phase_cases as bpc
from bottleneck_phase_cases import CASES, W8_SETTINGS, case_id, geometry, has_property, kernel_for
from semanticsegmentationactivelearning_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "semanticsegmentationactivelearning_amd", "csrc", "ssal_bottleneck_mfma.hip")

# the table, written out: (layer, dil, asym, H, W) -- the smallest shapes that reach each edge
LISTED = [
    ("Bottleneck2_1", 1, False, 8, 16), ("Bottleneck2_1", 1, False, 8, 17),
    ("Bottleneck2_2", 2, False, 16, 32), ("Bottleneck2_2", 2, False, 16, 33),
    ("Bottleneck2_4", 4, False, 32, 64), ("Bottleneck2_4", 4, False, 32, 65),
    ("Bottleneck2_6", 8, False, 64, 128), ("Bottleneck2_6", 8, False, 64, 129),
    ("Bottleneck2_2", 2, False, 17, 65), ("Bottleneck2_4", 4, False, 33, 129), ("Bottleneck2_6", 8, False, 65, 257),
    ("Bottleneck2_4", 4, False, 11, 67), ("Bottleneck2_6", 8, False, 11, 133),
    ("Bottleneck2_2", 2, False, 1, 34), ("Bottleneck2_4", 4, False, 3, 67), ("Bottleneck2_6", 8, False, 5, 133),
    ("Bottleneck2_8", 16, False, 17, 257),
] + [(name, 1, True, h, w) for name in ("Bottleneck2_3", "Bottleneck3_7") for h, w in ((8, 16), (8, 17), (1, 33), (3, 40), (13, 65))]


def test_the_table_holds_the_listed_cases():
    assert [tuple(c[:5]) for c in CASES] == LISTED
    assert len({case_id(c) for c in CASES}) == len(CASES)
    assert all(c.props for c in CASES)


def test_layers_have_the_dilation_and_form_the_table_says(enet_c3k19):
    net, _ = enet_c3k19
    for c in CASES:
        layer = getattr(net, c.layer)
        assert layer.dilation_rate[0] == c.dil and bool(layer.asymmetric) == c.asym, case_id(c)
        assert tuple(layer.proj_kernel.shape) == (1, 1, 128, 32) and layer.output_channels == 128, case_id(c)
        assert _lib.layer_dispatch("regular", 128, 128, 32, c.asym, c.h, c.w) == "fused", case_id(c)


def test_the_restated_dispatch_lines_are_the_launcher_s():
    """kernel_for follows these lines of launch_bottleneck_mfma and geometry() these of decode_tile"""
    with open(SOURCE) as f:
        text = re.sub(r"\s+", " ", f.read())
    for line in [
        "a.TH = 8;",
        "const int Hp = (H + dil - 1) / dil, Wp = (W + dil - 1) / dil;",
        "const bool o4 = !asym && Cin == C && (kn.bnk_o4 == 1 || (kn.bnk_o4 == 2 && Wp <= 16));",
        "const bool w8_shape = Wp > 16 && kn.bnk_tw != 16 && wq != nullptr && (long)H * W * C <= W8_MAX_ELEMS;",
        "const bool w8 = !asym && !o4 && dil <= 8 && kn.bnk_w8 >= 1 && w8_shape;",
        "const bool asym_w8 = asym && kn.bnk_w8 >= 2 && w8_shape;",
        "const bool asym16x = asym && kn.asym_tw16 != 0 && !asym_w8;",
        "const bool wide = (Wp > 16 && kn.bnk_tw != 16 && !o4 && !asym16x) || w8 || asym_w8;",
        "const int TW = wide ? 32 : 16;",
        "a.tiles_y = (Hp + a.TH - 1) / a.TH;",
        "a.tiles_x = (Wp + TW - 1) / TW;",
        "const long grid = (long)N * dil * dil * a.tiles_y * a.tiles_x;",
        "constexpr long W8_MAX_ELEMS = 1L << 28;",
        "t.Hp = (a.H - t.py + d - 1) / d;",
        "t.Wp = (a.W - t.px + d - 1) / d;",
        "t.empty = (t.ty0 >= t.Hp) || (t.tx0 >= t.Wp);",
        "q.bnk_tw = 0;", "q.bnk_o4 = 2;", "q.bnk_w8 = BNK_W8_DEFAULT;", "q.asym_tw16 = ASYM_TW16_DEFAULT;",
    ]:
        assert line in text, line
    assert bpc.DEFAULT_KNOBS == dict(bnk_o4=2, asym_tw16=1, bnk_tw=0) and bpc.TH == 8 and bpc.W8_MAX_ELEMS == 2 ** 28
    for name in bpc.KERNELS:  # every name is a profile row the launcher can file a launch under
        assert '"%s"' % name in text, name


def test_library_defaults_are_the_restated_ones():
    """host-only: the knobs of a freshly loaded library"""
    kn = _lib.get_knobs()
    assert kn["bnk_w8"] == 2 and kn["bnk_o4"] == 2 and kn["bnk_tw"] == 0 and kn["asym_tw16"] == 1 and kn["bnk_xcd"] == 1


@pytest.mark.parametrize("h,w,d", [(17, 65, 2), (33, 129, 4), (65, 257, 8), (11, 67, 4), (5, 133, 8), (1, 34, 2), (3, 7, 16), (19, 67, 1)])
def test_phases_partition_the_image(h, w, d):
    """phase_sizes against a count of the pixels themselves; the non-empty tiles of a phase cover it exactly once"""
    count = {}
    for y in range(h):
        for x in range(w):
            count[y % d, x % d] = count.get((y % d, x % d), 0) + 1
    phases = bpc.phase_sizes(h, w, d)
    assert [(py, px) for py, px, _, _ in phases] == [(py, px) for py in range(d) for px in range(d)]
    for py, px, hp, wp in phases:
        assert hp * wp == count.get((py, px), 0)
        assert hp == len(range(py, h, d)) and wp == len(range(px, w, d))
    assert sum(hp * wp for _, _, hp, wp in phases) == h * w
    for tw in (16, 32):
        tiles_y, tiles_x = bpc.cdiv(bpc.cdiv(h, d), bpc.TH), bpc.cdiv(bpc.cdiv(w, d), tw)
        for py, px, hp, wp in phases:
            covered = sum(max(0, min(hp - ty * bpc.TH, bpc.TH)) * max(0, min(wp - tx * tw, tw))
                          for ty in range(tiles_y) for tx in range(tiles_x))
            assert covered == hp * wp  # the grid sized for the largest phase reaches every pixel of every phase


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_case_has_the_properties_it_is_listed_for(case):
    for prop in case.props:
        assert has_property(case, prop), "%s is listed for %s" % (case_id(case), prop)
    assert case.h * case.w * 128 <= 65 * 257 * 128  # the largest single-layer tensor of the table
    g = geometry(case, 2)
    # the equal-phase and empty-tile facts hold whether or not the case is listed for them: say so both ways
    sizes = {(hp, wp) for _, _, hp, wp in g.phases}
    assert (bpc.UNEQUAL in case.props) == (len(sizes) > 1), sizes
    assert (bpc.EMPTY_TILE in case.props) == (len(g.empty_tiles) > 0), g.empty_tiles
    assert (bpc.ZERO_ROWS in case.props) == (len(g.zero_row_phases) > 0)
    assert (bpc.NARROW_PHASE in case.props) == (len(g.narrow_phases) > 0)
    assert len(g.empty_tiles) < g.tiles_per_image  # some tile does work


@pytest.mark.parametrize("d", [1, 2, 4, 8])
def test_regular_dispatch_boundary(d):
    layer = bpc.REGULAR_LAYER[d]
    at, above = [c for c in CASES if c.layer == layer and c.h == 8 * d and c.w in (16 * d, 16 * d + 1)]
    assert (at.w, above.w) == (16 * d, 16 * d + 1)
    for s in W8_SETTINGS:
        g = geometry(at, s)
        assert (g.kernel, g.tw, g.tiles_y, g.tiles_x) == ("k_bottleneck_o4", 16, 1, 1)
        assert {(hp, wp) for _, _, hp, wp in g.phases} == {(8, 16)} and not g.empty_tiles
        g = geometry(above, s)
        assert g.kernel == ("k_bottleneck_w8" if s >= 1 else "k_bottleneck_mfma<32>") and g.tw == 32
        assert (g.tiles_y, g.tiles_x) == (1, 1) and not g.empty_tiles
        assert [wp for _, _, _, wp in g.phases] == [17 if px == 0 else 16 for _ in range(d) for px in range(d)]
        assert all(hp == 8 for _, _, hp, _ in g.phases)


def test_asymmetric_dispatch_boundary_and_tiles():
    for name in bpc.ASYM_LAYERS:
        by_shape = {(c.h, c.w): c for c in CASES if c.layer == name}
        for s in W8_SETTINGS:
            assert geometry(by_shape[8, 16], s).kernel == "k_bottleneck_mfma_asym16x"
            assert geometry(by_shape[8, 16], s).tw == 16
            g = geometry(by_shape[8, 17], s)
            assert (g.kernel, g.tw) == (("k_bottleneck_asym_w8", 32) if s == 2 else ("k_bottleneck_mfma_asym16x", 16))
            assert (g.tiles_y, g.tiles_x) == ((1, 1) if s == 2 else (1, 2))
        for shape in ((1, 33), (3, 40), (13, 65)):
            assert geometry(by_shape[shape], 2).kernel == "k_bottleneck_asym_w8"
            assert geometry(by_shape[shape], 1).kernel == "k_bottleneck_mfma_asym16x"
        g = geometry(by_shape[13, 65], 2)
        assert (g.tiles_y, g.tiles_x) == (2, 3) and 65 - 2 * g.tw == 1 and 13 - bpc.TH == 5
        assert (geometry(by_shape[1, 33], 2).tiles_x, geometry(by_shape[3, 40], 2).tiles_x) == (2, 2)


@pytest.mark.parametrize("d,h,w", [(2, 17, 65), (4, 33, 129), (8, 65, 257)])
def test_unequal_phases_with_empty_tiles(d, h, w):
    case, = [c for c in CASES if (c.dil, c.h, c.w) == (d, h, w)]
    for s in W8_SETTINGS:
        g = geometry(case, s)
        assert g.kernel == ("k_bottleneck_w8" if s >= 1 else "k_bottleneck_mfma<32>")
        assert (g.tw, g.tiles_y, g.tiles_x) == (32, 2, 2)
        assert {wp for _, _, _, wp in g.phases} == {33, 32} and {hp for _, _, hp, _ in g.phases} == {9, 8}
        assert [(py, px) for py, px, hp, wp in g.phases if (hp, wp) == (9, 33)] == [(0, 0)]  # one phase fills the grid
        kinds = {}
        for py, px, ty, tx in g.empty_tiles:
            kinds.setdefault((py, px), set()).add((ty, tx))
        # a phase short in x only owns the empty x-tile of each tile row, short in y only the empty y-tile of each tile
        # column, short in both all three
        assert kinds[0, 1] == {(0, 1), (1, 1)} and kinds[1, 0] == {(1, 0), (1, 1)} and kinds[1, 1] == {(0, 1), (1, 0), (1, 1)}
        assert len(g.empty_tiles) == 2 * (d - 1) + 2 * (d - 1) + 3 * (d - 1) ** 2


@pytest.mark.parametrize("d,h,w", [(2, 1, 34), (4, 3, 67), (8, 5, 133)])
def test_images_with_fewer_rows_than_the_dilation(d, h, w):
    case, = [c for c in CASES if (c.dil, c.h, c.w) == (d, h, w)]
    for s in W8_SETTINGS:
        g = geometry(case, s)
        assert g.kernel == ("k_bottleneck_w8" if s >= 1 else "k_bottleneck_mfma<32>") and (g.tiles_y, g.tiles_x) == (1, 1)
        assert sorted(g.zero_row_phases) == [(py, px) for py in range(h, d) for px in range(d)]
        assert sorted(g.empty_tiles) == [(py, px, 0, 0) for py, px in sorted(g.zero_row_phases)]  # every tile of them
        assert all(hp == 1 for py, _, hp, _ in g.phases if py < h)
        assert max(wp for _, _, _, wp in g.phases) == 17


def test_dilation_16_keeps_the_four_wave_kernel():
    case, = [c for c in CASES if c.dil == 16]
    for s in W8_SETTINGS:
        g = geometry(case, s)
        assert (g.kernel, g.tw, g.tiles_y, g.tiles_x) == ("k_bottleneck_mfma<32>", 32, 1, 1)
        assert [wp for _, _, _, wp in g.phases] == [17 if px == 0 else 16 for _ in range(16) for px in range(16)]
        assert [hp for _, _, hp, _ in g.phases] == [2 if py == 0 else 1 for py in range(16) for _ in range(16)]
    assert kernel_for(16, False, 8 * 16, 16 * 16, 2) == ("k_bottleneck_o4", 16)


def test_the_table_reaches_every_kernel_the_default_knobs_can_reach():
    """of the seven entries of the dispatch, five can run with the default knobs (bnk_o4 = 2, asym_tw16 = 1, bnk_tw = 0)
    under some bnk_w8 setting, and the table runs each of them; k_bottleneck_mfma<16> and k_bottleneck_mfma_asym<32|16> need
    bnk_o4 = 0 / bnk_tw = 16 and asym_tw16 = 0"""
    assert bpc.DISPATCH_ENTRIES == ("k_bottleneck_w8", "k_bottleneck_asym_w8", "k_bottleneck_mfma<32>", "k_bottleneck_mfma<16>",
                                    "k_bottleneck_o4", "k_bottleneck_mfma_asym16x", "k_bottleneck_mfma_asym<32|16>")

    def entry(kernel):
        return "k_bottleneck_mfma_asym<32|16>" if kernel in ("k_bottleneck_mfma_asym<32>", "k_bottleneck_mfma_asym<16>") else kernel

    table = {}
    for c in CASES:
        for s in W8_SETTINGS:
            table.setdefault(entry(geometry(c, s).kernel), set()).add((case_id(c), s))
    # every shape class the dispatch can tell apart, exhaustively: which entries can the default knobs reach at all?
    reachable = {entry(kernel_for(d, asym, h, w, s)[0])
                 for d in (1, 2, 4, 8, 16) for asym in ((False, True) if d == 1 else (False,))
                 for h in (1, 8, 2 ** 16) for w in list(range(1, 40 * d, max(1, d // 2))) + [2 ** 16] for s in W8_SETTINGS}
    assert reachable == {"k_bottleneck_w8", "k_bottleneck_asym_w8", "k_bottleneck_mfma<32>", "k_bottleneck_o4",
                         "k_bottleneck_mfma_asym16x"}
    assert set(table) == reachable, sorted(reachable - set(table))
    # the shipping default alone runs both eight-wave kernels and both 8x16 kernels; the four-wave 8x32 kernel at dilation 16
    default = {entry(geometry(c, 2).kernel) for c in CASES}
    assert default == reachable
    # the two remaining entries are reachable only with other knobs, and the restatement knows them
    assert kernel_for(1, False, 8, 16, 2, bnk_o4=0) == ("k_bottleneck_mfma<16>", 16)
    assert kernel_for(1, False, 8, 17, 2, bnk_tw=16) == ("k_bottleneck_mfma<16>", 16)
    assert kernel_for(1, True, 8, 17, 0, asym_tw16=0) == ("k_bottleneck_mfma_asym<32>", 32)
    assert kernel_for(1, True, 8, 16, 2, asym_tw16=0) == ("k_bottleneck_mfma_asym<16>", 16)
    assert set(bpc.DISPATCH_ENTRIES) - reachable == {"k_bottleneck_mfma<16>", "k_bottleneck_mfma_asym<32|16>"}
    # eight-wave kernels with unequal phases at every dilation they serve, and with empty tiles at 2, 4 and 8
    for d in (2, 4, 8):
        mine = [c for c in CASES if c.dil == d and geometry(c, 2).kernel == "k_bottleneck_w8"]
        assert sum(bpc.UNEQUAL in c.props for c in mine) >= 3
        assert sum(bpc.EMPTY_TILE in c.props for c in mine) >= 2
        assert sum(bpc.NARROW_PHASE in c.props for c in mine) >= 1


def test_images_above_2_pow_28_floats_keep_the_four_wave_kernels():
    assert kernel_for(1, False, 1020, 2056, 2)[0] == "k_bottleneck_w8" and kernel_for(1, False, 1021, 2056, 2)[0] == "k_bottleneck_mfma<32>"
    assert kernel_for(1, True, 1020, 2056, 2)[0] == "k_bottleneck_asym_w8" and kernel_for(1, True, 1021, 2056, 2)[0] == "k_bottleneck_mfma_asym16x"


def test_whole_network_frame_of_the_gpu_test():
    """152 x 536 frames: 1/8 maps of 19 x 67, unequal phases at every dilation > 1, eight-wave kernels at d = 1, 2, 4"""
    h, w = 152 // 8, 536 // 8
    assert (h, w) == (19, 67) and 152 % 8 == 0 and 536 % 8 == 0
    want = {1: (67, "k_bottleneck_w8"), 2: (34, "k_bottleneck_w8"), 4: (17, "k_bottleneck_w8"), 8: (9, "k_bottleneck_o4"),
            16: (5, "k_bottleneck_o4")}
    for d, (wp, kernel) in want.items():
        assert bpc.cdiv(w, d) == wp and kernel_for(d, False, h, w, 2)[0] == kernel
        if d > 1:
            assert len({(hp, wp_) for _, _, hp, wp_ in bpc.phase_sizes(h, w, d)}) > 1
    assert kernel_for(1, True, h, w, 2)[0] == "k_bottleneck_asym_w8"


def test_bf16x3_cases_are_dispatched_to_the_split_operand_kernels():
    cases = bpc.bf16x3_cases()
    assert {c.dil for c in cases if not c.asym} == {2, 4, 8}
    assert sorted({(c.h, c.w) for c in cases if c.asym}) == [(13, 65)]
    assert all(bpc.UNEQUAL in c.props for c in cases if not c.asym)
    for c in cases:
        assert _lib.layer_dispatch("regular", 128, 128, 32, c.asym, c.h, c.w, arithmetic="bf16x3") == "fused_bf16x3", case_id(c)
    assert set(bpc.xcd_cases()) == {c for c in CASES if geometry(c, 2).empty_tiles}
