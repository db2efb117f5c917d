"""Case table for the 128-channel bottleneck kernels on UNEQUAL dilation phases, and the launcher's arithmetic restated in
plain Python (launch_bottleneck_mfma / decode_tile in csrc/ssal_bottleneck_mfma.hip).  No GPU, no torch.

A layer of dilation d splits its H x W map into d x d phase sub-images; phase (py, px) has
Hp = ceil((H - py) / d) rows and Wp = ceil((W - px) / d) columns.  The launcher picks the kernel and the tile width from the
LARGEST phase and sizes the grid N * d * d * tiles_y * tiles_x for it; a tile that lies past a shorter phase is empty.
Each case below is (layer, dil, asym, H, W) plus the properties it is listed for; test_bottleneck_phase_cases_cpu.py
asserts that every case has them, test_gpu_bottleneck_phases.py runs them."""
from collections import namedtuple

C = 128   # channels of the block
TH = 8    # tile rows of every kernel of the family
W8_MAX_ELEMS = 1 << 28  # floats per image the eight-wave kernels take

# every kernel symbol launch_bottleneck_mfma can launch for a 128-channel block
KERNELS = ("k_bottleneck_w8", "k_bottleneck_asym_w8", "k_bottleneck_mfma<32>", "k_bottleneck_mfma<16>", "k_bottleneck_o4",
           "k_bottleneck_mfma_asym16x", "k_bottleneck_mfma_asym<32>", "k_bottleneck_mfma_asym<16>")
# the dispatch has seven entries: the two widths of k_bottleneck_mfma_asym are one template behind one condition
DISPATCH_ENTRIES = ("k_bottleneck_w8", "k_bottleneck_asym_w8", "k_bottleneck_mfma<32>", "k_bottleneck_mfma<16>",
                    "k_bottleneck_o4", "k_bottleneck_mfma_asym16x", "k_bottleneck_mfma_asym<32|16>")
W8_SETTINGS = (0, 1, 2)
DEFAULT_KNOBS = dict(bnk_o4=2, asym_tw16=1, bnk_tw=0)

REGULAR_LAYER = {1: "Bottleneck2_1", 2: "Bottleneck2_2", 4: "Bottleneck2_4", 8: "Bottleneck2_6", 16: "Bottleneck2_8"}
ASYM_LAYERS = ("Bottleneck2_3", "Bottleneck3_7")

# properties a case can be listed for (checked by geometry(), see has_property)
O4_SIDE = "o4_side"              # largest phase exactly 16 wide: the 8x16 kernel under every setting
W8_SIDE = "w8_side"              # largest phase 17 wide: first width of the 8x32 kernels
UNEQUAL = "unequal"              # the d x d phases are not all the same size
NARROW_PHASE = "narrow_phase"    # a 32-wide-tile launch with at least one non-empty phase <= 16 wide
EMPTY_TILE = "empty_tile"        # at least one tile of the grid lies past its (non-empty) phase, or its phase has no pixel
ZERO_ROWS = "zero_rows"          # H < d: whole phase rows have Hp = 0
NO_EMPTY_TILE = "no_empty_tile"  # ragged in both axes, yet every tile of every phase holds a pixel
SHORT_COLUMN = "short_column"    # asymmetric block, H < 5: every pixel's (5,1) window reaches into the SAME padding
ALL_PADDING_TAPS = "all_padding_taps"  # H = 1: every off-centre (5,1) tap row is padding
MULTI_TILE = "multi_tile"        # three x-tiles, the last one column wide, and two y-tiles
D16_KEEPS_MFMA32 = "d16_keeps_mfma32"  # dilation 16: k_bottleneck_mfma<32> under every bnk_w8 setting

Case = namedtuple("Case", "layer dil asym h w props")


def _regular(d, h, w, *props):
    return Case(REGULAR_LAYER[d], d, False, h, w, tuple(props))


def _cases():
    out = []
    for d in (1, 2, 4, 8):  # dispatch boundary
        out.append(_regular(d, 8 * d, 16 * d, O4_SIDE))
        # for d > 1 phase column 0 is 17 wide and every other phase 16 wide inside the 32-wide tile
        out.append(_regular(d, 8 * d, 16 * d + 1, W8_SIDE, *((UNEQUAL, NARROW_PHASE) if d > 1 else ())))
    for d, h, w in ((2, 17, 65), (4, 33, 129), (8, 65, 257)):  # phases 33 / 32 wide, 9 / 8 high
        out.append(_regular(d, h, w, UNEQUAL, EMPTY_TILE))
    for d, h, w in ((4, 11, 67), (8, 11, 133)):
        out.append(_regular(d, h, w, UNEQUAL, NARROW_PHASE, NO_EMPTY_TILE))
    for d, h, w in ((2, 1, 34), (4, 3, 67), (8, 5, 133)):
        # (1, 34): both phase columns are 17 wide; the other two also hold 16-wide phases
        out.append(_regular(d, h, w, UNEQUAL, ZERO_ROWS, EMPTY_TILE, *((NARROW_PHASE,) if d > 2 else ())))
    out.append(_regular(16, 17, 257, W8_SIDE, UNEQUAL, NARROW_PHASE, D16_KEEPS_MFMA32))
    for name in ASYM_LAYERS:
        out.append(Case(name, 1, True, 8, 16, (O4_SIDE,)))
        out.append(Case(name, 1, True, 8, 17, (W8_SIDE,)))
        out.append(Case(name, 1, True, 1, 33, (SHORT_COLUMN, ALL_PADDING_TAPS)))
        out.append(Case(name, 1, True, 3, 40, (SHORT_COLUMN,)))
        out.append(Case(name, 1, True, 13, 65, (MULTI_TILE,)))
    return tuple(out)


CASES = _cases()


def case_id(c):
    return "%s-d%d-%dx%d" % (c.layer, c.dil, c.h, c.w)


def cdiv(a, b):
    return (a + b - 1) // b


def phase_sizes(h, w, dil):
    """[(py, px, Hp, Wp)] in decode_tile's order; Hp = 0 where H <= py"""
    return [(py, px, cdiv(h - py, dil), cdiv(w - px, dil)) for py in range(dil) for px in range(dil)]


def kernel_for(dil, asym, h, w, bnk_w8, bnk_o4=2, asym_tw16=1, bnk_tw=0):
    """the profile row launch_bottleneck_mfma files the launch under, and that kernel's tile width"""
    wp = cdiv(w, dil)  # largest phase sub-image
    o4 = (not asym) and (bnk_o4 == 1 or (bnk_o4 == 2 and wp <= 16))
    w8_shape = wp > 16 and bnk_tw != 16 and h * w * C <= W8_MAX_ELEMS
    w8 = (not asym) and (not o4) and dil <= 8 and bnk_w8 >= 1 and w8_shape
    asym_w8 = asym and bnk_w8 >= 2 and w8_shape
    asym16x = asym and asym_tw16 != 0 and not asym_w8
    wide = (wp > 16 and bnk_tw != 16 and not o4 and not asym16x) or w8 or asym_w8
    tw = 32 if wide else 16
    if asym_w8:
        name = "k_bottleneck_asym_w8"
    elif w8:
        name = "k_bottleneck_w8"
    elif asym16x:
        name = "k_bottleneck_mfma_asym16x"
    elif asym:
        name = "k_bottleneck_mfma_asym<%d>" % tw
    elif o4:
        name = "k_bottleneck_o4"
    else:
        name = "k_bottleneck_mfma<%d>" % tw
    return name, tw


Geometry = namedtuple("Geometry", "kernel tw tiles_y tiles_x phases tiles_per_image empty_tiles narrow_phases zero_row_phases")


def geometry(case, bnk_w8, **knobs):
    """kernel, grid and the per-phase facts of one launch of this case (per image)"""
    kernel, tw = kernel_for(case.dil, case.asym, case.h, case.w, bnk_w8, **knobs)
    d = case.dil
    tiles_y, tiles_x = cdiv(cdiv(case.h, d), TH), cdiv(cdiv(case.w, d), tw)
    phases = phase_sizes(case.h, case.w, d)
    empty = [(py, px, ty, tx) for py, px, hp, wp in phases for ty in range(tiles_y) for tx in range(tiles_x)
             if ty * TH >= hp or tx * tw >= wp]  # decode_tile's t.empty
    narrow = [(py, px) for py, px, hp, wp in phases if tw == 32 and hp > 0 and 0 < wp <= 16]
    zero = [(py, px) for py, px, hp, wp in phases if hp == 0]
    return Geometry(kernel, tw, tiles_y, tiles_x, phases, d * d * tiles_y * tiles_x, empty, narrow, zero)


def is_eight_wave(kernel):
    return kernel in ("k_bottleneck_w8", "k_bottleneck_asym_w8")


def has_property(case, prop):
    """does the case have the property, under the launch the shipping default (bnk_w8 = 2) makes?"""
    g = geometry(case, 2)
    sizes = {(hp, wp) for _, _, hp, wp in g.phases}
    wp_max = cdiv(case.w, case.dil)
    if prop == O4_SIDE:
        return wp_max == 16
    if prop == W8_SIDE:
        return wp_max == 17
    if prop == UNEQUAL:
        return len(sizes) > 1
    if prop == NARROW_PHASE:
        return g.tw == 32 and len(g.narrow_phases) > 0
    if prop == EMPTY_TILE:
        return len(g.empty_tiles) > 0
    if prop == NO_EMPTY_TILE:
        return len(g.empty_tiles) == 0 and len({hp for hp, _ in sizes}) > 1 and len({wp for _, wp in sizes}) > 1
    if prop == ZERO_ROWS:
        return case.h < case.dil and len(g.zero_row_phases) == (case.dil - case.h) * case.dil
    if prop == SHORT_COLUMN:
        return case.asym and case.h < 5
    if prop == ALL_PADDING_TAPS:
        return case.asym and case.h == 1
    if prop == MULTI_TILE:
        return g.tw == 32 and g.tiles_x == 3 and case.w - 2 * g.tw == 1 and g.tiles_y == 2
    if prop == D16_KEEPS_MFMA32:
        return case.dil == 16 and all(geometry(case, s).kernel == "k_bottleneck_mfma<32>" for s in W8_SETTINGS)
    raise KeyError(prop)


def xcd_cases():
    """the cases whose grid holds per-phase empty tiles: they also run bnk_xcd = 0 against bnk_xcd = 1"""
    return tuple(c for c in CASES if EMPTY_TILE in c.props)


def bf16x3_cases():
    """the unequal-phase cases of dilation 2, 4 and 8 and the asymmetric (13, 65) case"""
    return tuple(c for c in CASES if (c.dil in (2, 4, 8) and UNEQUAL in c.props) or (c.asym and (c.h, c.w) == (13, 65)))
