"""CPU model of which kernel instantiation the batched chain and the blur launch (csrc/hf_launch_plan.h plan_flow_level_small,
plan_flow_big_waves, plan_sad_tables, plan_blur; csrc/hf_calc.hip enqueue_flow_chain, choose_tab_mode).

The launchers choose by more than the frame geometry: the batch size, the resolution scalar, the search radius and the table mode each
select another instantiation, and inside a kernel a tile's position selects the body.  This module restates those selectors in Python,
it is compared with the launchers' plan functions by tests/test_chain_variant_model.py, and CASES -- the matrix tests/test_chain_variants_gpu.py runs against
the oracle -- must reach every variant and every (variant, tile class) pair the model knows.

Variant labels
  level32.four_wave.* / level32.wave.*        flow_level_small_kernel<32, false, false, TABK> / flow_level32_wave_kernel<TABK> (n >= 4)
  level16.*  level8.*                         flow_level_small_kernel<16 | 8, true, false, TABK>
  level4.row.* / level4.block.*               MapRow<4> (n <= 4) / Map<4>;   level2.* likewise, MapRow<2> with 16 x 32 tiles
      .tab    TABK: tables on, R == 16, the level reads or writes them        .plain  R == 16 without tables       .anyR  R < 16 (masked bodies)
  big.wave1.* / big.wave4.*                   flow_big_partial_kernel<1> (n >= 4 and rs >= 2) / <4>;  .r16 / .anyR
  argmin.lazy / argmin.explicit               a large-window step's argmin taken by the next launch / by flow_big_argmin_kernel
  blur.32x4.window_sums / blur.32x4.taps / blur.32x0 / blur.16x0
  tables.on / tables.off / tables.default     HF_FLAG_SAD_REUSE_ALWAYS / HF_FLAG_NO_SAD_REUSE / neither (n >= 4: decided by a timing-dependent report)
  grid.exact / grid.padded                    a launch whose unit count is / is not a multiple of the eight XCD slices (decode_tile)

Tile classes of a launch at R == 16: "full" (the tile lies inside the grid), "right" / "bottom" (it crosses that edge; a corner tile is both),
and for MapRow<2> "half": a 16-wide tile inside the grid whose 32-wide tile is not (no table body there).  At R < 16 no tile is full: "any".
"""
import collections
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import oracle  # noqa: E402  (test infrastructure)

# thresholds of the launchers (compared with the launchers' plan functions by tests/test_chain_variant_model.py)
ROW_PER_LANE_MAX_BATCH = 4        # hf_flow.hip kRowPerLaneMaxBatch
LEVEL32_ONE_WAVE_MIN_BATCH = 4    # HF_LEVEL32_ONE_WAVE_MIN_BATCH
BIG_ONE_WAVE_MIN_BATCH = 4        # HF_BIG_ONE_WAVE_MIN_BATCH
BIG_ONE_WAVE_MIN_RS = 2           # kBigOneWaveMinRs
MAX_FLOW_BATCH = 32               # hf_kernels.h kMaxFlowBatch
WINDOW_SUM_MIN_DIM = 64           # hf_kernels.hip: lw >= 64 && lh >= 64
TABLES_MIN_BATCH = 4              # hf_calc.hip choose_tab_mode: n < 4 -> off
NEIGHBOUR_FIRST_LEVEL = 4         # hf_calc.hip: use_neighbors = k >= 4

ALWAYS, NEVER, DEFAULT = "always", "never", "default"

Case = collections.namedtuple("Case", "name hdr H W max_res n R iterations blur_radius tables delta nb in_stride", defaults=(8, 6, 0))
Launch = collections.namedtuple("Launch", "window axis variant tile_classes units table_windows")

_SMALL = ["level32.four_wave", "level32.wave", "level16", "level8", "level4.row", "level4.block", "level2.row", "level2.block"]
ALL_VARIANTS = frozenset(
    [f"{v}.{k}" for v in _SMALL for k in ("tab", "plain", "anyR")] + [f"big.wave{w}.{k}" for w in (1, 4) for k in ("r16", "anyR")] +
    ["argmin.lazy", "argmin.explicit", "blur.32x4.window_sums", "blur.32x4.taps", "blur.32x0", "blur.16x0",
     "tables.on", "tables.off", "tables.default", "grid.exact", "grid.padded"])


def required_pairs():
    """Every (variant, tile class) that some geometry reaches."""
    out = set()
    for v in ALL_VARIANTS:
        if not (v.startswith("level") or v.startswith("big.")):
            continue
        if v.endswith(".anyR"):
            out.add((v, "any"))
            continue
        out |= {(v, "full"), (v, "right"), (v, "bottom")}
        if v.startswith("level2.row"):
            out.add((v, "half"))
    return out


def geometry(case):
    return oracle.make_geom(case.hdr, case.H, case.W, case.in_stride, 0, case.max_res)


def windows(case, g=None):
    """The chain's window sizes, level by level."""
    g = g or geometry(case)
    L = oracle.lib()
    ws0 = L.hfo_initial_window(g.lw, g.lh)
    return [ws0 >> k for k in range(L.hfo_iterations(ws0, case.iterations))]


def tables_on(case):
    """True / False, or None where the host decides from a report of an earlier chain."""
    if case.tables == NEVER:
        return False
    if case.tables == ALWAYS:
        return True
    return False if case.n < TABLES_MIN_BATCH else None


def _tiles(lw, lh, tw, th, r16, half_tiles):
    """(tile classes, number of tiles that take a table body)."""
    classes, tab = set(), 0
    for ty in range((lh + th - 1) // th):
        for tx in range((lw + tw - 1) // tw):
            in_x, in_y = (tx + 1) * tw <= lw, (ty + 1) * th <= lh
            if not r16:
                classes.add("any")
            elif in_x and in_y:
                if half_tiles and ((tx * tw) | 31) >= lw:
                    classes.add("half")
                else:
                    classes.add("full")
                    tab += 1
            else:
                if not in_x:
                    classes.add("right")
                if not in_y:
                    classes.add("bottom")
    return frozenset(classes), tab


def launches(case, tab=None):
    """The chain's refinement launches.  `tab`: the table mode where the case leaves it to the host (tables_on(case) is None)."""
    g = geometry(case)
    ws_list = windows(case, g)
    on = tables_on(case)
    on = tab if on is None else on
    assert on is not None, "the table mode of this case is decided at run time"
    r16 = case.R == 16
    out = []
    for k, ws in enumerate(ws_list):
        if ws > 32:
            wpb = 1 if case.n >= BIG_ONE_WAVE_MIN_BATCH and g.rs >= BIG_ONE_WAVE_MIN_RS else 4
            classes, _ = _tiles(g.lw, g.lh, 64, 4 * wpb, r16, False)
            units = ((g.lw + 63) // 64) * ((g.lh + 4 * wpb - 1) // (4 * wpb)) * case.n
            for axis in (0, 1):
                out.append(Launch(ws, axis, f"big.wave{wpb}.{'r16' if r16 else 'anyR'}", classes, units, 0))
            continue
        rows1 = case.n <= ROW_PER_LANE_MAX_BATCH and ws <= 4
        tw = 16 if rows1 and ws == 2 else 32
        sad_write = on and ws >= 4
        sad_read = on and k > 0 and ws_list[k - 1] <= 32
        tabk = r16 and (sad_read or sad_write)
        if ws == 32:
            one_wave = case.n >= LEVEL32_ONE_WAVE_MIN_BATCH
            name, waves = ("level32.wave" if one_wave else "level32.four_wave"), 1
        elif ws >= 8:
            name, waves = f"level{ws}", 4
        else:
            name, waves = f"level{ws}.{'row' if rows1 else 'block'}", (4 if rows1 or ws == 2 else 2)
        classes, tab_tiles = _tiles(g.lw, g.lh, tw, 32, r16, tw == 16)
        units = ((g.lw + tw - 1) // tw) * ((g.lh + 31) // 32) * waves * case.n
        kind = "tab" if tabk else "plain" if r16 else "anyR"
        out.append(Launch(ws, 0, f"{name}.{kind}", classes, units, case.n * tab_tiles * (tw // ws) * (32 // ws) if tabk else 0))
    return out


def argmin_labels(case):
    """How the large-window steps' argmins are taken (hf_calc.hip enqueue_flow_chain, lazy argmin on)."""
    out, pending = set(), False
    for k, ws in enumerate(windows(case)):
        nb = k >= NEIGHBOUR_FIRST_LEVEL
        if nb and pending:
            out.add("argmin.explicit"); pending = False
        for _axis in ((0, 1) if ws > 32 else (0,)):
            if pending:
                out.add("argmin.lazy"); pending = False
            if ws > 32:
                pending = True
                if nb:
                    out.add("argmin.explicit"); pending = False
    if pending:
        out.add("argmin.explicit")
    return out


def blur_variant(case):
    g = geometry(case)
    ws_list = windows(case, g)
    r = case.blur_radius
    window_sums = bool(ws_list) and ws_list[-1] == 2 and not (g.lw & 1) and not (g.lh & 1) and g.lw >= WINDOW_SUM_MIN_DIM and g.lh >= WINDOW_SUM_MIN_DIM
    if r == 4 and (case.n > 4 or window_sums):
        return "blur.32x4.window_sums" if window_sums else "blur.32x4.taps"
    if window_sums and 2 <= r <= 64 and not (r & 1):
        return "blur.32x0"
    return "blur.16x0"


def labels(case):
    """Variant labels of one case.  A case whose table mode is left to the host contributes no chain variants: which it runs is not known."""
    out = {blur_variant(case), {ALWAYS: "tables.on", NEVER: "tables.off", DEFAULT: "tables.default"}[case.tables]}
    if tables_on(case) is None:
        return out
    out |= argmin_labels(case)
    for ln in launches(case):
        out.add(ln.variant)
        out.add("grid.padded" if ln.units % 8 else "grid.exact")
    return out


def pairs(case):
    if tables_on(case) is None:
        return set()
    return {(ln.variant, c) for ln in launches(case) for c in ln.tile_classes}


def expected_table_windows(case):
    """{window: windows that take a table body, all members together} -- what hf_debug_counters reports per axis in level_windows."""
    return {ln.window: ln.table_windows for ln in launches(case) if ln.table_windows}


# ------------------------------------------------------------------------------------------------
# the window-sum blur's gather indices (hf_kernels.hip blur_flow_kernel<32, 0> and the window-sum form of <32, 4>)
# ------------------------------------------------------------------------------------------------
def blur_window_indices(dim, r, fixed4=False, clamp=True):
    """Every window index one axis of the launch gathers on a grid of `dim` pixels (dim even, windows of 2): tile origins X0 = 0, 32, ..;
    NW = 16 + r windows from X0 / 2 - r / 2 (radius fixed at 4: 20 from X0 / 2 - 2), reflected once; clamp: then clamped like mirror_flow."""
    nw = dim // 2
    count, half = (20, 2) if fixed4 else (16 + r, r // 2)
    out = []
    for x0 in range(0, dim, 32):
        for k in range(count):
            w = x0 // 2 - half + k
            w = -1 - w if w < 0 else 2 * nw - 1 - w if w >= nw else w
            out.append(min(max(w, 0), nw - 1) if clamp else w)
    return out


def blur_windows_of_outputs(dim, r):
    """Window indices (before reflection) that the outputs INSIDE the grid sum: r windows from X / 2 - r / 2, one more for odd X."""
    return [w for x in range(dim) for w in range(x // 2 - r // 2, x // 2 - r // 2 + r + (x & 1))]


# ------------------------------------------------------------------------------------------------
# the matrix (tests/test_chain_variants_gpu.py)
# ------------------------------------------------------------------------------------------------
def _c(name, hdr, H, W, max_res, n, R=16, it=0, blur=4, tables=ALWAYS, delta=8, nb=6, stride=0):
    return Case(name, hdr, H, W, max_res, n, R, it, blur, tables, delta, nb, stride)


CASES = [
    # 1080p SDR, rs 2, 480 x 270 (bottom tiles partial): the timed shape at 16, every batch-size class, both table modes
    _c("sdr1080-n16-tab", 0, 1080, 1920, 270, 16),
    _c("sdr1080-n16-notab", 0, 1080, 1920, 270, 16, tables=NEVER),
    _c("sdr1080-n4-tab", 0, 1080, 1920, 270, 4),                       # row per lane together with the one-wave launches
    _c("sdr1080-n5-notab-b2", 0, 1080, 1920, 270, 5, tables=NEVER, blur=2),      # the first block-per-lane size
    _c("sdr1080-n7-tab-b32", 0, 1080, 1920, 270, 7, blur=32, delta=3, nb=0),
    _c("sdr1080-n4-notab-b32", 0, 1080, 1920, 270, 4, tables=NEVER, blur=32, delta=10, nb=10),
    _c("sdr1080-n3-tab", 0, 1080, 1920, 270, 3),                       # below every batch threshold: four-wave level 32, four-wave large windows
    _c("sdr1080-n5-default", 0, 1080, 1920, 270, 5, tables=DEFAULT),
    _c("sdr1080-n5-R11", 0, 1080, 1920, 270, 5, R=11),
    _c("sdr1080-n4-R5", 0, 1080, 1920, 270, 4, R=5, tables=NEVER),
    _c("sdr1080-n5-it4", 0, 1080, 1920, 270, 5, it=4),                 # ends at 32: tables written, never read; the blur reads 32-windows
    _c("sdr1080-n4-it6", 0, 1080, 1920, 270, 4, it=6, blur=2),         # ends at 8
    _c("sdr1080-n7-it3", 0, 1080, 1920, 270, 7, it=3),                 # ends on a large window: the final argmin is flushed explicitly
    _c("sdr1080-n4-it3-b7", 0, 1080, 1920, 270, 4, it=3, blur=7, tables=NEVER),
    _c("sdr1080-n5-strided", 0, 1080, 1920, 270, 5, stride=2048, delta=0, nb=10),
    # 1080p / 2160p HDR
    _c("hdr1080-n5-tab", 1, 1080, 1920, 270, 5),
    _c("hdr2160-n16-tab", 1, 2160, 3840, 270, 16),                     # rs 3: the other timed shape
    _c("hdr2160-n4-notab", 1, 2160, 3840, 270, 4, tables=NEVER),
    # 240 x 136: partial tiles right and bottom; 240 = 7.5 x 32, so MapRow<2>'s last 16-wide tile is a full one inside a partial 32-wide tile
    _c("hdr1088-n5-tab", 1, 1088, 1920, 136, 5),
    _c("hdr1088-n4-tab", 1, 1088, 1920, 136, 4),
    _c("sdr544-n13-notab-b64", 0, 544, 960, 136, 13, tables=NEVER, blur=64),
    _c("sdr544-n4-notab-b64", 0, 544, 960, 136, 4, tables=NEVER, blur=64),
    _c("sdr544-n3-tab", 0, 544, 960, 136, 3),
    _c("sdr544-n3-notab", 0, 544, 960, 136, 3, tables=NEVER),
    _c("sdr544-n7-default", 0, 544, 960, 136, 7, tables=DEFAULT),
    _c("sdr544-n5-R2", 0, 544, 960, 136, 5, R=2, tables=NEVER),
    _c("sdr544-n3-R5", 0, 544, 960, 136, 3, R=5),
    # rs 1: one-wave level 32 beside the four-wave large-window kernel;  rs 0: every tile full
    _c("sdr540-n4-tab", 0, 540, 960, 270, 4),
    _c("hdr540-n13-notab", 1, 540, 960, 270, 13, tables=NEVER),
    _c("sdr256-n32-tab", 0, 256, 480, 270, 32),
    _c("sdr256-n5-notab", 0, 256, 480, 270, 5, tables=NEVER, delta=3, nb=0),
    # odd 481 x 271 grid: the blur's pixel forms inside a batch
    _c("sdr1082-n4-tab", 0, 1082, 1922, 270, 4),
    _c("sdr1082-n5-tab-b2", 0, 1082, 1922, 270, 5, blur=2),
    _c("sdr1082-n7-notab-b7", 0, 1082, 1922, 270, 7, tables=NEVER, blur=7),
    _c("sdr1082-n3-notab", 0, 1082, 1922, 270, 3, tables=NEVER),       # 481 = 30 x 16 + 1: a 16-wide tile of MapRow<2> across the right edge
    # chains that start at a small level: no large-window launches
    _c("sdr64-n32-tab", 0, 64, 64, 32, 32),                            # 32 x 32 grid: first level 16, nothing before it to reuse
    _c("sdr128-n13-tab", 0, 128, 128, 64, 13, blur=32),                # 64 x 64 grid: first level 32
    _c("hdr128-n4-default-b32", 1, 128, 128, 64, 4, tables=DEFAULT, blur=32),
    # 694 x 284 grid, wider than 512: large windows at neighbour-term levels, so a pending argmin is flushed inside the batch
    _c("sdr568x1388-n5-tab", 0, 568, 1388, 1000, 5),
]


def case(name):
    return next(c for c in CASES + DEEP_CASES if c.name == name)


# ------------------------------------------------------------------------------------------------
# resolution scalars 4, 5 and 6 (tests/test_chain_deep_rs_gpu.py; tests/test_chain_deep_rs_model.py proves what the matrix and its content reach)
# ------------------------------------------------------------------------------------------------
# (hdr, H, W, max_res, in_stride) -> (rs, lw, lh): the smallest shapes with H >= 1084, where every offset the chain can reach stays inside
# one reflection.  The chain's staged Y-row and 8-window forms stop at rs 4 and so does the fast plane kernel: at rs 5 and 6 every tile takes
# the fallback bodies and the generic kernel builds every plane, 16 or 32 phase-pair rows per luma row.
DEEP_GEOMETRIES = {
    (1, 1088, 1536, 68, 0): (4, 96, 68),        # first window 64; the last staged rs; partial tiles at the bottom
    (0, 1088, 2816, 68, 0): (4, 176, 68),       # first window 128: two large-window levels
    (0, 1088, 1536, 34, 0): (5, 48, 34),        # first window 32; 1.5 tiles wide, 2 rows below the first tile row
    (1, 1088, 2816, 34, 0): (5, 88, 34),        # first window 64
    (1, 1084, 1608, 34, 1616): (5, 51, 34),     # ragged W and H: the ceil grid's last column and row reach beyond the frame
    (1, 1088, 1536, 17, 0): (6, 24, 17),        # first window 16; the grid is smaller than one tile
    (0, 2176, 4352, 34, 0): (6, 68, 34),        # large windows at rs 6
    (0, 1084, 1608, 17, 0): (6, 26, 17),        # ragged at rs 6
}

DEEP_CASES = [
    # rs 4, 96 x 68 from P010
    _c("r4-hdr1536-n1-notab", 1, 1088, 1536, 68, 1, tables=NEVER),
    _c("r4-hdr1536-n3-tab", 1, 1088, 1536, 68, 3, delta=0, nb=0),
    _c("r4-hdr1536-n5-default", 1, 1088, 1536, 68, 5, tables=DEFAULT),
    _c("r4-hdr1536-n13-notab", 1, 1088, 1536, 68, 13, tables=NEVER, delta=10, nb=10),
    _c("r4-hdr1536-n5-R11", 1, 1088, 1536, 68, 5, R=11),
    _c("r4-hdr1536-n3-it3-b2", 1, 1088, 1536, 68, 3, it=3, blur=2, tables=NEVER),       # ends at 16: the blur's pixel form at radius 2
    # rs 4, 176 x 68
    _c("r4-sdr2816-n1-tab", 0, 1088, 2816, 68, 1, delta=10, nb=10),
    _c("r4-sdr2816-n3-notab", 0, 1088, 2816, 68, 3, tables=NEVER),
    _c("r4-sdr2816-n5-notab", 0, 1088, 2816, 68, 5, tables=NEVER),
    _c("r4-sdr2816-n13-tab", 0, 1088, 2816, 68, 13, delta=0, nb=0),
    _c("r4-sdr2816-n3-R5", 0, 1088, 2816, 68, 3, R=5, tables=NEVER),
    # rs 5, 48 x 34
    _c("r5-sdr1536-n1-tab", 0, 1088, 1536, 34, 1),
    _c("r5-sdr1536-n3-notab-b2", 0, 1088, 1536, 34, 3, tables=NEVER, blur=2, delta=0, nb=0),
    _c("r5-sdr1536-n5-tab", 0, 1088, 1536, 34, 5, delta=10, nb=10),
    _c("r5-sdr1536-n13-tab", 0, 1088, 1536, 34, 13),
    _c("r5-sdr1536-n3-R5", 0, 1088, 1536, 34, 3, R=5),
    # rs 5, 88 x 34 from P010
    _c("r5-hdr2816-n3-tab", 1, 1088, 2816, 34, 3),
    _c("r5-hdr2816-n5-notab", 1, 1088, 2816, 34, 5, tables=NEVER, delta=0, nb=0),
    _c("r5-hdr2816-n13-tab-it3", 1, 1088, 2816, 34, 13, it=3),                          # ends at 16
    _c("r5-hdr2816-n1-notab", 1, 1088, 2816, 34, 1, tables=NEVER, delta=10, nb=10),
    _c("r5-hdr2816-n5-R11", 1, 1088, 2816, 34, 5, R=11, tables=NEVER),
    # rs 5, ragged 51 x 34 from P010 rows of 1616
    _c("r5-hdr1608-n3-notab", 1, 1084, 1608, 34, 3, tables=NEVER, stride=1616),
    _c("r5-hdr1608-n13-tab", 1, 1084, 1608, 34, 13, stride=1616, delta=0, nb=0),
    _c("r5-hdr1608-n5-tab", 1, 1084, 1608, 34, 5, stride=1616, delta=10, nb=10),
    # rs 6, 24 x 17 from P010: no tile lies inside the grid
    _c("r6-hdr1536-n1-tab", 1, 1088, 1536, 17, 1, delta=0, nb=0),
    _c("r6-hdr1536-n3-tab-b2", 1, 1088, 1536, 17, 3, blur=2),
    _c("r6-hdr1536-n5-notab", 1, 1088, 1536, 17, 5, tables=NEVER, delta=10, nb=10),
    _c("r6-hdr1536-n13-tab", 1, 1088, 1536, 17, 13),
    _c("r6-hdr1536-n5-tab", 1, 1088, 1536, 17, 5, delta=0, nb=0),
    # rs 6, 68 x 34 from 2176 x 4352
    _c("r6-sdr4352-n3-tab", 0, 2176, 4352, 34, 3),
    _c("r6-sdr4352-n5-notab-it3", 0, 2176, 4352, 34, 5, it=3, tables=NEVER),            # ends at 16
    _c("r6-sdr4352-n5-R11", 0, 2176, 4352, 34, 5, R=11),
    # rs 6, ragged 26 x 17
    _c("r6-sdr1608-n3-notab", 0, 1084, 1608, 17, 3, tables=NEVER, delta=10, nb=10),
    _c("r6-sdr1608-n5-tab", 0, 1084, 1608, 17, 5),
    _c("r6-sdr1608-n1-notab", 0, 1084, 1608, 17, 1, tables=NEVER),
    _c("r6-sdr1608-n3-R5", 0, 1084, 1608, 17, 3, R=5, tables=NEVER),
]
# flags beside the table mode (tests/test_chain_deep_rs_gpu.py): a batch with large windows without the lazy argmin, a lone context without its graph
DEEP_NO_LAZY, DEEP_NO_GRAPH = "r5-hdr2816-n5-notab", "r5-hdr2816-n1-notab"

# Content of the members (tests/chain_content.py): the four drift directions and full-range noise first, so that every batch of five has
# them -- windows at each frame edge then settle on offsets that point out of the frame -- then the other kinds on which the oracle samples
# nothing beyond the single reflection at these shapes.
DEEP_KINDS = ["drift-se", "drift-nw", "noise", "drift-sw", "drift-ne", "chaotic", "patches", "pan64", "static"]


def deep_member_kinds(c):
    """Content of member i of a deep case.  A lone context runs the first four kinds one after the other; three members start where the
    case's place in DEEP_CASES says, so that every kind runs at that size too (tests/test_chain_deep_rs_model.py: every geometry runs the drifts and
    noise, every resolution scalar every kind)."""
    if c.n == 1:
        return DEEP_KINDS[:4]
    pool = DEEP_KINDS[:5] if c.H > 1088 else DEEP_KINDS       # (the 2176 x 4352 frames: the kinds that take no seconds to draw)
    s = [x.name for x in DEEP_CASES].index(c.name) * 3 if c.n == 3 else 0
    return [pool[(s + i) % len(pool)] for i in range(c.n)]


def deep_geom_key(c):
    return (c.hdr, c.H, c.W, c.max_res, c.in_stride)
