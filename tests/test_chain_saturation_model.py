"""CPU: the content of tests/test_chain_saturation_gpu.py reaches the bounds hf_flow.hip's integer widths are argued from, its winners depend
on the high bits of the sums, and its matrix reaches the kernel variants -- proved on the oracle (tests/chain_saturation_model.py).

Every step's window sums are split into SAD and bias with the oracle's public calls (bias = calc_delta_sums of two all-zero frames at
the same offsets; SAD = the delta-0 sums of the real pair minus it; ((SAD << delta) + bias) mod 2^32 must give the oracle's sums back).
Per geometry of the matrix:
  * "saturated" / "sat-y" / "sat-uv", the pair dark -> bright at the geometry's first setting (the SADs depend on no setting): no sample
    beyond the single reflection (oob == 0), the SAD of every window at every level and every candidate is 765 / 255 / 510 x its pixels
    inside the grid (a full window: x ws^2), every offset stays zero.
  * "specks", both pairs, at EVERY (delta, nb) the geometry's cases run at R 16: oob == 0 -- the reference is defined on this content.
    (Small frames carry the lattice form for that reason: tests/chain_content.py.)
  * "specks", the pair whose frame N - 1 carries the cells, at every such setting and at both steps: of all windows, a quarter at level 32
    and half at level 16 change their first-minimum argmin when the SAD part of every candidate is taken mod 2^16 before the shift and the
    bias, and half at level 8 when it is taken mod 2^15.  The floors are conditions on the INPUT, not measurements of the product.
  * the same pair at (0, 0), which a case WITH tables runs at every geometry: the largest SAD of a full window is 765 ws^2 at every level
    ws <= 32 (with delta >= 8 the chain walks the corner window out of the clean corner before level 32), and at every step of levels 16
    and 8 that can reuse by tests/flow_reuse_model.py's rule -- all but level 16 of the chain that starts there -- five reusing windows
    change under at least one of four mutations (mod 2^16, mod 2^15, clamped to 65,535, low 16 bits read as signed).
Levels 4 and 2 peak at 12,240 and 3,060, where no plausible width slip lies: they are held by the maxima and by bit-exactness alone.

Measured (python tests/chain_saturation_model.py; windows that change under the level's floor mutation / all windows, X and Y step;
r: reusing windows that change under some mutation / reusing windows; max: the levels whose maximum is reached; "tab": a case with tables
runs the setting):
  480 x 256 rs 0 SDR  ( 0,  0) tab: 32 91,100/120   16 385,416/480 r42/44,33/34       8 1868,1912/1920 r132/132,88/88     max 32..2
                      ( 8,  6)    : 32 112,112/120  16 479,473/480 r12/12,9/9         8 1920,1916/1920 r40/40,40/40       max 16..2
                      (10, 10) tab: 32 118,103/120  16 458,468/480 r0/0,1/1           8 1918,1919/1920 r36/36,62/62       max 16..2
  240 x 136 rs 2 SDR  ( 0,  0) tab: 32 28,28/40     16 113,119/135 r42/44,28/30       8 443,461/510 r79/80,74/75          max 32..2
                      ( 8,  6) tab: 32 34,33/40     16 125,124/135 r0/0,0/0           8 494,503/510 r8/8,2/2              max 8..2
                      (10, 10)    : 32 34,33/40     16 125,124/135 r0/0,0/0           8 458,485/510 r8/8,3/3              max 8..2
  240 x 136 rs 3 P010 ( 0,  0) tab: 32 30,32/40     16 108,112/135 r53/56,42/43       8 423,436/510 r131/132,151/152      max 32..2
                      ( 8,  6) tab: 32 36,33/40     16 114,118/135 r0/0,2/2           8 493,498/510 r8/8,7/7              max 16..2
                      (10, 10)    : 32 36,33/40     16 114,118/135 r0/0,2/2           8 458,449/510 r8/8,6/6              max 16..2
  480 x 270 rs 1 P010 ( 0,  0) tab: 32 82,70/135    16 332,349/510 r64/72,55/61       8 1866,1934/2040 r174/176,136/141   max 32..2
                      ( 8,  6) tab: 32 103,77/135   16 461,433/510 r0/0,1/1           8 1950,1963/2040 r20/20,51/52       max 8..2
                      (10, 10)    : 32 108,86/135   16 402,396/510 r0/0,0/0           8 1946,1931/2040 r40/40,41/41       max 8..2
  64 x 64 rs 1 SDR    ( 0,  0) tab: 32 4,4/4        16 16,16/16 r16/16,16/16          8 64,64/64 r64/64,64/64             max 32..2     (lattice)
                      (10, 10)    : 32 4,4/4        16 16,16/16 r16/16,16/16          8 64,64/64 r64/64,64/64             max 32..2
  32 x 32 rs 1 P010   ( 0,  0) tab:                 16 4,4/4 (first level)            8 16,16/16 r16/16,16/16             max 16..2     (lattice)
                      ( 8,  6)    :                 16 4,4/4                          8 16,16/16 r16/16,16/16             max 16..2
  1388 x 568 rs 0 SDR ( 0,  0) tab: 32 305,255/792  16 2519,2220/3132 r1506/1572,541/560  8 11171,9762/12354 r1270/1396,686/973  max 32..2
                      ( 8,  6)    : 32 694,665/792  16 2888,2488/3132 r16/16,17/18    8 11104,9882/12354 r106/128,159/239   max 16..2
  480 x 270 rs 2 SDR  ( 0,  0) tab: 32 79,80/135    16 314,328/510 r187/216,207/229   8 1490,1624/2040 r917/924,826/831   max 32..2
A change of the case list or of the content that drops these shows here.

The matrix's coverage is proved from tests/chain_variant_model.py: every small-level variant as .tab and as .plain and both large-window
kernels at R 16 in every tile class the model lists for them, every .anyR body (R 5 and 11), both ways of taking a large window's argmin.
Reachable only at 1080p, hence the one 1080p case: the one-wave large-window kernel's tiles across the bottom edge (it needs rs >= 2 and a
grid height that is no multiple of 4; the small shapes at rs >= 2 are 136 rows high).  Nothing the list asks for is left unreached."""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_saturation_model as S  # noqa: E402
import chain_variant_model as M  # noqa: E402
from chain_content import SAT_KINDS, frames  # noqa: E402
from flow_reuse_model import reuse_shares  # noqa: E402

GEOMETRIES = S.geometries()
UNIFORM = {"saturated": 765, "sat-y": 255, "sat-uv": 510}
_jobs = {}


def jobs():
    """Every walk of the module, started together on first use (the oracle is plain C behind ctypes: the walks run side by side)."""
    if not _jobs:
        pool = ThreadPoolExecutor(8)
        for key, cases in sorted(GEOMETRIES.items(), key=lambda kc: -M.geometry(kc[1][0]).lw * M.geometry(kc[1][0]).lh):     # the large grids first
            for c in S.configs(cases):
                _jobs[(key, "specks") + c] = pool.submit(S.analyse_specks, cases[0], *c)
            for kind in UNIFORM:
                _jobs[(key, kind)] = pool.submit(S.analyse_uniform, cases[0], kind, *min(S.configs(cases)))
        pool.shutdown(wait=False)
    return _jobs


def _id(key):
    return GEOMETRIES[key][0].name.split("-")[0]


@pytest.mark.parametrize("key", list(GEOMETRIES), ids=_id)
def test_uniform_kinds_sit_at_the_maximum(key):
    case = GEOMETRIES[key][0]
    for kind, per_pixel in UNIFORM.items():
        oob, zero_flow, sads = jobs()[(key, kind)].result()
        assert oob == 0 and zero_flow, (case.name, kind, oob)
        assert sorted(sads, reverse=True) == M.windows(case), (case.name, sorted(sads))
        for ws, values in sads.items():            # (every window, the partial ones by their pixels inside the grid)
            assert values == {per_pixel}, (case.name, kind, ws, sorted(values)[:4])


@pytest.mark.parametrize("key", list(GEOMETRIES), ids=_id)
def test_specks_reach_the_bounds_and_the_winner_depends_on_the_high_bits(key):
    cases = GEOMETRIES[key]
    g = M.geometry(cases[0])
    cfg = S.configs(cases)
    res = {c: jobs()[(key, "specks") + c].result() for c in cfg}
    small = [ws for ws in M.windows(cases[0]) if ws <= 32]
    assert cfg.get(S.FLOOR_SETTING) is True, (cases[0].name, cfg)          # a case with tables runs the setting of the maxima and the reusing floors
    for c, a in res.items():
        print(cases[0].name, c, a["oob"], a["max"], a["sens"])
        assert a["oob"] == (0, 0), (cases[0].name, c, a["oob"])
        assert set(a["sens"]) == {(ws, ax) for ws in small if ws >= 8 for ax in (0, 1)}
        for (ws, axis), v in a["sens"].items():
            mutation, share = S.FLOORS[ws]
            assert v["changed"][mutation][0] * share >= v["windows"], (cases[0].name, c, ws, "XY"[axis], mutation, v["changed"][mutation][0], v["windows"])
    a = res[S.FLOOR_SETTING]
    assert all(a["max"].get(ws) == 765 * ws * ws for ws in small), (cases[0].name, a["max"])
    reusing_steps = [(ws, axis) for (ws, axis), v in a["sens"].items() if v["can_reuse"]]
    assert reusing_steps == [(ws, axis) for ws in small[1:] if ws >= 8 for axis in (0, 1)], reusing_steps     # every step of 16 and 8 but a chain's first level
    for ws, axis in reusing_steps:
        v = a["sens"][(ws, axis)]
        assert v["any_reusing"] >= S.REUSING_FLOOR, (cases[0].name, ws, "XY"[axis], v["any_reusing"], v["reusing"])


def test_reusing_windows_follow_the_reuse_model():
    """reuse_windows is flow_reuse_model.reuse_shares' rule window by window: the same share of full-tile pixels at every step."""
    case = S.CASES[4]
    g = M.geometry(case)
    assert (g.lw, g.lh) == (240, 136)
    f = S.sat_frames(case, "specks")
    steps, _ = S.split_steps(f[2], f[3], g, 16, 0, 0, max_window=0)
    shares = reuse_shares(f[2], f[3], g, 16, 0, 0)
    n_full = (g.lw // 32) * (g.lh // 32) * 1024
    seen = 0
    for i, (st, (ws, axis, share)) in enumerate(zip(steps, shares)):
        assert (st["ws"], st["axis"]) == (ws, axis)
        if ws <= 32:
            assert abs(int(S.reuse_windows(steps, i).sum()) * ws * ws / n_full - share) < 1e-12, (ws, axis)
            seen += share > 0
    assert seen >= 6


def test_mutations():
    s = np.array([0, 32767, 32768, 48960, 65535, 65536, 137088, 195840], dtype=np.uint64)
    assert S.MUTATIONS["mod 2^16"](s).tolist() == [0, 32767, 32768, 48960, 65535, 0, 6016, 64768]
    assert S.MUTATIONS["mod 2^15"](s).tolist() == [0, 32767, 0, 16192, 32767, 0, 6016, 32000]
    assert S.MUTATIONS["clamp 65535"](s).tolist() == [0, 32767, 32768, 48960, 65535, 65535, 65535, 65535]
    assert S.MUTATIONS["signed 16"](s).tolist() == [0, 32767, 2**32 - 32768, 2**32 - 16576, 2**32 - 1, 0, 6016, 2**32 - 768]


# ------------------------------------------------------------------------------------------------
# the content
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hdr", [0, 1])
def test_saturation_kinds_are_what_they_say(hdr):
    H, W, S_ = 132, 200, 208
    bright = [255] * 4 if not hdr else [0xFFFF, 0xFF00]
    dark, grey = (0x00FF, 0x8000) if hdr else (0, 128)
    for kind in SAT_KINDS:
        a = frames(kind, H, W, bool(hdr), 77, 5, S_, 1)
        b = frames(kind, H, W, bool(hdr), 77, 5, S_, 1)
        assert len(a) == 5 and all((x == y).all() and x.dtype == (np.uint16 if hdr else np.uint8) and x.size == (H + H // 2) * S_ for x, y in zip(a, b))
        assert all((x.reshape(-1, S_)[:, W:] == 0).all() for x in a)               # the pitch is honoured: nothing lands in the padding
        for i, x in enumerate(a):
            y, uv = x.reshape(-1, S_)[:H, :W], x.reshape(-1, S_)[H:, :W]
            br = bright[(i // 2) % len(bright)]
            base = br if i & 1 else dark
            if kind == "specks":
                if i & 1:
                    assert (y == br).all() and (uv == br).all()
                else:
                    assert set(np.unique(x.reshape(-1, S_)[:, :W])) == {dark, sat_bright(hdr, i)}
                    assert (y[:64, :64] == dark).all() and (uv[:32, :64] == dark).all()         # the clean corner: 32 x 32 grid samples at rs 1
                    cells = y.reshape(H // 2, 2, W // 2, 2)
                    assert (cells == cells[:, :1, :, :1]).all()                                 # 2 x 2 luma cells
                    assert 0.2 < (y[:, W // 4:] != dark).mean() < 0.45
            else:
                assert (y == (grey if kind == "sat-uv" else base)).all() and (uv == (grey if kind == "sat-y" else base)).all(), (kind, i)
    fresh = frames("specks", H, W, bool(hdr), 77, 3, S_, 1)
    assert (fresh[0] != fresh[2]).any() and (frames("specks", H, W, bool(hdr), 78, 1, S_, 1)[0] != fresh[0]).any()
    if hdr:      # what a plane build that rounds, or lets the low byte leak, would turn into a difference
        assert dark >> 8 == 0 and dark & 0xFF == 0xFF and {b >> 8 for b in bright} == {255} and {b & 0xFF for b in bright} == {0xFF, 0}


@pytest.mark.parametrize("hdr", [0, 1])
def test_small_frames_carry_the_lattice(hdr):
    """Up to 128 luma pixels on the shorter side: luma bright exactly at the grid samples, everything else dark, in every dark frame."""
    from chain_content import SPECK_LATTICE_MAX, sat_codes
    for H, W, rs in ((64, 64, 1), (128, 128, 1), (SPECK_LATTICE_MAX, 200, 2)):
        a = frames("specks", H, W, bool(hdr), 5, 3, W + 8, rs)
        for i in (0, 2):
            bright, dark, _ = sat_codes(hdr, i)
            x = a[i].reshape(-1, W + 8)
            want = np.full((H, W), dark)
            want[::1 << rs, ::1 << rs] = bright
            assert (x[:H, :W] == want).all() and (x[H:, :W] == dark).all() and (x[:, W:] == 0).all()
        assert (a[1].reshape(-1, W + 8)[:, :W] == sat_codes(hdr, 1)[0]).all()
    assert (frames("specks", SPECK_LATTICE_MAX + 2, 200, bool(hdr), 5, 1, 0, 1)[0].reshape(-1, 200)[1::2] != sat_codes(hdr, 0)[1]).any()      # (beyond it: cells)


def sat_bright(hdr, i):
    from chain_content import sat_codes
    return sat_codes(hdr, i)[0]


# ------------------------------------------------------------------------------------------------
# the matrix
# ------------------------------------------------------------------------------------------------
def test_matrix_reaches_the_variants_and_tile_classes():
    names = [c.name for c in S.CASES]
    assert len(set(names)) == len(names) and set(S.FLAGS) <= set(names)
    got = set().union(*(M.pairs(c) for c in S.CASES))
    assert S.REQUIRED_PAIRS <= got, sorted(S.REQUIRED_PAIRS - got)
    want = {f"{v}.{k}" for v in M._SMALL for k in ("tab", "plain")} | {"big.wave1.r16", "big.wave4.r16"}
    assert {v for v, _ in S.REQUIRED_PAIRS} == want
    for v in want:
        classes = {"full", "right", "bottom"} | ({"half"} if v.startswith("level2.row") else set())
        assert {c for w, c in S.REQUIRED_PAIRS if w == v} == classes, v
    seen = set().union(*(M.labels(c) for c in S.CASES))
    assert S.REQUIRED_LABELS <= seen, sorted(S.REQUIRED_LABELS - seen)
    assert {c.R for c in S.CASES if c.R != 16} == {5, 11}
    # only the 1080p case reaches the one-wave large-window kernel's bottom tiles, and nothing else keeps it in the matrix
    big = [c for c in S.CASES if c.H == 1080]
    assert len(big) == 1 and max(c.H * c.W for c in S.CASES if c.H != 1080) <= 1088 * 1920
    others = set().union(*(M.pairs(c) for c in S.CASES if c.H != 1080))
    assert S.REQUIRED_PAIRS - others == {("big.wave1.r16", "bottom")}


def test_matrix_holds_what_the_issue_lists():
    cs = S.CASES
    grids = {}
    for c in cs:
        g = M.geometry(c)
        grids.setdefault((c.hdr, c.H, c.W, c.max_res), (g.rs, g.lw, g.lh))
    assert grids == {(0, 256, 480, 270): (0, 480, 256), (0, 544, 960, 136): (2, 240, 136), (1, 1088, 1920, 136): (3, 240, 136),
                     (1, 540, 960, 270): (1, 480, 270), (0, 128, 128, 64): (1, 64, 64), (1, 64, 64, 32): (1, 32, 32),
                     (0, 568, 1388, 1000): (0, 1388, 568), (0, 1080, 1920, 270): (2, 480, 270)}
    assert M.windows(M._c("x", 0, 128, 128, 64, 1))[0] == 32 and M.windows(M._c("x", 1, 64, 64, 32, 1))[0] == 16
    assert 64 in M.windows(M._c("x", 0, 568, 1388, 1000, 1))[M.NEIGHBOUR_FIRST_LEVEL:]
    assert {c.n for c in cs} == {1, 3, 4, 5, 16} and sum(c.n == 16 for c in cs) == 1
    for key, cases in GEOMETRIES.items():
        if key[1] != 1080:
            assert {c.tables for c in cases} == {M.ALWAYS, M.NEVER}, key
    assert {(c.delta, c.nb) for c in cs} == {(0, 0), (8, 6), (10, 10)}
    # delta 10: the shifted sum of a saturated large window wraps (765 x 256 x 256 x 2^10 > 2^32), and so does the first-level sum behind m_totalFrameDelta
    assert any(c.delta == 10 and 765 * min(M.windows(c)[0], M.geometry(c).lw) * min(M.windows(c)[0], M.geometry(c).lh) << 10 >= 1 << 32 for c in cs)
    flags = sorted(S.FLAGS.values())
    assert flags == sorted([S.NO_LAZY, S.NO_GRAPH])
    lazy_case = next(c for c in cs if S.FLAGS.get(c.name) == S.NO_LAZY)
    assert lazy_case.n > 1 and M.windows(lazy_case)[0] > 32                       # a batch with large windows: the flag changes its launches
    assert next(c for c in cs if S.FLAGS.get(c.name) == S.NO_GRAPH).n == 1         # (the flag does not count inside a batch)


def test_every_kind_runs_in_every_case():
    small = {}
    for c in S.CASES:
        kinds = S.member_kinds(c)
        assert len(kinds) == c.n and kinds[0] == "specks" and set(kinds) <= set(SAT_KINDS)
        if c.n >= 4 or c.n == 1:          # (a lone context runs the four kinds one after the other)
            assert c.n == 1 or set(kinds) == set(SAT_KINDS), c.name
        else:
            assert len(set(kinds)) == c.n
            small.setdefault(c.hdr, set()).update(kinds)
    assert small == {0: set(SAT_KINDS), 1: set(SAT_KINDS)}      # three members: every kind at that batch size, in SDR and in P010
