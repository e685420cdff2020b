"""CPU: the matrix and the content of tests/test_chain_deep_rs_gpu.py (chain_variant_model.DEEP_CASES: resolution scalars 4, 5 and 6) reach
what they are for -- proved on the oracle and on flow_reuse_model.chain_steps alone.  These are conditions on the INPUT, not measurements
of the product.

Per geometry of DEEP_GEOMETRIES, over every run its cases make (each distinct (R, iterations, delta, nb) x each content kind of its members
x both pairs):
  * oob == 0 for every pair: the reference is defined on all of it;
  * the final offsets' x phase pairs (offset_x & (2^rs - 1)) >> 1 take ALL 2^rs / 2 values -- every phase-pair row of the plane is read by
    some winner -- and their y row phases offset_y & (2^rs - 1) at least three quarters of the 2^rs values;
  * some window's winner samples beyond each of the four frame edges (cx 2^rs + offset_x < 0, >= W; cy 2^rs + offset_y < 0, >= H), so the
    margins' reflection and, on the ragged shapes, the out-of-frame phases of the ceil grid's last column are read on both sides.
White noise alone leaves x pairs unreached on the 24 x 17 grid and hardly reaches the right and the bottom edge (the candidates lean to
the negative side: -64 .. +49 a level).  The "drift" kinds of tests/chain_content.py close both: a noise field seen
through a frame that moves by (+-75, +-67) pixels a frame, one kind per direction -- odd, and beyond 2^6: on an aligned shape the last
grid column and row lie 2^rs short of the edge, so a smaller step never crosses the right or the bottom edge at rs 6.

Measured (python tests/test_chain_deep_rs_model.py; runs = chains walked; x pairs and y phases reached / all; windows of the final offsets
that sample beyond the left, right, top and bottom edge, all runs together; the largest |offset|):
   96 x 68 rs 4 P010 runs  50  oob 0  x pairs 8/8  y phases 16/16  beyond L/R/T/B 5762/3012/6516/3668  reach 226
  176 x 68 rs 4 SDR  runs  44  oob 0  x pairs 8/8  y phases 16/16  beyond L/R/T/B 4612/1732/6398/4926  reach 198
   48 x 34 rs 5 SDR  runs  40  oob 0  x pairs 16/16  y phases 32/32  beyond L/R/T/B 1288/440/1458/292  reach 213
   88 x 34 rs 5 P010 runs  52  oob 0  x pairs 16/16  y phases 32/32  beyond L/R/T/B 1784/626/3234/1502  reach 163
   51 x 34 rs 5 P010 runs  34  oob 0  x pairs 16/16  y phases 32/32  beyond L/R/T/B 970/434/1199/270  reach 227
   24 x 17 rs 6 P010 runs  38  oob 0  x pairs 32/32  y phases 64/64  beyond L/R/T/B 379/38/504/8  reach 173
   68 x 34 rs 6 SDR  runs  26  oob 0  x pairs 32/32  y phases 64/64  beyond L/R/T/B 396/114/1164/154  reach 119
   26 x 17 rs 6 SDR  runs  22  oob 0  x pairs 32/32  y phases 62/64  beyond L/R/T/B 185/63/188/2  reach 163
A change of the case list or of the content that drops these shows here.

The matrix: every label of DEEP_LABELS below and every (variant, tile class) pair of chain_variant_model.required_pairs() is reached, the launch-plan probe
decides every launch of every case as the model does, no case at rs >= 5 defers its phase planes (plane_emission_geometry stops at rs 4: the
generic kernel builds every plane there), and the plane layout restated in tests/phase_plane_model.py is the compiled header's."""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_variant_model as M  # noqa: E402
import launch_plan_probe  # noqa: E402
import phase_plane_model as P  # noqa: E402
import test_chain_variant_model as T  # noqa: E402
from chain_content import DRIFT_KINDS, DRIFT_STEP, frames, kind_seed  # noqa: E402
from flow_reuse_model import chain_steps  # noqa: E402

probe = T.probe        # (the module's fixture: the compiled launch-plan header)

GEOMETRIES = {}
for _case in M.DEEP_CASES:
    GEOMETRIES.setdefault(M.deep_geom_key(_case), []).append(_case)
_jobs = {}


def runs_of(cases):
    """{(R, iterations, delta, nb): kinds} -- the distinct chains the geometry's cases run, with the content of their members."""
    out = {}
    for c in cases:
        out.setdefault((c.R, c.iterations, c.delta, c.nb), set()).update(M.deep_member_kinds(c))
    return out


def walk(f1, f2, g, R, iterations, delta, nb):
    """(oob, final offsets) of the oracle's chain, step by step."""
    oob, off = 0, None
    for st in chain_steps(f1, f2, g, R, delta, nb, iterations, with_sums=True):
        oob += st[6]
        off = st[4]
    return oob, off


def analyse(key):
    """dict(runs, oob, xpairs, yphases, edges = windows beyond [left, right, top, bottom], reach) of one geometry."""
    cases = GEOMETRIES[key]
    c0 = cases[0]
    g = M.geometry(c0)
    fr, xs, ys, edges, oob_total, n_runs, reach = {}, set(), set(), np.zeros(4, dtype=np.int64), 0, 0, 0
    mask = (1 << g.rs) - 1
    cx, cy = (np.arange(g.lw) << g.rs)[None, :], (np.arange(g.lh) << g.rs)[:, None]
    for (R, it, delta, nb), kinds in sorted(runs_of(cases).items()):
        for kind in sorted(kinds):
            if kind not in fr:
                fr[kind] = frames(kind, c0.H, c0.W, bool(c0.hdr), kind_seed(kind), 4, c0.in_stride, g.rs)
            for pair in (1, 2):
                oob, off = walk(fr[kind][pair], fr[kind][pair + 1], g, R, it, delta, nb)
                oob_total += oob
                n_runs += 1
                ox, oy = off[0].astype(np.int64), off[1].astype(np.int64)
                xs.update(np.unique((ox & mask) >> 1).tolist())
                ys.update(np.unique(oy & mask).tolist())
                edges += [int((cx + ox < 0).sum()), int((cx + ox >= g.W).sum()), int((cy + oy < 0).sum()), int((cy + oy >= g.H).sum())]
                reach = max(reach, int(np.abs(off).max()))
    return dict(runs=n_runs, oob=oob_total, xpairs=len(xs), yphases=len(ys), edges=edges.tolist(), reach=reach)


def jobs():
    """Every geometry's walk, started together on first use (the oracle is plain C behind ctypes), the large grids first."""
    if not _jobs:
        pool = ThreadPoolExecutor(8)
        for key in sorted(GEOMETRIES, key=lambda k: -k[1] * k[2]):
            _jobs[key] = pool.submit(analyse, key)
        pool.shutdown(wait=False)
    return _jobs


def _id(key):
    return GEOMETRIES[key][0].name.rsplit("-n", 1)[0]


@pytest.mark.parametrize("key", list(GEOMETRIES), ids=_id)
def test_content_reaches_every_phase_and_every_edge(key):
    g = M.geometry(GEOMETRIES[key][0])
    a = jobs()[key].result()
    print(_id(key), a)
    assert a["oob"] == 0, (key, a)
    assert a["xpairs"] == max(1, (1 << g.rs) // 2), (key, a)
    assert 4 * a["yphases"] >= 3 * (1 << g.rs), (key, a)
    assert min(a["edges"]) >= 1, (key, a)


def test_geometries_are_the_listed_grids():
    assert set(GEOMETRIES) == set(M.DEEP_GEOMETRIES)
    firsts = {}
    for key, cases in GEOMETRIES.items():
        g = M.geometry(cases[0])
        assert (g.rs, g.lw, g.lh) == M.DEEP_GEOMETRIES[key], (key, g.rs, g.lw, g.lh)
        assert g.H >= 1084 and (g.H >> g.rs) <= key[3] < (g.H >> (g.rs - 1))
        firsts[M.DEEP_GEOMETRIES[key]] = M.windows(cases[0])[0]
        assert (g.H + g.H // 2) * g.in_stride * (2 if g.hdr else 1) <= 14.3e6            # the largest frame: 14 MB
    assert firsts == {(4, 96, 68): 64, (4, 176, 68): 128, (5, 48, 34): 32, (5, 88, 34): 64, (5, 51, 34): 32, (6, 24, 17): 16, (6, 68, 34): 64,
                      (6, 26, 17): 16}
    # ragged: the ceil grid's last column and row carry phases beyond the frame
    for key in ((1, 1084, 1608, 34, 1616), (0, 1084, 1608, 17, 0)):
        rs, lw, lh = M.DEEP_GEOMETRIES[key]
        assert (lw << rs) > key[2] > ((lw - 1) << rs) and (lh << rs) > key[1] > ((lh - 1) << rs)


def test_matrix_holds_what_the_issue_lists():
    cs = M.DEEP_CASES
    names = [c.name for c in cs]
    assert len(set(names)) == len(names) and 28 <= len(cs) <= 36
    assert {c.n for c in cs} == {1, 3, 5, 13}
    assert {c.tables for c in cs} == {M.ALWAYS, M.NEVER, M.DEFAULT} and sum(c.tables == M.DEFAULT for c in cs) == 1
    by_rs = {}
    for c in cs:
        by_rs.setdefault(M.geometry(c).rs, []).append(c)
    assert sorted(by_rs) == [4, 5, 6]
    for rs, group in by_rs.items():
        assert {c.n for c in group} == {1, 3, 5, 13}, rs
        assert sorted(c.R for c in group if c.R != 16) == [5, 11], rs
        assert {(c.delta, c.nb) for c in group} == {(8, 6), (0, 0), (10, 10)}, rs
        assert sum(c.iterations == 3 for c in group) == 1 and {c.iterations for c in group} == {0, 3}, rs
        assert sum(c.blur_radius == 2 for c in group) == 1 and {c.blur_radius for c in group} == {4, 2}, rs
        assert all(M.blur_variant(c) == "blur.16x0" for c in group if c.blur_radius == 2), rs       # the pixel form
        assert {M.tables_on(c) for c in group if c.n == 1} == {True, False}, rs                   # a lone context in both table modes
    for key, cases in GEOMETRIES.items():
        assert {M.ALWAYS, M.NEVER} <= {c.tables for c in cases}, key
        assert any(c.n > 1 and M.tables_on(c) and c.R == 16 for c in cases), key                  # the counters are checked on every grid
    lazy, graph = M.case(M.DEEP_NO_LAZY), M.case(M.DEEP_NO_GRAPH)
    assert lazy.n > 1 and M.windows(lazy)[0] > 32 and M.geometry(lazy).rs >= 5
    assert graph.n == 1 and M.geometry(graph).rs >= 5


def test_every_geometry_runs_the_drifts_and_every_scalar_every_kind():
    assert set(DRIFT_KINDS) < set(M.DEEP_KINDS) and all(d & 1 and d > 64 for d in DRIFT_STEP)
    by_rs = {}
    for key, cases in GEOMETRIES.items():
        kinds = set().union(*(M.deep_member_kinds(c) for c in cases))
        assert set(DRIFT_KINDS) | {"noise"} <= kinds, (key, sorted(kinds))
        by_rs.setdefault(M.DEEP_GEOMETRIES[key][0], set()).update(kinds)
    assert by_rs == {rs: set(M.DEEP_KINDS) for rs in (4, 5, 6)}
    for c in M.DEEP_CASES:
        k = M.deep_member_kinds(c)
        assert len(k) == (4 if c.n == 1 else c.n) and (c.n > len(M.DEEP_KINDS) or len(set(k)) == len(k)), c.name


# ------------------------------------------------------------------------------------------------
# the variants and tile classes of the matrix
# ------------------------------------------------------------------------------------------------
_SM = ("level32.four_wave", "level32.wave", "level16", "level8", "level4.row", "level4.block", "level2.row", "level2.block")
DEEP_LABELS = frozenset(
    [f"{v}.{k}" for v in _SM for k in ("tab", "plain", "anyR")] + [f"big.wave{w}.{k}" for w in (1, 4) for k in ("r16", "anyR")] +
    ["argmin.lazy", "blur.32x4.window_sums", "blur.32x4.taps", "blur.16x0", "tables.on", "tables.off", "tables.default",
     "grid.exact", "grid.padded"])
# (argmin.explicit: no deep chain ends on a large window or carries one at a neighbour-term level; the case without the lazy argmin runs that
#  kernel.  blur.32x0: the radius-2 cases run on grids below 64 and on a chain that ends at 16 -- the pixel form.)
DEEP_PAIRS_MISSING = frozenset()


def test_matrix_reaches_its_variants_and_tile_classes():
    seen = set().union(*(M.labels(c) for c in M.DEEP_CASES))
    assert seen == DEEP_LABELS, (sorted(DEEP_LABELS - seen), sorted(seen - DEEP_LABELS))
    got = set().union(*(M.pairs(c) for c in M.DEEP_CASES))
    assert M.required_pairs() - got == DEEP_PAIRS_MISSING, (sorted(M.required_pairs() - got), sorted(DEEP_PAIRS_MISSING - (M.required_pairs() - got)))
    # per resolution scalar: what staging's end at rs 4 leaves to the fallback bodies is run in every tile class the grids have
    for rs in (4, 5, 6):
        at = set().union(*(M.pairs(c) for c in M.DEEP_CASES if M.geometry(c).rs == rs))
        for v in ("level16", "level8", "level4.row", "level4.block", "level2.row", "level2.block"):
            for k in ("tab", "plain"):
                name = "%s.%s" % (v, k)
                assert (name, "bottom") in at and ((name, "right") in at or (v == "level2.row" and (name, "half") in at)), (rs, name)      # (176 = 11 x 16)
            assert ("%s.anyR" % v, "any") in at, (rs, v)
        assert {v for v, _ in at} >= {"big.wave4.r16", "big.wave1.r16", "big.wave1.anyR"}, rs
    # rs 6, 24 x 17 and 26 x 17: no 32 x 32 tile lies inside the grid -- every window goes through an edge body, the table counters read 0 levels
    for c in M.DEEP_CASES:
        g = M.geometry(c)
        if g.lh == 17 and M.tables_on(c) is not None:
            assert not any("full" in ln.tile_classes for ln in M.launches(c)), c.name
            assert M.expected_table_windows(c) == {}, c.name


@pytest.mark.parametrize("case", M.DEEP_CASES, ids=lambda c: c.name)
def test_chain_plans_equal_the_model_on_the_deep_matrix(probe, case):
    T.test_chain_plans_equal_the_model_on_the_matrix(probe, case)
    T.test_stale_table_invariant_of_the_matrix(case)
    g = M.geometry(case)
    for n in (1, 3, 4, 5, 13, 32):
        assert probe.plan_flow_big_waves(n, g.rs) == (1 if n >= M.BIG_ONE_WAVE_MIN_BATCH else 4)


@pytest.mark.parametrize("case", M.DEEP_CASES, ids=lambda c: c.name)
def test_no_case_beyond_rs_4_defers_its_planes(probe, case):
    g = M.geometry(case)
    gt = T.g_tuple(g)
    iters = P.max_iterations(g.lw, g.lh)
    assert (1 << iters) == M.windows(M._c("x", *case[1:5], 1))[0]
    if g.rs >= 5:
        for n in sorted({case.n, 3, 16, 32}):
            assert not probe.can_build_planes(gt, iters, n), (case.name, n)


# ------------------------------------------------------------------------------------------------
# the plane layout (tests/phase_plane_model.py) against the compiled header
# ------------------------------------------------------------------------------------------------
def test_plane_layout_model_equals_the_header(probe):
    geoms = {M.deep_geom_key(c): M.geometry(c) for c in M.CASES + M.DEEP_CASES}
    seen = set()
    for g in geoms.values():
        iters = P.max_iterations(g.lw, g.lh)
        assert iters == M.oracle.lib().hfo_initial_window(g.lw, g.lh).bit_length() - 1
        want = probe.phase_layout(T.g_tuple(g), iters)
        assert tuple(P.layout(g.H, g.rs, g.lw, g.lh)) == tuple(want), (g.H, g.W, g.rs, want)
        seen.add(g.rs)
        assert want.lwp >= g.lw + 2 * want.mx + 4
        if g.rs >= 4:
            assert (want.mx << g.rs) <= g.W        # the deep shapes: a margin is one reflection deep at most, the clamp behind it never acts
    assert seen == set(range(7))


def test_plane_model_on_a_known_frame():
    """8 x 8 at rs 2 with a margin of 4 columns: element by element from the documented formula."""
    H = W = 8
    f = (np.arange(H * W * 3 // 2, dtype=np.int64).reshape(-1, W) * 517 % 65536).astype(np.uint16)
    L = P.Layout(2, 4, 2, 4, 32, 0)
    pl = P.plane(f.reshape(-1), True, H, W, 0, L, 2)
    assert pl.shape == (8, 2, 10)
    t = f >> 8
    refl = lambda x: min(max(2 * W - x - 1 if x >= W else -x - 1 if x < 0 else x, 0), W - 1)
    for y in range(H):
        for ph2 in range(2):
            for j in range(-4, 6):
                x = 4 * j + 2 * ph2
                xa, xb = refl(x), refl(x + 1)
                want = int(t[y, xa]) | int(t[y, xb]) << 8 | int(t[H + y // 2, xa & ~1]) << 16 | int(t[H + y // 2, (xa & ~1) + 1]) << 24
                assert int(pl[y, ph2, j + 4]) == want, (y, ph2, j)
    assert int(pl[0, 0, 4]) == int(t[0, 0]) | int(t[0, 1]) << 8 | int(t[8, 0]) << 16 | int(t[8, 1]) << 24
    assert int(pl[0, 1, 3]) & 0xFFFF == int(t[0, 1]) | int(t[0, 0]) << 8          # x = -2: reflected to 1, its neighbour -1 to 0


def test_drift_is_what_it_says():
    """Frame k + 1 is frame k moved by the kind's (dx, dy); the codes span the element type's range; P010 carries low bits."""
    H, W, S = 132, 200, 208
    for hdr in (0, 1):
        for kind in DRIFT_KINDS:
            dx = DRIFT_STEP[0] * (1 if kind[-1] == "e" else -1)
            dy = DRIFT_STEP[1] * (1 if kind[-2] == "s" else -1)
            a = [x.reshape(-1, S) for x in frames(kind, H, W, bool(hdr), 5, 3, S, 5)]
            assert all(x.dtype == (np.uint16 if hdr else np.uint8) and (x[:, W:] == 0).all() for x in a)
            for k in (0, 1):
                y0, y1 = a[k][:H, :W], a[k + 1][:H, :W]
                ys, xs = slice(max(dy, 0), H + min(dy, 0)), slice(max(dx, 0), W + min(dx, 0))
                yd, xd = slice(max(-dy, 0), H + min(-dy, 0)), slice(max(-dx, 0), W + min(-dx, 0))
                assert (y0[ys, xs] == y1[yd, xd]).all(), (kind, k)
            span = int(a[0][:H, :W].max()) - int(a[0][:H, :W].min())
            assert span >= (65536 if hdr else 256) // 2, (kind, span)                 # (the whole field spans every code: this window of it half)
            if hdr:
                assert len(np.unique(a[0][:H, :W] & 0xFF)) > 200
    assert (frames("drift-se", H, W, False, 5, 2)[0] != frames("drift-se", H, W, False, 6, 2)[0]).any()


if __name__ == "__main__":
    for key in GEOMETRIES:
        rs, lw, lh = M.DEEP_GEOMETRIES[key]
        a = jobs()[key].result()
        print(f"  {lw:3d} x {lh} rs {rs} {'P010' if key[0] else 'SDR '} runs {a['runs']:3d}  oob {a['oob']}  x pairs {a['xpairs']}/{max(1, (1 << rs) // 2)}  "
              f"y phases {a['yphases']}/{1 << rs}  beyond L/R/T/B {'/'.join(str(e) for e in a['edges'])}  reach {a['reach']}", flush=True)
