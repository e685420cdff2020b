"""CPU: the content of tests/test_chain_ties_gpu.py puts exact ties between a window's best candidates at every step class of the chain, in
the tiles and the reusing windows the kernel variants treat differently, and a tie rule other than the reference's -- the first minimum
wins, determineLowestLayerKernelSDR.h:19-24 -- changes the chain's result on it.  Proved on the oracle (tests/chain_tie_model.py).

How the ties come about (tests/chain_content.py tie_sites): frame N is flat, frame N - 1 is flat with two bars of luma marks at the first
and the last sample of one window along the searched axis, mirror images about the window's centre.  While the window's offset is 0,
d = 0 sees both bars, -d and +d each miss one and pay the same bias, so they tie exactly and the first, -d, wins; the amplitude decides at
which level a window leaves 0 (one bar's SAD << delta above d x window pixels x bias, and below the same figure of the parent, which
loses the bar at its own border).  Every ancestor keeps d = 0 on both axes -- the SAD tables' reuse condition -- so tied winners land in
reusing windows too.  The amplitudes depend on (delta, nb): one kind per setting, (0, 0), (3, 2) and (8, 6); every member of a case
runs every kind, and a kind made for another setting still ties here and there.  The first level with the neighbour term (the chain's
fifth) cannot be reached this way -- its bias is five times its parent's or more -- which is level 16 on the 480-wide grids, 8 on
240 x 136 and 64 on 1388 x 568; the other geometries reach each of them.

What is asserted, all of it on the oracle alone (conditions on the INPUT, not measurements of the product):
  * no sample beyond the single reflection, for every case, kind and pair;
  * every (window, axis) from 256 down to 2: some case and kind with two tied winners or more inside full tiles; for 128 and 64 in a case
    whose large-window argmins are taken lazily (and in one that has no other way) and in a case that takes some explicitly -- the
    1388-wide grid for 128, a chain of three levels that ends on 64 for 64.  UNREACHED is empty: level 256 is reached on the 1388-wide grid;
  * every chain variant of tests/chain_variant_model.py (level*.tab / .plain / .anyR, big.wave1 / wave4 .r16 / .anyR) has a case in which
    one of its launches holds a tied winner in a full tile -- for .tab of 16, 8, 4 and 2 in a window that reuses;
  * the tied pairs hold (7, 9), (6, 10) and more at R 16, and two or more at R < 16;
  * the last minimum in place of the first, at any single (window, axis) from 128 down to 2, changes the final offsets of some case, and
    so does a best_xor stage that keeps its partner on equality, for each of the four lane distances (bit 0 through the pair (8, 9));
  * the oracle's offsets on the two tie cases of tests/ref_live_cases.py are those the reference itself returned on an MI355X.

Measured (python tests/chain_tie_model.py, the rows of the kind made for the setting; tied winners per step class over both pairs, every
tile class; rN: those in reusing windows of full tiles; then the (first, last) candidates that tied):
  480 x 256 rs 0 SDR  R 16 ( 0,  0) tie-d0: 128X 2  64X 3  64Y 2  32X 4  32Y 4  8X 6 r2  8Y 2 r2  4X 4 r4  2X 4 r4 | (5, 11), (6, 10), (7, 9)
  480 x 256 rs 0 SDR  R 16 ( 3,  2) tie-d3: 128X 2  64X 3  64Y 2  32X 4  32Y 4  8X 4 r4  8Y 2 r2  4X 12 r12  4Y 4 r4  2X 8 r4 | (5, 11), (6, 10), (7, 9), (9, 11)
  480 x 256 rs 0 SDR  R 16 ( 8,  6) tie-d8: 128X 2  64X 3  64Y 2  32X 4  32Y 3  4X 3 r3  2X 4 r4 | (5, 11), (6, 10), (7, 9)
  480 x 256 rs 0 SDR  R 11 ( 0,  0) tie-d0: 128X 2  64X 3  64Y 2  32X 4  32Y 4  8X 6  8Y 2  4X 4  2X 4 | (2, 8), (3, 7), (4, 6)
  480 x 256 rs 0 SDR  R 16 ( 0,  0) tie-d0, three levels: 128X 2  64X 3  64Y 2 | (5, 11), (6, 10), (7, 9)
  240 x 136 rs 2 SDR  R 16 ( 0,  0) tie-d0: 64X 1  64Y 2  32X 1  32Y 4  16X 4 r4  16Y 5 r5  4X 8 r2  4Y 9 r2  2X 2 r2 | (6, 10), (7, 9)
  240 x 136 rs 2 SDR  R 16 ( 3,  2) tie-d3: 64X 1  64Y 3  32X 1  32Y 4  16X 6 r5  16Y 5 r5  4X 2  4Y 2  2X 2 r2 | (6, 10), (7, 9)
  240 x 136 rs 2 SDR  R  5 ( 0,  0) tie-d0: 64X 1  64Y 2  32X 1  32Y 4  16X 4  16Y 5  4X 8  4Y 9  2X 2 | (0, 4), (1, 3)
  240 x 136 rs 2 SDR  R 11 ( 3,  2) tie-d3: 64X 1  64Y 3  32X 1  32Y 4  16X 6  16Y 5  4X 2  4Y 2  2X 2 | (3, 7), (4, 6)
  240 x 136 rs 3 P010 R 16 ( 0,  0) tie-d0: 64X 1  64Y 4  32X 3  32Y 3  16X 2 r2  16Y 1 r1  4X 6  4Y 10 r4  2X 4 r4 | (7, 9)
  240 x 136 rs 3 P010 R 16 ( 3,  2) tie-d3: 128Y 1  64X 1  64Y 2  32X 3  32Y 3  16X 2 r2  16Y 6 r6  8Y 1  4X 4  4Y 3  2X 4 r4 | (7, 9), (8, 9)
  480 x 270 rs 1 P010 R 16 ( 3,  2) tie-d3: 128X 1  128Y 2  64X 1  64Y 6  32X 4  32Y 5  8Y 4  4X 4 r4  4Y 4 r4  2X 36 r36  2Y 32 r32 | (6, 10), (7, 9)
  480 x 270 rs 1 P010 R 16 ( 0,  0) tie-d0: 128X 1  128Y 2  64X 1  64Y 4  32X 4  32Y 6  8X 9 r1  8Y 11 r3  4X 4 r4  4Y 4 r4  2X 4 r4 | (6, 10), (7, 9)
  480 x 270 rs 1 P010 R 16 ( 8,  6) tie-d8: 256Y 2  128X 2  128Y 3  64X 3  64Y 1  32X 8  32Y 5  4X 2 r2  4Y 2 r2  2X 4 r4 | (6, 7), (6, 10), (7, 9)
  64 x 64 rs 1 SDR    R 16 ( 0,  0) tie-d0: 32Y 2  16X 2 r2  8Y 1 r1  4X 3 r3  4Y 1 r1  2Y 4 | (7, 9), (8, 9)
  64 x 64 rs 1 SDR    R 16 ( 3,  2) tie-d3: 32Y 2  16X 2 r2  16Y 1 r1  4X 2 r2 | (7, 9)
  32 x 32 rs 1 P010   R 16 ( 0,  0) tie-d0: 16Y 2  4X 1 r1  4Y 1 r1  2X 3 r3  2Y 1 | (7, 9)
  1388 x 568 rs 0 SDR R 16 ( 0,  0) tie-d0: 128X 4  128Y 4  16X 4 r4  16Y 4 r4  8X 6 r6  8Y 2 r2  4X 8 r4  2X 12 r4 | (5, 7), (5, 11), (6, 10), (7, 9), (9, 11)
  1388 x 568 rs 0 SDR R 16 ( 8,  6) tie-d8: 256X 2  256Y 3  128X 4  128Y 5  32X 1  32Y 1  16X 2 r2  16Y 2 r2  8X 6 r6  8Y 2 r2  4X 4 r4  2X 22 r6  2Y 21 r21 | (5, 11), (6, 8), (6, 10), (7, 9), (9, 10), (9, 11)
  480 x 270 rs 2 SDR  R 16 ( 0,  0) tie-d0: 128X 1  128Y 2  64X 1  64Y 2  32X 4  32Y 4  8X 9 r1  8Y 14 r6  4X 6 r6  4Y 6 r6  2X 2 r2 | (6, 10), (7, 9)
The setting (10, 10) has no kind of its own; at 240 x 136 P010 the three kinds as they are give
  tie-d0: 128X 3  128Y 2  4X 6  4Y 6  2X 4 r4      tie-d3: 128X 3  128Y 2  64X 1  8Y 2  4X 6  4Y 12 r4  2X 18 r18  2Y 62 r62
  tie-d8: 128X 2  128Y 3  64X 4  64Y 1             all of them (7, 9)
A change of the case list or of the content that drops these shows here."""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_tie_model as T  # noqa: E402
import chain_variant_model as M  # noqa: E402
from chain_content import KIND_ORDER, SAT_KINDS, DRIFT_KINDS, TIE_BASE, TIE_KINDS, TIE_SETTINGS, frames, kind_seed, tie_sites  # noqa: E402

LEVELS = (128, 64, 32, 16, 8, 4, 2)
FLOOR = 2                 # tied winners inside full tiles that one case and kind must show per (window, axis)
# (window, axis) the content does not reach -> why.  Nothing but (256, 0) and (256, 1) may stand here; both are reached.
UNREACHED = {}
_jobs = {}


def _size(case):
    g = M.geometry(case)
    return g.lw * g.lh


def jobs():
    """tied_winners of every distinct chain of the matrix and every kind, started together on first use (the oracle is plain C behind
    ctypes: the walks run side by side), the large grids first."""
    if not _jobs:
        pool = ThreadPoolExecutor(8)
        for c in sorted(T.CASES, key=_size, reverse=True):
            for kind in TIE_KINDS:
                if (T.walk_key(c), kind) not in _jobs:
                    _jobs[(T.walk_key(c), kind)] = pool.submit(T.tied_winners, c, kind)
        pool.shutdown(wait=False)
    return _jobs


def results():
    """[(case, kind, tied_winners)] for every case and every kind (every case runs every kind: test_every_kind_runs_in_every_case)."""
    return [(c, kind, jobs()[(T.walk_key(c), kind)].result()) for c in T.CASES for kind in TIE_KINDS]


def full_tied(tw, ws, axis):
    return sum(rec["tied"].get("full", 0) for rec in tw["steps"] if (rec["ws"], rec["axis"]) == (ws, axis))


def test_no_sample_beyond_the_reflection():
    for case, kind, tw in results():
        assert tw["oob"] == (0, 0), (case.name, kind, tw["oob"])


@pytest.mark.parametrize("axis", [0, 1], ids=["X", "Y"])
@pytest.mark.parametrize("ws", (256,) + LEVELS)
def test_every_step_class_has_tied_winners_in_full_tiles(ws, axis):
    best = {}
    for case, kind, tw in results():
        n = full_tied(tw, ws, axis)
        print(case.name, kind, ws, "XY"[axis], n)
        for label in M.argmin_labels(case) or {None}:
            best[label] = max(best.get(label, 0), n)
        best["all"] = max(best.get("all", 0), n)
    if (ws, axis) in UNREACHED:
        assert ws == 256
        return
    assert best["all"] >= FLOOR, (ws, "XY"[axis], best)
    if ws in (128, 64):          # both ways of taking a large window's argmin
        assert best.get("argmin.lazy", 0) >= FLOOR and best.get("argmin.explicit", 0) >= FLOOR, (ws, "XY"[axis], best)


def test_unreached_lists_level_256_alone():
    assert set(UNREACHED) <= {(256, 0), (256, 1)}
    # a case whose labels hold argmin.explicit alone does not exist; one that holds argmin.lazy alone reaches every large step class too
    lazy_only = [c for c in T.CASES if M.argmin_labels(c) == {"argmin.lazy"}]
    for ws in (128, 64):
        for axis in (0, 1):
            assert max(full_tied(jobs()[(T.walk_key(c), k)].result(), ws, axis) for c in lazy_only for k in TIE_KINDS) >= FLOOR, (ws, axis)


def test_every_chain_variant_holds_a_tied_winner():
    want = {v for v in M.ALL_VARIANTS if v.startswith("level") or v.startswith("big.")}
    got = {}
    for case, kind, tw in results():
        for v in T.tied_variants(case, tw):
            assert v in M.labels(case)
            assert not v.endswith(".anyR") or case.R < 16
            got.setdefault(v, []).append((case.name, kind))
    assert want <= set(got), sorted(want - set(got))


def test_the_pairs_that_tie():
    r16, low = set(), set()
    for case, kind, tw in results():
        (r16 if case.R == 16 else low).update(tw["pairs"])
    print(sorted(r16), sorted(low))
    assert {(7, 9), (6, 10)} <= r16 and len(r16) >= 3, sorted(r16)
    assert len(low) >= 2, sorted(low)
    assert all(a < b for a, b in r16 | low)


def _tied_at(ws, axis):
    """[(case, kind, pair)] whose chain has a tied winner at step (ws, axis), the small grids first, one per distinct chain."""
    out, seen = [], set()
    for case, kind, tw in sorted(results(), key=lambda r: _size(r[0])):
        for rec in tw["steps"]:
            if (rec["ws"], rec["axis"]) == (ws, axis) and rec["tied"] and (T.walk_key(case), kind, rec["pair"]) not in seen:
                seen.add((T.walk_key(case), kind, rec["pair"]))
                out.append((case, kind, rec["pair"]))
    return out


_walks = {}


def _changes(case, kind, pair, ws, axis, mutation):
    k = (T.walk_key(case), kind, pair)
    if k not in _walks:
        _walks.clear()          # (one chain's steps at a time)
        _walks[k] = T.walk(case, kind, pair)[0]
    steps = _walks[k]
    off = T.mutated_final(case, kind, pair, steps, ws, axis, mutation)
    return off is not None and bool((off != steps[-1]["after"]).any())


@pytest.mark.parametrize("axis", [0, 1], ids=["X", "Y"])
@pytest.mark.parametrize("ws", LEVELS)
def test_the_last_minimum_changes_the_result(ws, axis):
    """`last` at this step class alone, the oracle's rule at every other step: the final offsets of some case differ."""
    tried = _tied_at(ws, axis)[:4]
    assert tried and any(_changes(c, kind, pair, ws, axis, "last") for c, kind, pair in tried), (ws, "XY"[axis], [(c.name, k, p) for c, k, p in tried])


@pytest.mark.parametrize("b", [0, 1, 2, 3])
def test_a_stage_that_keeps_its_partner_changes_the_result(b):
    """`bit b` (a best_xor stage of lane distance 2^b that keeps its partner on equality): the final offsets of some case differ.
    It needs a tied pair whose first member has bit b clear and whose last has it set: (7, 9) for bit 3, (5, 11) for bit 1, (3, 7) at
    R 11 for bit 2, (8, 9) for bit 0."""
    mutation = f"bit {b}"
    for case, kind, tw in sorted(results(), key=lambda r: _size(r[0])):
        for rec in tw["steps"]:
            if any(not (lo >> b) & 1 and (hi >> b) & 1 for lo, hi in rec["pairs"]):
                if _changes(case, kind, rec["pair"], rec["ws"], rec["axis"], mutation):
                    return
    pytest.fail(f"no case changes under {mutation}")


def test_mutated_rules():
    s = np.array([5, 3, 9, 3, 7, 3, 3, 8, 3], dtype=np.uint32).reshape(9, 1, 1)        # minima at 1, 3, 5, 6, 8
    assert [int(a[0, 0]) for a in T.first_last(s)] == [1, 8]
    assert [int(T.mutated_pick(s, m)[0, 0]) for m in T.MUTATIONS] == [8, 1, 3, 5, 8]
    s[1] = 4                                                                           # minima at 3, 5, 6, 8
    assert [int(T.mutated_pick(s, m)[0, 0]) for m in T.MUTATIONS] == [8, 3, 3, 5, 8]
    one = np.array([5, 3, 9], dtype=np.uint32).reshape(3, 1, 1)
    assert all(int(T.mutated_pick(one, m)[0, 0]) == 1 for m in T.MUTATIONS)             # no tie: every rule elects the minimum
    none = np.array([3, 9, 9, 9, 3], dtype=np.uint32).reshape(5, 1, 1)                  # minima at 0 and 4: no tied candidate has bit 0 or 1
    assert [int(T.mutated_pick(none, m)[0, 0]) for m in T.MUTATIONS] == [4, 0, 0, 4, 0]


def test_a_mutation_away_from_the_ties_changes_nothing():
    """mutated_final is the oracle's chain: where the mutated rule elects the same winners it says so, and a walk from a step's own
    winners arrives at the oracle's offsets."""
    case = next(c for c in T.CASES if c.name == "sdr544-n4-tab")
    steps, _ = T.walk(case, "tie-d0", 2)
    i = next(j for j, st in enumerate(steps) if (st["first"] != st["last"]).any())
    j = next(j for j, st in enumerate(steps) if (st["first"] == st["last"]).all())
    assert T.mutated_final(case, "tie-d0", 2, steps, steps[j]["ws"], steps[j]["axis"], "last") is None
    st = steps[i]
    only = np.where(np.arange(case.R)[:, None, None] == st["first"][None], 0, 1).astype(np.uint32)      # sums whose one minimum is the oracle's winner
    forced = steps[:i] + [dict(st, pick=only, first=np.full_like(st["first"], -1))] + steps[i + 1:]      # (.. taken as a change: the walk runs)
    off = T.mutated_final(case, "tie-d0", 2, forced, st["ws"], st["axis"], "last")
    assert off is not None and (off == steps[-1]["after"]).all()
    assert _changes(case, "tie-d0", 2, st["ws"], st["axis"], "last")
    from oracle import oracle
    f = T.tie_frames(case, "tie-d0")
    assert (oracle.calculate_optical_flow(f[2], f[3], M.geometry(case), case.R, 0, case.delta, case.nb, 0)[0] == steps[-1]["after"]).all()


def test_the_oracle_reads_ties_as_the_live_reference_does():
    """The two tie cases of tests/ref_live_cases.py: the reference itself ran them on an MI355X (tests/golden/ref_live.json), and the
    oracle's offsets of both pairs are its offsets bit for bit -- on pairs with tied winners at eight step classes or more, where the last
    minimum in place of the first at any one of them would have given other offsets."""
    import ref_live_cases as RC
    from oracle import oracle
    cases = [p for p in RC.HIP_CASES if isinstance(p[8], str)]
    assert [(p[0], p[8]) for p in cases] == [(0, "tie-d0"), (1, "tie-d3")]
    for hdr, H, W, si, so, R, delta, nb, kind, max_res in cases:
        assert TIE_SETTINGS[kind] == (delta, nb)
        rc = RC.hip_case(hdr, H, W, si, so, R, delta, nb, kind, max_res)
        ref = RC.Recorded(rc)
        case = M._c("ref", hdr, H, W, max_res, 1, R=R, delta=delta, nb=nb, stride=si)
        f = rc["frames"]
        assert all((a == b).all() for a, b in zip(f, T.tie_frames(case, kind)))
        walks = (T.walk(case, kind, 1), T.walk(case, kind, 2))
        tw = T.tied_winners(case, kind, walks)
        assert tw["oob"] == (0, 0)
        for name, (steps, _) in zip(("off", "off2"), walks):
            assert ref.same(name, steps[-1]["after"]), (kind, name)
        tied = {(rec["pair"], rec["ws"], rec["axis"]) for rec in tw["steps"] if rec["tied"]}
        assert len({t[1:] for t in tied}) >= 8, sorted(tied)
        changed = 0
        for pair, ws, axis in sorted(tied):
            off = T.mutated_final(case, kind, pair, walks[pair - 1][0], ws, axis, "last")
            changed += off is not None and not ref.same("off" if pair == 1 else "off2", off)
        assert changed >= 8, (kind, changed, len(tied))


# ------------------------------------------------------------------------------------------------
# the content
# ------------------------------------------------------------------------------------------------
def test_existing_kinds_keep_their_seeds():
    assert KIND_ORDER[-len(TIE_KINDS):] == TIE_KINDS and set(TIE_SETTINGS) == set(TIE_KINDS)
    assert [kind_seed(k) for k in ("patches", "pan64", SAT_KINDS[0], DRIFT_KINDS[-1])] == [9000, 9078, 9091, 9182]


@pytest.mark.parametrize("hdr", [0, 1])
def test_tie_frames_are_what_they_say(hdr):
    """Flat luma and chroma, the marks of a site mirror images about its window's centre, even and odd frames marked in different
    windows, the pitch honoured."""
    H, W, S_, rs = 272, 480, 496, 1
    s = 1 << rs
    for kind in TIE_KINDS:
        a = frames(kind, H, W, bool(hdr), kind_seed(kind), 4, S_, rs)
        assert len(a) == 4 and all(x.dtype == (np.uint16 if hdr else np.uint8) and x.size == (H + H // 2) * S_ for x in a)
        assert (a[0] == a[2]).all() and (a[1] == a[3]).all() and (a[0] != a[1]).any()
        sites = tie_sites(kind, H, W, rs, kind_seed(kind))
        assert {st["set"] for st in sites} == {0, 1} and {st["axis"] for st in sites} == {0, 1} and len({st["ws"] for st in sites}) >= 4
        top = [(x.reshape(-1, S_)[:, :W] >> (8 if hdr else 0)).astype(int) for x in a[:2]]
        for i, t in enumerate(top):
            assert (a[i].reshape(-1, S_)[:, W:] == 0).all()
            assert (t[H:] == 128).all() and t[:H].min() == TIE_BASE and t[:H].max() > TIE_BASE
            if hdr:
                low = a[i].reshape(-1, S_)[:H, :W] & 0xFF
                assert ((low == 0xFF) == (t[:H] == TIE_BASE)).all() and set(np.unique(low)) == {0, 0xFF}
        for st in sites:
            y = top[st["set"]][:H]
            other = top[1 - st["set"]][:H]
            x0, y0, ws = st["wx"] * s, st["wy"] * s, st["ws"]
            span = (ws - 1) * s + 1
            win = y[y0:y0 + span, x0:x0 + span]
            assert (win == (win[:, ::-1] if st["axis"] == 0 else win[::-1])).all(), st       # mirror images along the searched axis
            assert win.max() == TIE_BASE + st["a"] and (other[y0:y0 + span, x0:x0 + span] == TIE_BASE).all(), st
            if st["thin"]:
                lines = win if st["axis"] == 0 else win.T
                assert (lines[:, 1:-1] == TIE_BASE).all() and lines[:, 0].max() > TIE_BASE, st       # on the first and last sample line alone


# ------------------------------------------------------------------------------------------------
# the matrix
# ------------------------------------------------------------------------------------------------
def test_matrix_holds_what_the_issue_lists():
    cs = T.CASES
    names = [c.name for c in cs]
    assert len(set(names)) == len(names) and set(T.FLAGS) <= set(names)
    grids = {}
    for c in cs:
        g = M.geometry(c)
        grids.setdefault((c.hdr, c.H, c.W, c.max_res), (g.rs, g.lw, g.lh))
    assert grids == {(0, 256, 480, 270): (0, 480, 256), (0, 544, 960, 136): (2, 240, 136), (1, 1088, 1920, 136): (3, 240, 136),
                     (1, 540, 960, 270): (1, 480, 270), (0, 128, 128, 64): (1, 64, 64), (1, 64, 64, 32): (1, 32, 32),
                     (0, 568, 1388, 1000): (0, 1388, 568), (0, 1080, 1920, 270): (2, 480, 270)}
    big = [c for c in cs if c.H == 1080]
    assert len(big) == 1 and big[0].n >= 4 and "big.wave1.r16" in M.labels(big[0])
    assert {c.n for c in cs} == {1, 3, 4, 5, 16} and sum(c.n == 16 for c in cs) == 1
    assert {c.tables for c in cs} == {M.ALWAYS, M.NEVER}          # never the timing-dependent default
    assert {c.R for c in cs} == {16, 11, 5}
    assert {(c.delta, c.nb) for c in cs} == {(0, 0), (3, 2), (8, 6), (10, 10)}
    assert set(TIE_SETTINGS.values()) <= {(c.delta, c.nb) for c in cs}
    assert sorted(T.FLAGS.values()) == sorted([T.NO_LAZY, T.NO_GRAPH])
    lazy_case = next(c for c in cs if T.FLAGS.get(c.name) == T.NO_LAZY)
    assert lazy_case.n > 1 and M.windows(lazy_case)[0] > 32                       # a batch with large windows: the flag changes its launches
    assert next(c for c in cs if T.FLAGS.get(c.name) == T.NO_GRAPH).n == 1         # (the flag does not count inside a batch)
    seen = set().union(*(M.labels(c) for c in cs))
    assert {v for v in M.ALL_VARIANTS if v.startswith("level") or v.startswith("big.") or v.startswith("argmin.")} <= seen


def test_every_kind_runs_in_every_case():
    for c in T.CASES:
        kinds = T.member_kinds(c)
        assert len(kinds) == c.n and set(kinds) <= set(TIE_KINDS)
        assert c.n == 1 or set(kinds) == set(TIE_KINDS), c.name          # (a lone context runs the kinds one after the other)
