"""The tie matrix of tests/test_chain_ties_gpu.py and the CPU analysis that proves its content bites (tests/test_chain_tie_model.py):
a walk of the oracle's chain that lists, per step, the windows whose first and last minimum differ ("tied winners") by tile class and by
whether the window reuses, and walks of the same chain with the tie rule mutated at one step class (window, axis) -- the last minimum wins,
or the lowest tied minimum with bit b of cz set, which is what a best_xor stage does when it keeps its partner on equality."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_variant_model as M  # noqa: E402
from chain_content import TIE_KINDS, TIE_SETTINGS, frames, kind_seed  # noqa: E402
from chain_saturation_model import reuse_windows  # noqa: E402
from flow_reuse_model import chain_steps  # noqa: E402
from oracle import oracle  # noqa: E402  (test infrastructure)

NO_LAZY, NO_GRAPH = "no-lazy-argmin", "no-graph"

_c = M._c
CASES = [
    # 480 x 256 grid, rs 0: every tile full
    _c("sdr256-n16-tab", 0, 256, 480, 270, 16, delta=0, nb=0),
    _c("sdr256-n5-notab", 0, 256, 480, 270, 5, tables=M.NEVER, delta=3, nb=2),
    _c("sdr256-n1-tab", 0, 256, 480, 270, 1),
    _c("sdr256-n3-notab", 0, 256, 480, 270, 3, tables=M.NEVER, delta=0, nb=0),
    _c("sdr256-n5-R11", 0, 256, 480, 270, 5, R=11, delta=0, nb=0),          # (level 8 of the 240 x 136 grid is the first with the neighbour term: no site there)
    _c("sdr256-n4-it3", 0, 256, 480, 270, 4, it=3, tables=M.NEVER, delta=0, nb=0),      # ends at 64: the last argmin is flushed by flow_big_argmin_kernel
    # 240 x 136 grid, rs 2: partial tiles right and bottom; the one-wave large-window kernel from four members on
    _c("sdr544-n4-tab", 0, 544, 960, 136, 4, delta=0, nb=0),
    _c("sdr544-n3-tab", 0, 544, 960, 136, 3, delta=3, nb=2),
    _c("sdr544-n5-notab", 0, 544, 960, 136, 5, tables=M.NEVER, delta=0, nb=0),
    _c("sdr544-n4-notab", 0, 544, 960, 136, 4, tables=M.NEVER, delta=3, nb=2),
    _c("sdr544-n1-notab", 0, 544, 960, 136, 1, tables=M.NEVER, delta=0, nb=0),
    _c("sdr544-n3-R5", 0, 544, 960, 136, 3, R=5, tables=M.NEVER, delta=0, nb=0),
    _c("sdr544-n4-R11", 0, 544, 960, 136, 4, R=11, delta=3, nb=2),
    # the same grid at rs 3 from P010
    _c("hdr1088-n5-tab", 1, 1088, 1920, 136, 5, delta=0, nb=0),
    _c("hdr1088-n4-notab", 1, 1088, 1920, 136, 4, tables=M.NEVER, delta=10, nb=10),
    _c("hdr1088-n3-notab", 1, 1088, 1920, 136, 3, tables=M.NEVER, delta=3, nb=2),
    # 480 x 270 grid, rs 1, P010
    _c("hdr540-n4-tab", 1, 540, 960, 270, 4, delta=3, nb=2),
    _c("hdr540-n5-notab", 1, 540, 960, 270, 5, tables=M.NEVER, delta=0, nb=0),
    _c("hdr540-n3-tab", 1, 540, 960, 270, 3, delta=0, nb=0),
    _c("hdr540-n1-notab", 1, 540, 960, 270, 1, tables=M.NEVER),
    # chains that start at 32 (64 x 64 grid) and at 16 (32 x 32 grid)
    _c("sdr128-n5-tab", 0, 128, 128, 64, 5, delta=0, nb=0),
    _c("sdr128-n3-notab", 0, 128, 128, 64, 3, tables=M.NEVER, delta=3, nb=2),
    _c("hdr64-n4-tab", 1, 64, 64, 32, 4, delta=0, nb=0),
    _c("hdr64-n3-notab", 1, 64, 64, 32, 3, tables=M.NEVER, delta=0, nb=0),
    # 1388 x 568 grid: large windows at neighbour-term levels, their argmin taken by flow_big_argmin_kernel
    _c("sdr568x1388-n4-tab", 0, 568, 1388, 1000, 4, delta=0, nb=0),
    _c("sdr568x1388-n3-notab", 0, 568, 1388, 1000, 3, tables=M.NEVER),
    # 1080p, 480 x 270 at rs 2: the one-wave large-window kernel on a grid with two rows of 128-windows
    _c("sdr1080-n4-tab", 0, 1080, 1920, 270, 4, delta=0, nb=0),
]
FLAGS = {"sdr256-n5-notab": NO_LAZY, "sdr544-n1-notab": NO_GRAPH}
MUTATIONS = ("last", "bit 0", "bit 1", "bit 2", "bit 3")


def member_kinds(case):
    """Content of member i: the tie kinds in turn, starting where the case's place in CASES says (a lone context runs them one after the
    other)."""
    s = [c.name for c in CASES].index(case.name)
    return [TIE_KINDS[(s + i) % len(TIE_KINDS)] for i in range(case.n)]


def tie_frames(case, kind, count=4):
    """The frames test_chain_variants_gpu.case_frames hands the GPU test for this case and kind."""
    return frames(kind, case.H, case.W, bool(case.hdr), kind_seed(kind), count, case.in_stride, M.geometry(case).rs)


def walk_key(case):
    """Cases with the same key walk the same chains."""
    return (case.hdr, case.H, case.W, case.max_res, case.in_stride, case.R, case.delta, case.nb, case.iterations)


# ------------------------------------------------------------------------------------------------
# tile classes of windows
# ------------------------------------------------------------------------------------------------
def _tile_shape(ln):
    if ln.variant.startswith("big."):
        return 64, 4 * (1 if ".wave1." in ln.variant else 4), False
    tw = 16 if ln.variant.startswith("level2.row") else 32
    return tw, 32, tw == 16


def window_classes(case, ws):
    """[nwy, nwx] of tile-class names (chain_variant_model._tiles' notion) for the windows of level ws: "full" when every tile of the level's
    launch that holds a part of the window lies inside the grid, else "right" / "bottom" ("right" where both), "half" for the row-per-lane
    level 2's 16-wide tile inside a partial 32-wide one, "any" at R < 16."""
    g = M.geometry(case)
    ln = next(l for l in M.launches(case) if l.window == ws)
    tw, th, half = _tile_shape(ln)
    nwy, nwx = -(-g.lh // ws), -(-g.lw // ws)
    if case.R != 16:
        return np.full((nwy, nwx), "any", dtype=object)
    x1 = np.minimum(np.arange(nwx) * ws + ws, g.lw) - 1           # the window's last column and row inside the grid
    y1 = np.minimum(np.arange(nwy) * ws + ws, g.lh) - 1
    in_x, in_y = (x1 // tw + 1) * tw <= g.lw, (y1 // th + 1) * th <= g.lh
    row = np.where(in_x, "full", "right").astype(object)
    if half:
        row[in_x & (((x1 // tw * tw) | 31) >= g.lw)] = "half"
    out = np.repeat(row[None], nwy, axis=0)
    out[~in_y] = np.where(in_x, "bottom", "right").astype(object)
    return out


# ------------------------------------------------------------------------------------------------
# the walk
# ------------------------------------------------------------------------------------------------
def first_last(pick):
    """(first minimum, last minimum) per window of pick[R, nwy, nwx]."""
    R = pick.shape[0]
    return pick.argmin(axis=0), R - 1 - pick[::-1].argmin(axis=0)


def walk(case, kind, pair):
    """The oracle's chain on pair `pair` (1: frames 1 and 2, 2: frames 2 and 3) of `kind`: (steps, oob); a step is dict(k, axis, ws,
    before, after, pick[R, nwy, nwx] (the window sums), first, last)."""
    g = M.geometry(case)
    f = tie_frames(case, kind)
    steps, oob = [], 0
    for k, axis, ws, before, after, sums, o in chain_steps(f[pair], f[pair + 1], g, case.R, case.delta, case.nb, case.iterations, with_sums=True):
        pick = sums[:, ::ws, ::ws].copy()
        first, last = first_last(pick)
        steps.append(dict(k=k, axis=axis, ws=ws, before=before, after=after, pick=pick, first=first, last=last))
        oob += o
    return steps, oob


def tied_winners(case, kind, walks=None):
    """dict(oob = (pair 1, pair 2), steps = [dict(pair, ws, axis, tied = {tile class: windows}, reusing = tied windows in full tiles that
    reuse, pairs = {(first, last)})], pairs = all of them, final = the offsets after each pair).  walks: (walk(.., 1), walk(.., 2)) if at hand."""
    walks = walks or (walk(case, kind, 1), walk(case, kind, 2))
    out = dict(oob=tuple(w[1] for w in walks), steps=[], pairs=set(), final=[w[0][-1]["after"] for w in walks])
    for pair, (steps, _) in zip((1, 2), walks):
        for i, st in enumerate(steps):
            tied = st["first"] != st["last"]
            rec = dict(pair=pair, ws=st["ws"], axis=st["axis"], tied={}, reusing=0, pairs=set())
            if tied.any():
                cls = window_classes(case, st["ws"])
                for c in np.unique(cls[tied]):
                    rec["tied"][c] = int((tied & (cls == c)).sum())
                if case.R == 16:
                    rec["reusing"] = int((tied & (cls == "full") & reuse_windows(steps, i)).sum())
                rec["pairs"] = set(zip(st["first"][tied].tolist(), st["last"][tied].tolist()))
                out["pairs"] |= rec["pairs"]
            out["steps"].append(rec)
    return out


def mutated_pick(pick, mutation):
    """The winner per window under a mutated tie rule (module docstring)."""
    first, last = first_last(pick)
    if mutation == "last":
        return last
    b = int(mutation.split()[1])
    cz = np.arange(pick.shape[0])[:, None, None]
    ok = (pick == pick.min(axis=0)) & ((cz >> b) & 1 == 1)
    return np.where(ok.any(axis=0), ok.argmax(axis=0), first)


def mutated_final(case, kind, pair, steps, ws, axis, mutation):
    """The chain's final offsets with `mutation` as the tie rule of step (ws, axis) and the oracle's own everywhere else, or None where the
    mutated rule elects the oracle's winners at that step (steps: walk(case, kind, pair)[0])."""
    i = next((j for j, st in enumerate(steps) if (st["ws"], st["axis"]) == (ws, axis)), None)
    if i is None:
        return None
    win = mutated_pick(steps[i]["pick"], mutation)
    if (win == steps[i]["first"]).all():
        return None
    g = M.geometry(case)
    L = oracle.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    f = tie_frames(case, kind)
    off = steps[i]["before"].copy()
    lowest = np.zeros((g.lh, g.lw), dtype=np.uint8)
    lowest[::ws, ::ws] = win
    L.hfo_adjust_offsets(p(off), p(lowest), ws, case.R, g.lh, g.lw, axis)
    for st in steps[i + 1:]:
        sums, _ = oracle.calc_delta_sums(f[pair], f[pair + 1], off, g, st["ws"], case.R, st["k"], st["axis"], case.delta, case.nb)
        sums = np.ascontiguousarray(sums)
        L.hfo_determine_lowest_layer(p(sums), p(lowest), st["ws"], case.R, g.lh, g.lw)
        L.hfo_adjust_offsets(p(off), p(lowest), st["ws"], case.R, g.lh, g.lw, st["axis"])
    return off


def tied_variants(case, tw):
    """The labels of the case's launches that hold a tied winner of tw = tied_winners(case, kind): at R 16 in a full tile for a .plain
    label, in a reusing window of a full tile for a .tab label of windows 16 to 2 (level 32 never reuses: any full tile)."""
    out = set()
    for ln in M.launches(case):
        for rec in tw["steps"]:
            if rec["ws"] != ln.window:
                continue
            if ln.variant.endswith(".tab") and ln.window < 32:
                hit = rec["reusing"] > 0
            elif case.R == 16:
                hit = rec["tied"].get("full", 0) > 0
            else:
                hit = bool(rec["tied"])
            if hit:
                out.add(ln.variant)
    return out


if __name__ == "__main__":
    from concurrent.futures import ThreadPoolExecutor
    seen = {}
    for case in CASES:
        seen.setdefault(walk_key(case), case)
    with ThreadPoolExecutor(8) as pool:
        jobs = {(c.name, kind): pool.submit(tied_winners, c, kind) for c in seen.values() for kind in TIE_KINDS}
    for case in seen.values():
        g = M.geometry(case)
        for kind in TIE_KINDS:
            tw = jobs[(case.name, kind)].result()
            row = {}
            for rec in tw["steps"]:
                if rec["tied"]:
                    key = f"{rec['ws']}{'XY'[rec['axis']]}"
                    n, r = row.get(key, (0, 0))
                    row[key] = (n + sum(rec["tied"].values()), r + rec["reusing"])
            cells = "  ".join(f"{k} {n}" + (f" r{r}" if r else "") for k, (n, r) in row.items())
            mark = "*" if TIE_SETTINGS[kind] == (case.delta, case.nb) else " "
            print(f"{g.lw} x {g.lh} rs {g.rs} {'P010' if g.hdr else 'SDR '} R {case.R:2d} ({case.delta:2d}, {case.nb:2d}) {kind}{mark}: {cells}   "
                  f"pairs {sorted(tw['pairs'])} oob {tw['oob']}", flush=True)
