"""The saturation matrix of tests/test_chain_saturation_gpu.py and the CPU analysis that proves its content bites
(tests/test_chain_saturation_model.py): a walk of the oracle's chain that splits every step's window sums into the SAD part and the bias
part through the oracle's public calls alone, and counts the windows whose winner depends on the high bits of the SAD part."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_variant_model as M  # noqa: E402
from chain_content import SAT_KINDS, frames, kind_seed  # noqa: E402
from flow_reuse_model import chain_steps  # noqa: E402
from oracle import oracle  # noqa: E402  (test infrastructure)

NO_LAZY, NO_GRAPH = "no-lazy-argmin", "no-graph"

_c = M._c
CASES = [
    # 480 x 256 grid, rs 0: every tile full
    _c("sdr256-n16-tab", 0, 256, 480, 270, 16, delta=0, nb=0),
    _c("sdr256-n5-notab", 0, 256, 480, 270, 5, tables=M.NEVER),
    _c("sdr256-n1-tab", 0, 256, 480, 270, 1, delta=10, nb=10),
    _c("sdr256-n3-notab", 0, 256, 480, 270, 3, tables=M.NEVER, delta=0, nb=0),
    # 240 x 136 grid, rs 2: partial tiles right and bottom, the half tile of the row-per-lane level 2
    _c("sdr544-n4-tab", 0, 544, 960, 136, 4, delta=0, nb=0),
    _c("sdr544-n3-tab", 0, 544, 960, 136, 3),
    _c("sdr544-n5-notab", 0, 544, 960, 136, 5, tables=M.NEVER, delta=10, nb=10),
    _c("sdr544-n4-notab", 0, 544, 960, 136, 4, tables=M.NEVER),
    _c("sdr544-n1-notab", 0, 544, 960, 136, 1, tables=M.NEVER, delta=0, nb=0),
    _c("sdr544-n5-R11", 0, 544, 960, 136, 5, R=11),
    _c("sdr544-n3-R5", 0, 544, 960, 136, 3, R=5, tables=M.NEVER, delta=0, nb=0),
    # the same grid at rs 3 from P010
    _c("hdr1088-n5-tab", 1, 1088, 1920, 136, 5),
    _c("hdr1088-n4-notab", 1, 1088, 1920, 136, 4, tables=M.NEVER, delta=10, nb=10),
    _c("hdr1088-n3-notab", 1, 1088, 1920, 136, 3, tables=M.NEVER, delta=0, nb=0),
    _c("hdr1088-n4-tab", 1, 1088, 1920, 136, 4, delta=0, nb=0),
    # 480 x 270 grid, rs 1, P010
    _c("hdr540-n4-tab", 1, 540, 960, 270, 4),
    _c("hdr540-n5-notab", 1, 540, 960, 270, 5, tables=M.NEVER, delta=10, nb=10),
    _c("hdr540-n3-tab", 1, 540, 960, 270, 3, delta=0, nb=0),
    _c("hdr540-n1-notab", 1, 540, 960, 270, 1, tables=M.NEVER),
    # chains that start at 32 (64 x 64 grid) and at 16 (32 x 32 grid)
    _c("sdr128-n5-tab", 0, 128, 128, 64, 5, delta=0, nb=0),
    _c("sdr128-n3-notab", 0, 128, 128, 64, 3, tables=M.NEVER, delta=10, nb=10),
    _c("hdr64-n4-tab", 1, 64, 64, 32, 4, delta=0, nb=0),
    _c("hdr64-n3-notab", 1, 64, 64, 32, 3, tables=M.NEVER),
    # 1388 x 568 grid: large windows at neighbour-term levels
    _c("sdr568x1388-n4-tab", 0, 568, 1388, 1000, 4, delta=0, nb=0),      # (1388 = 86.75 x 16: the row-per-lane level 2's tile across the right edge)
    _c("sdr568x1388-n3-notab", 0, 568, 1388, 1000, 3, tables=M.NEVER),
    # 1080p, 480 x 270 at rs 2: the one-wave large-window kernel's tiles across the bottom edge (270 = 67.5 x 4; no small shape has them)
    _c("sdr1080-n4-tab", 0, 1080, 1920, 270, 4, delta=0, nb=0),
]
FLAGS = {"sdr256-n5-notab": NO_LAZY, "sdr544-n1-notab": NO_GRAPH}

# what the cases together must reach: every small-level variant as .tab and as .plain and both large-window kernels at R 16, in every tile
# class the model lists for them; the masked bodies and both ways of taking a large window's argmin at least once
REQUIRED_PAIRS = {p for p in M.required_pairs() if not p[0].endswith(".anyR")}
REQUIRED_LABELS = {v for v in M.ALL_VARIANTS if v.endswith(".anyR")} | {"argmin.lazy", "argmin.explicit"}


def member_kinds(case):
    """Content of member i: the four kinds in turn.  A case of fewer than four members starts where its place in CASES says, so that
    every kind runs at every batch size; "specks" is in every case (a lone context runs the four kinds one after the other)."""
    if case.n >= len(SAT_KINDS):
        return [SAT_KINDS[i % len(SAT_KINDS)] for i in range(case.n)]
    rest = SAT_KINDS[1:]
    s = [c.name for c in CASES].index(case.name)
    return ["specks"] + [rest[(s + i) % len(rest)] for i in range(case.n - 1)]


def geom_key(case):
    return (case.hdr, case.H, case.W, case.max_res, case.in_stride)


def sat_frames(case, kind, count=4):
    """The frames test_chain_variants_gpu.case_frames hands the GPU test for this case and kind."""
    return frames(kind, case.H, case.W, bool(case.hdr), kind_seed(kind), count, case.in_stride, M.geometry(case).rs)


# ------------------------------------------------------------------------------------------------
# the walk
# ------------------------------------------------------------------------------------------------
MUTATIONS = {
    "mod 2^16": lambda s: s & 0xFFFF,
    "mod 2^15": lambda s: s & 0x7FFF,
    "clamp 65535": lambda s: np.minimum(s, 65535),
    "signed 16": lambda s: (((s & 0xFFFF) ^ 0x8000) - 0x8000) & 0xFFFFFFFF,
}


def split_steps(f1, f2, g, R=16, delta=8, nb=6, min_window=0, max_window=1 << 30):
    """For every step of the oracle's chain on (f1, f2) with window in [min_window, max_window]:
    dict(k, axis, ws, sad[R, nwy, nwx], bias[R, nwy, nwx], sums[R, nwy, nwx] (uint64, a row per candidate, one entry per window),
    full[nwy, nwx] (the window lies inside the grid), before, after), and the oracle's out-of-bounds sample count over the whole chain.
    SAD and bias come from the oracle's public calls: calc_delta_sums of two all-zero frames at the same offsets is the bias part, the
    delta-0 sums of the real pair minus it the SAD part; ((sad << delta) + bias) mod 2^32 must be the oracle's sums."""
    zero = np.zeros_like(f1)
    out, oob = [], 0
    for k, axis, ws, before, after, sums, o in chain_steps(f1, f2, g, R, delta, nb, with_sums=True):
        oob += o
        if not (min_window <= ws <= max_window):
            out.append(dict(k=k, axis=axis, ws=ws, before=before, after=after))
            continue
        bias = oracle.calc_delta_sums(zero, zero, before, g, ws, R, k, axis, delta, nb)[0]
        pick = lambda a: a[:, ::ws, ::ws].astype(np.uint64)
        s0 = sums if delta == 0 else oracle.calc_delta_sums(f1, f2, before, g, ws, R, k, axis, 0, nb)[0]
        sums_w, bias_w = pick(sums), pick(bias)
        sad_w = (pick(s0) - bias_w) & 0xFFFFFFFF
        assert ((((sad_w << delta) + bias_w) & 0xFFFFFFFF) == sums_w).all(), (k, axis, ws)
        wy, wx = np.meshgrid(np.arange(0, g.lh, ws), np.arange(0, g.lw, ws), indexing="ij")
        full = (wy + ws <= g.lh) & (wx + ws <= g.lw)
        assert (sad_w <= 765 * ws * ws).all(), (k, axis, ws, int(sad_w.max()))      # (the subtraction did not wrap: the split is a SAD)
        out.append(dict(k=k, axis=axis, ws=ws, sad=sad_w, bias=bias_w, sums=sums_w, full=full, before=before, after=after))
    return out, oob


def reuse_windows(steps, i):
    """[nwy, nwx] booleans: the windows of step i that may reuse, by the rule of flow_reuse_model.reuse_shares (R 16: the parent chose d = 0 at
    both steps of the level before -- Y step: at its Y step, and the window itself at this level's X step -- inside 32 x 32 tiles that lie
    in the grid; the first level of a chain and level 32 never reuse)."""
    st = steps[i]
    k, axis, ws = st["k"], st["axis"], st["ws"]
    lh, lw = st["before"].shape[1:]
    none = np.zeros(((lh + ws - 1) // ws, (lw + ws - 1) // ws), dtype=bool)
    if ws >= 32 or k == 0:
        return none
    same = lambda s: (s["before"][s["axis"]] == s["after"][s["axis"]])
    px, py = [s for s in steps if s["k"] == k - 1]
    ok = same(px) & same(py) if axis == 0 else same(py) & same(steps[i - 1])
    ok[(lh // 32) * 32:, :] = False
    ok[:, (lw // 32) * 32:] = False
    return ok[::ws, ::ws]


def sensitivity(steps, delta):
    """{(ws, axis): dict(windows, reusing, changed={mutation: (all windows, reusing windows)}, any_reusing, can_reuse)} for the steps of windows 32, 16, 8:
    how many windows' first-minimum argmin changes when the SAD part of every candidate is mutated before the shift and the bias."""
    out = {}
    for i, st in enumerate(steps):
        if st["ws"] not in (32, 16, 8) or "sad" not in st:
            continue
        win = st["sums"].argmin(axis=0)
        assert (np.take_along_axis(st["sums"], win[None], 0)[0] == st["sums"].min(axis=0)).all()
        reuse = reuse_windows(steps, i)
        changed, any_reusing = {}, np.zeros_like(reuse)
        for name, mut in MUTATIONS.items():
            cost = ((mut(st["sad"]) << delta) + st["bias"]) & 0xFFFFFFFF
            diff = cost.argmin(axis=0) != win
            changed[name] = (int(diff.sum()), int((diff & reuse).sum()))
            any_reusing |= diff & reuse
        out[(st["ws"], st["axis"])] = dict(windows=int(win.size), reusing=int(reuse.sum()), changed=changed, any_reusing=int(any_reusing.sum()),
                                           can_reuse=st["ws"] < 32 and st["k"] > 0)       # (reuse_windows' rule: level 32 and a chain's first level never reuse)
    return out


# ------------------------------------------------------------------------------------------------
# per geometry: what tests/test_chain_saturation_model.py asserts and its docstring records
# ------------------------------------------------------------------------------------------------
FLOORS = {32: ("mod 2^16", 4), 16: ("mod 2^16", 2), 8: ("mod 2^15", 2)}     # level: (mutation, 1 / share of all windows that must change)
REUSING_FLOOR = 5                # levels 16 and 8, per axis: reusing windows that change under at least one mutation
FLOOR_SETTING = (0, 0)           # the (delta, nb) at which the maxima and the reusing floors are asserted: a case with tables runs it at every geometry


def geometries():
    """{geometry key: its cases}, in the order of CASES."""
    out = {}
    for c in CASES:
        out.setdefault(geom_key(c), []).append(c)
    return out


def configs(cases):
    """The (delta, nb) the geometry's cases run at R 16 -> whether a case with tables runs it."""
    out = {}
    for c in cases:
        if c.R == 16:
            out[(c.delta, c.nb)] = out.get((c.delta, c.nb), False) or bool(M.tables_on(c))
    return out


def analyse_specks(case, delta, nb):
    """The second pair of "specks" (frame N - 1 speckled, frame N bright) at the case's geometry: dict(oob of both pairs, max = {window: the
    largest SAD of a full window}, sens = sensitivity())."""
    g = M.geometry(case)
    f = sat_frames(case, "specks")
    steps, oob2 = split_steps(f[2], f[3], g, 16, delta, nb, max_window=32)
    oob1 = sum(st[6] for st in chain_steps(f[1], f[2], g, 16, delta, nb, with_sums=True))
    mx = {}
    for st in steps:
        if "sad" in st and st["full"].any():
            mx[st["ws"]] = max(mx.get(st["ws"], 0), int(st["sad"][:, st["full"]].max()))
    return dict(oob=(oob1, oob2), max=mx, sens=sensitivity(steps, delta))


def analyse_uniform(case, kind, delta, nb):
    """A pair of "saturated", "sat-y" or "sat-uv": (oob, every offset zero, {window: the set of SAD / pixels inside the grid over every
    window of the level, partial ones too, and every candidate; -1 where the SAD is no multiple of the pixels})."""
    g = M.geometry(case)
    f = sat_frames(case, kind)
    steps, oob = split_steps(f[2], f[3], g, 16, delta, nb)
    per_pixel = {}
    for st in steps:
        ws = st["ws"]
        ny, nx = st["full"].shape
        npix = np.outer(np.minimum(ws, g.lh - ws * np.arange(ny)), np.minimum(ws, g.lw - ws * np.arange(nx))).astype(np.uint64)
        q = np.where(st["sad"] % npix == 0, st["sad"] // npix, np.uint64(2**63)).astype(np.int64)
        per_pixel.setdefault(ws, set()).update(np.unique(q).tolist())
    return oob, not any(st["after"].any() for st in steps), per_pixel


if __name__ == "__main__":
    for key, cases in geometries().items():
        g = M.geometry(cases[0])
        for (delta, nb), tab in configs(cases).items():
            a = analyse_specks(cases[0], delta, nb)
            row = []
            for (ws, ax), v in a["sens"].items():
                row.append(f"{ws}{'XY'[ax]} {v['changed'][FLOORS[ws][0]][0]}/{v['windows']}" + (f" r{v['any_reusing']}/{v['reusing']}" if v["can_reuse"] else ""))
            reached = [w for w, m in a["max"].items() if m == 765 * w * w]
            print(f"{g.lw} x {g.lh} rs {g.rs} {'P010' if g.hdr else 'SDR '} ({delta:2d}, {nb:2d}){' tab' if tab else '    '}: " + "  ".join(row) + f"   max {reached} oob {a['oob']}", flush=True)
