"""GPU: every instantiation of the chain and blur kernels that the BATCH SIZE, the resolution scalar, the search radius and the table mode
select (tests/chain_variant_model.py; csrc/hf_flow.hip launch_flow_level_small / launch_flow_big_partial, csrc/hf_kernels.hip
launch_blur_flow) against the CPU oracle.  The model's CASES is the matrix; tests/test_chain_variant_model.py proves on the CPU that it
reaches every variant and every (variant, tile class) pair.

Each case: n asynchronous members of one geometry in a FlowBatch, fed DIFFERENT content (noise patches in a static frame, the bench scene,
chaotic, static, a 64 px pan, hard cuts, full-range noise -- for P010 with the low bits set), the batched chain on two consecutive pairs
(both ring and blur phases) and once more on the second (the cached graph's replay), every member compared with the oracle of its own pair.
The table mode is pinned by flag in all but a few cases (the default decides from a timing-dependent report: parity only there).  With
tables at R = 16 the leader's debug counters prove which body ran: per small level exactly the windows of the tiles the model sends to
the table body, all members counted, edge tiles left out.
Bar: bit-exact offsets, blurred flow and total frame delta -- integer arithmetic (calcDeltaSumsKernelSDR.h:61-190,
determineLowestLayerKernelSDR.h:16-26, adjustOffsetArrayKernelSDR.h:11-19, blurFlowKernelSDR.h:17-92, opticalFlowCalcSDR.cpp:68-116).
The oracle's chain and its blur (hf_oracle.c hfo_calculate_optical_flow = the chain, then hfo_blur_flow on its offsets) are cached
separately per distinct pair, so cases that differ only in the blur radius or the batch size share the chain."""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_variant_model as M  # noqa: E402
from chain_content import frames, kind_seed  # noqa: E402

pytestmark = pytest.mark.gpu

KINDS = ["patches", "chaotic", "noise", "static", "bench", "cut", "pan64"]
_frame_cache, _chain_cache, _blur_cache = {}, {}, {}
_pool = ThreadPoolExecutor(8)     # (the oracle is plain C behind ctypes: the calls of a case's distinct pairs run side by side)


def member_kinds(n):
    """Content of member i.  Up to 13 members cycle all seven kinds; 16 and 32 cycle five (the oracle runs once per distinct pair, every member
    is compared)."""
    d = min(n, 7) if n <= 13 else 5
    return [KINDS[i % d] for i in range(n)]


def _geom_key(case):
    return (case.hdr, case.H, case.W, case.max_res, case.in_stride)


def case_frames(case, kind):
    """Four consecutive frames of `kind` at the case's geometry (kept for the cases of one geometry: they follow each other in CASES)."""
    gk = _geom_key(case)
    if _frame_cache.get("geometry") != gk:
        _frame_cache.clear()
        _frame_cache["geometry"] = gk
    if kind not in _frame_cache:
        _frame_cache[kind] = frames(kind, case.H, case.W, bool(case.hdr), kind_seed(kind), 4, case.in_stride, M.geometry(case).rs)
    return _frame_cache[kind]


def _oracle_chain(case, g, f1, f2, key):
    from oracle import oracle
    k = _geom_key(case) + key + (case.R, case.iterations, case.delta, case.nb)
    if k not in _chain_cache:
        off, _, tot, _ = oracle.calculate_optical_flow(f1, f2, g, case.R, case.iterations, case.delta, case.nb, 0)
        _chain_cache[k] = (off, tot)
    off, tot = _chain_cache[k]
    kb = k + (case.blur_radius,)
    if kb not in _blur_cache:
        _blur_cache[kb] = oracle.blur_flow(off, g, case.blur_radius)
    return off, _blur_cache[kb], tot


def oracle_results(case, pairs):
    """{key: (offsets, blurred, total delta)} for pairs = {key: (frame N-1, frame N)}; key = (content, index of the pair)."""
    g = M.geometry(case)
    keys = list(pairs)
    return dict(zip(keys, _pool.map(lambda k: _oracle_chain(case, g, pairs[k][0], pairs[k][1], k), keys)))


def make_members(case, n=None, more_flags=0):
    from hopperrender_amd import capi
    from hopperrender_amd.calc import OpticalFlowCalcHDR, OpticalFlowCalcSDR
    cls = OpticalFlowCalcHDR if case.hdr else OpticalFlowCalcSDR
    flags = capi.HF_FLAG_ASYNC | more_flags | {M.ALWAYS: capi.HF_FLAG_SAD_REUSE_ALWAYS, M.NEVER: capi.HF_FLAG_NO_SAD_REUSE, M.DEFAULT: 0}[case.tables]
    return [cls(case.H, case.W, case.in_stride, 0, case.delta, case.nb, 0.0, 255.0, case.max_res, iterations=case.iterations,
                blur_radius=case.blur_radius, search_radius=case.R, flags=flags) for _ in range(case.n if n is None else n)]


def read(c):
    return c.readOffsets(), c.readBlurredFlow(1), c.m_totalFrameDelta


def assert_members(case, cs, keys, want, what):
    out = []
    for i, (c, k) in enumerate(zip(cs, keys)):
        off, blur, tot = read(c)
        w = want[k]
        assert (off == w[0]).all(), (case.name, what, "offsets", i, k, int((off != w[0]).sum()))
        assert (blur == w[1]).all(), (case.name, what, "blur", i, k, int((blur != w[1]).sum()))
        assert tot == w[2], (case.name, what, "delta", i, k, tot, w[2])
        out.append((off, blur, tot))
    return out


def assert_table_counters(case, cc):
    """level_windows, both axes: the windows of the tiles that take a table body, every member's (derived from the model, not from the kernel)."""
    want = M.expected_table_windows(case)
    g = M.geometry(case)
    full = (g.lw // 32) * (g.lh // 32)
    assert want == {ws: case.n * full * (32 // ws) ** 2 for ws in M.windows(case) if ws <= 32 and full}, (case.name, want)
    assert set(cc["levels"]) == set(want), (case.name, cc["levels"], want)
    for ws, lv in cc["levels"].items():
        assert lv["X"][0] == want[ws] and lv["Y"][0] == want[ws], (case.name, ws, lv, want[ws])


def run_case(case, kinds=None, more_flags=0):
    """kinds: the content of each member (default: member_kinds);  more_flags: flags of every member beside the table mode's."""
    from hopperrender_amd.calc import FlowBatch
    kinds = member_kinds(case.n) if kinds is None else list(kinds)
    assert len(kinds) == case.n
    fr = {k: case_frames(case, k) for k in dict.fromkeys(kinds)}
    cs = make_members(case, more_flags=more_flags)
    b = None
    try:
        for c, k in zip(cs, kinds):
            for x in fr[k][:3]:
                c.updateFrame(x)
        b = FlowBatch(cs)
        on = M.tables_on(case)
        counted = bool(on) and case.R == 16
        for pair in (1, 2):
            if pair == 2:
                for c, k in zip(cs, kinds):
                    c.updateFrame(fr[k][3])
                if counted:
                    cs[0].countersEnable(True)
            b.calculateOpticalFlow()
            want = oracle_results(case, {(k, pair): (fr[k][pair], fr[k][pair + 1]) for k in fr})     # (while the GPU works)
            b.sync()
            got = assert_members(case, cs, [(k, pair) for k in kinds], want, f"pair {pair}")
            if on is not None:
                assert all(c.stats()["sad_tables"] == int(on) for c in cs), case.name
        if counted:
            assert_table_counters(case, cs[0].counters(reset=True))
            cs[0].countersEnable(False)
        b.calculateOpticalFlow()         # the same ring positions again: the cached graph's replay (after the counters: a new capture without them)
        b.sync()
        for i, c in enumerate(cs):
            again = read(c)
            assert (again[0] == got[i][0]).all() and (again[1] == got[i][1]).all() and again[2] == got[i][2], (case.name, "replay", i)
    finally:
        if b is not None:
            b.close()
        for c in cs:
            c.close()


@pytest.mark.parametrize("case", M.CASES, ids=lambda c: c.name)
def test_batched_chain_variant_matches_oracle(native_lib, case):
    run_case(case)


@pytest.mark.parametrize("kind", ["static", "noise"])
def test_reuse_count_of_a_batch_of_identical_members(native_lib, kind):
    """The counters are the leader's, all members together: with five members of the SAME content the reused count must be five times the CPU
    model's (tests/flow_reuse_model.py), window for window -- static: every window behind level 32 reuses; noise: the decision flips from
    window to window (about one in seven reuses) -- on a grid with partial tiles."""
    from flow_reuse_model import reuse_shares
    from hopperrender_amd.calc import FlowBatch
    case = M._c("identical", 0, 544, 960, 136, 5)
    f = case_frames(case, kind)
    g = M.geometry(case)
    cs = make_members(case)
    for c in cs:
        for x in f[:3]:
            c.updateFrame(x)
    b = FlowBatch(cs)
    cs[0].countersEnable(True)
    b.calculateOpticalFlow(); b.sync()
    cc = cs[0].counters()
    assert_table_counters(case, cc)
    assert_members(case, cs, [(kind, 1)] * case.n, oracle_results(case, {(kind, 1): (f[1], f[2])}), kind)
    model = {(ws, ax): s for ws, ax, s in reuse_shares(f[1], f[2], g)}
    for ws, lv in cc["levels"].items():
        for ai, ax in enumerate("XY"):
            windows, reused = lv[ax]
            assert abs(reused / windows - model[(ws, ai)]) < 1e-9, (kind, ws, ax, reused, windows, model[(ws, ai)])
            if kind == "static":
                assert reused == (windows if ws < 32 else 0), (ws, ax, lv)
    b.close()
    for c in cs:
        c.close()


def test_members_of_a_batch_are_isolated(native_lib):
    """Seven members, seven different pairs, large-window levels, SAD tables and partial tiles (240 x 136).  After a second run in which only
    member 3's newest frame differs (the same ring positions: the cached graph), every other member's offsets, blur and delta are what they
    were and member 3 has its new oracle's: a member-index rebase (decode_tile, member_step) that reads or writes a neighbour's tables,
    window sums or pending argmin would show in the neighbour or in member 3."""
    from hopperrender_amd.calc import FlowBatch
    case = M._c("isolation", 0, 544, 960, 136, 7)
    kinds = member_kinds(7)
    assert len(set(kinds)) == 7
    fr = {k: case_frames(case, k) for k in kinds}
    cs = make_members(case)
    for c, k in zip(cs, kinds):
        for x in fr[k][:3]:
            c.updateFrame(x)
    b = FlowBatch(cs)
    b.calculateOpticalFlow(); b.sync()
    first = assert_members(case, cs, [(k, 1) for k in kinds], oracle_results(case, {(k, 1): (fr[k][1], fr[k][2]) for k in kinds}), "first run")
    changed = fr["chaotic"][3]              # (member 3 is the static one: its newest frame becomes a frame of other content)
    for i, (c, k) in enumerate(zip(cs, kinds)):      # three frames on: the ring is where it was
        for x in fr[k][:2] + [changed if i == 3 else fr[k][2]]:
            c.updateFrame(x)
    b.calculateOpticalFlow(); b.sync()
    want3 = oracle_results(case, {("changed", 0): (fr[kinds[3]][1], changed)})[("changed", 0)]
    for i, c in enumerate(cs):
        off, blur, tot = read(c)
        w = want3 if i == 3 else first[i]
        assert (off == w[0]).all() and (blur == w[1]).all() and tot == w[2], ("member", i, int((off != w[0]).sum()), int((blur != w[1]).sum()))
    assert (want3[0] != first[3][0]).any()
    b.close()
    for c in cs:
        c.close()


# ------------------------------------------------------------------------------------------------
# the window-sum blur at large even radii on small even grids (blur_flow_kernel<32, 0>: a tile gathers 16 + r windows per edge, more than
# the grid has; the surplus is reflected once and clamped -- tests/test_chain_variant_model.py has the index model)
# ------------------------------------------------------------------------------------------------
SMALL_GRIDS = [(66, 66), (64, 80), (80, 66)]        # lw x lh, resolution scalar 0: the grid is the frame


def run_small_grid_blur(lw, lh, r, n):
    from hopperrender_amd.calc import FlowBatch
    from oracle import oracle
    case = M._c(f"blur-{lw}x{lh}-r{r}-n{n}", 0, lh, lw, 270, n, blur=r, tables=M.NEVER if n < 4 else M.ALWAYS)
    g = M.geometry(case)
    assert (g.rs, g.lw, g.lh) == (0, lw, lh) and M.blur_variant(case) == "blur.32x0"
    kinds = [KINDS[(2 + i) % 7] for i in range(n)]          # noise first: offsets all over the range
    fr = {k: frames(k, lh, lw, False, 9300 + 13 * KINDS.index(k), 3) for k in kinds}
    cs = make_members(case)
    b = None
    try:
        for c, k in zip(cs, kinds):
            for x in fr[k]:
                c.updateFrame(x)
        if n > 1:
            b = FlowBatch(cs)
            b.calculateOpticalFlow(); b.sync()
        else:
            cs[0].calculateOpticalFlow(); cs[0].sync()
        for i, (c, k) in enumerate(zip(cs, kinds)):
            off, _, tot, _ = oracle.calculate_optical_flow(fr[k][1], fr[k][2], g, 16, 0, 8, 6, 0)
            assert (c.readOffsets() == off).all() and c.m_totalFrameDelta == tot, (case.name, i, k)
            assert (c.readBlurredFlow(1) == oracle.blur_flow(off, g, r)).all(), (case.name, i, k)
    finally:
        if b is not None:
            b.close()
        for c in cs:
            c.close()


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("r", [38, 48, 64])
@pytest.mark.parametrize("lw,lh", SMALL_GRIDS)
def test_window_sum_blur_on_small_grids(native_lib, lw, lh, r, n):
    run_small_grid_blur(lw, lh, r, n)
