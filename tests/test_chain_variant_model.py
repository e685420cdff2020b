"""CPU: the model of the chain's and the blur's variant selection (tests/chain_variant_model.py) is compared with the launchers' own plan
functions (csrc/hf_launch_plan.h, called through tests/launch_plan_probe.cpp), and the matrix
that tests/test_chain_variants_gpu.py runs against the oracle reaches every variant and every (variant, tile class) pair the model knows.
A changed threshold in the launchers fails here until the matrix has been reconsidered.  Also: the window-sum blur's gather indices stay
inside the offset tables (the condition the bounds build checks on the device at site 201)."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_variant_model as M  # noqa: E402
import launch_plan_probe  # noqa: E402

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hopperrender_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _int(text, pattern):
    m = re.findall(pattern, text)
    assert len(m) == 1, (pattern, m)
    return int(m[0])


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return launch_plan_probe.load(tmp_path_factory.mktemp("launch_plan_probe"))


def test_thresholds_equal_the_sources(probe):
    """The thresholds of hf_launch_plan.h as the compiled header has them; those of the API layer and of the kernel by their lines."""
    k, kern, calc = probe.constants, _src("hf_kernels.hip"), _src("hf_calc.hip")
    assert k["kRowPerLaneMaxBatch"] == M.ROW_PER_LANE_MAX_BATCH
    assert k["kLevel32OneWaveMinBatch"] == M.LEVEL32_ONE_WAVE_MIN_BATCH
    assert (k["kBigOneWaveMinBatch"], k["kBigOneWaveMinRs"], k["kBigWavesPerBlock"]) == (M.BIG_ONE_WAVE_MIN_BATCH, M.BIG_ONE_WAVE_MIN_RS, 4)
    assert k["kMaxFlowBatch"] == M.MAX_FLOW_BATCH and k["kBlurWindowSumMinDim"] == M.WINDOW_SUM_MIN_DIM
    assert _int(calc, r"if \(n < (\d+)\) return false;") == M.TABLES_MIN_BATCH
    assert _int(calc, r"const bool use_neighbors = k >= (\d+);") == M.NEIGHBOUR_FIRST_LEVEL
    # the window-sum condition the kernel re-tests on the device: the same bound
    dims = re.findall(r"lw >= (\d+) && (?:g\.)?lh >= (\d+)", kern)
    assert dims == [(str(M.WINDOW_SUM_MIN_DIM),) * 2], dims


# ------------------------------------------------------------------------------------------------
# the model against the launchers' own plan functions (hf_launch_plan.h through tests/launch_plan_probe.cpp)
# ------------------------------------------------------------------------------------------------
def model_small_level(n, ws, R, tables_present, sad_read, sad_write):
    """The fields of a small level's launch as M.launches decides them (one_wave32, rows1, tile_w, waves, tabk, block)."""
    rows1 = n <= M.ROW_PER_LANE_MAX_BATCH and ws <= 4
    one_wave = ws == 32 and n >= M.LEVEL32_ONE_WAVE_MIN_BATCH
    waves = 1 if ws == 32 else 4 if ws >= 8 else (4 if rows1 or ws == 2 else 2)
    return (int(one_wave), int(rows1), 16 if rows1 and ws == 2 else 32, waves, int(tables_present and R == 16 and (sad_read or sad_write)),
            256 if ws == 32 and not one_wave else 64)


def test_chain_plans_equal_the_model_on_the_grid(probe):
    """Every n in 1 .. 32, every window 2 .. 256, R in {2, 5, 11, 16}, rs 0 .. 6, tables on / off: the three chain plan functions against the
    selectors the model's launches() restates; moving a threshold in the header names the inputs that changed kernel here."""
    windows = [256, 128, 64, 32, 16, 8, 4, 2]
    for n in range(1, 33):
        for rs in range(7):
            assert probe.plan_flow_big_waves(n, rs) == (1 if n >= M.BIG_ONE_WAVE_MIN_BATCH and rs >= M.BIG_ONE_WAVE_MIN_RS else 4), (n, rs)
        for ws in windows[3:]:
            for R in (2, 5, 11, 16):
                for present in (False, True):
                    for rd, wr in ((0, 0), (0, 1), (1, 0), (1, 1)):
                        assert tuple(probe.plan_flow_level_small(n, ws, R, present, rd, wr)) == model_small_level(n, ws, R, present, rd, wr), (n, ws, R, present, rd, wr)
    for first in range(len(windows)):
        for last in range(first + 1, len(windows) + 1):
            ws_list = windows[first:last]
            for k, ws in enumerate(ws_list):
                for on in (False, True):
                    want = (on and ws <= 32 and k > 0 and ws_list[k - 1] <= 32, on and 4 <= ws <= 32)
                    assert probe.plan_sad_tables(ws_list, k, on) == want, (ws_list, k, on)


@pytest.mark.parametrize("case", M.CASES, ids=lambda c: c.name)
def test_chain_plans_equal_the_model_on_the_matrix(probe, case):
    """Every launch of every case of the matrix, in each table mode the case can run in: the plan's variant is the model's."""
    g = M.geometry(case)
    ws_list = M.windows(case, g)
    for on in ((False, True) if M.tables_on(case) is None else (M.tables_on(case),)):
        lns = M.launches(case, tab=on)
        steps = [(k, ws) for k, ws in enumerate(ws_list) for _axis in ((0, 1) if ws > 32 else (0,))]
        assert len(steps) == len(lns)
        for (k, ws), ln in zip(steps, lns):
            kind = ln.variant.rsplit(".", 1)[1]
            if ws > 32:
                wpb = probe.plan_flow_big_waves(case.n, g.rs)
                assert ln.variant == f"big.wave{wpb}.{'r16' if case.R == 16 else 'anyR'}"
                assert ln.units == -(-g.lw // 64) * -(-g.lh // (4 * wpb)) * case.n
                continue
            rd, wr = probe.plan_sad_tables(ws_list, k, on)
            P = probe.plan_flow_level_small(case.n, ws, case.R, on, rd, wr)
            name = ("level32.wave" if P.one_wave32 else "level32.four_wave") if ws == 32 else f"level{ws}" if ws >= 8 else f"level{ws}.{'row' if P.rows1 else 'block'}"
            assert ln.variant == f"{name}.{'tab' if P.tabk else 'plain' if case.R == 16 else 'anyR'}", (case.name, ws, ln.variant, P)
            assert ln.units == -(-g.lw // P.tile_w) * -(-g.lh // 32) * P.waves * case.n
            assert (kind == "tab") == bool(P.tabk) and bool(ln.table_windows) == (bool(P.tabk) and "full" in ln.tile_classes)     # (a grid without a full tile has no table body)
    blur = probe.plan_blur(tuple(g_tuple(g)), case.n, case.blur_radius, ws_list[-1] if ws_list else 0)
    assert launch_plan_probe.BLUR_KERNELS[blur.kernel] == M.blur_variant(case), case.name


def g_tuple(g):
    return (g.hdr, g.H, g.W, g.in_stride, g.out_stride, g.rs, g.lw, g.lh)


def model_blur(lw, lh, n, r, last_window):
    """M.blur_variant's decision and the launch's tile and dynamic LDS bytes (hf_kernels.hip blur_flow_kernel's layouts)."""
    window_sums = last_window == 2 and not (lw & 1) and not (lh & 1) and lw >= M.WINDOW_SUM_MIN_DIM and lh >= M.WINDOW_SUM_MIN_DIM
    if r == 4 and (n > 4 or window_sums):
        return ("blur.32x4.window_sums" if window_sums else "blur.32x4.taps"), 32, 40 * 41 * 4 + 2 * 40 * 32 * 4
    if window_sums and 2 <= r <= 64 and not (r & 1):
        return "blur.32x0", 32, (16 + r) ** 2 * 4 + 2 * (16 + r) * 17 * 4 + 2 * 17 * 17 * 4
    return "blur.16x0", 16, (16 + 2 * r) * (17 + 2 * r) * 4 + 2 * (16 + 2 * r) * 16 * 4


def test_blur_plan_equals_the_model_on_the_grid(probe):
    """Every even and a few odd radii 2 .. 64 on grids 62 .. 162, even and odd, batches on both sides of n > 4, last level 2 or not."""
    seen = set()
    for lw in list(range(62, 68)) + [96, 127, 128, 161, 162]:
        for lh in list(range(62, 68)) + [97, 160, 162]:
            g = (0, lh * 4, lw * 4, lw * 4, lw * 4, 2, lw, lh)
            for r in list(range(2, 65, 2)) + [3, 5, 7, 33, 63]:
                for n in (1, 4, 5, 32):
                    for last in (2, 4, 32, 0):
                        P = probe.plan_blur(g, n, r, last)
                        want = model_blur(lw, lh, n, r, last)
                        assert (launch_plan_probe.BLUR_KERNELS[P.kernel], P.tile, P.lds_bytes) == want, (lw, lh, r, n, last, P)
                        assert (P.grid_x, P.grid_y) == (-(-lw // P.tile), -(-lh // P.tile))
                        seen.add(want[0])
    # a last level of 2 whose tables do not cover the grid (never built by the API layer) has no window sums
    assert launch_plan_probe.BLUR_KERNELS[probe.plan_blur((0, 256, 256, 256, 256, 2, 64, 64), 1, 4, 2, nwx=31).kernel] == "blur.16x0"
    assert seen == set(launch_plan_probe.BLUR_KERNELS)


def test_batch_argument_limit():
    """A 32-member case is in the matrix and it is the largest a launch's 4 KB of kernel arguments hold (hf_flow.hip FlowBatchArgs; 33 members
    are refused: test_batch_period_gpu.py)."""
    flow = _src("hf_flow.hip")
    assert "FlowPtrs m[kMaxFlowBatch];" in flow
    assert "static_assert(sizeof(FlowBatchArgs) + sizeof(Geom) <= 4096" in flow
    assert "if (n > hf::kMaxFlowBatch) return batch_fail(nullptr, HF_ERR_INVALID_ARGUMENT" in _src("hf_batch.hip")
    # 13 buffer pointers are named in the comment, seven allocations travel: 56 bytes a member; one FlowStep + Geom must fit beside 32 of them
    assert M.MAX_FLOW_BATCH * 7 * 8 < 4096
    assert max(c.n for c in M.CASES) == M.MAX_FLOW_BATCH and all(1 <= c.n <= M.MAX_FLOW_BATCH for c in M.CASES)


def test_model_on_known_shapes():
    c = M._c("x", 0, 1080, 1920, 270, 6)
    assert M.windows(c) == [256, 128, 64, 32, 16, 8, 4, 2]
    v = M.labels(c)
    assert {"big.wave1.r16", "level32.wave.tab", "level16.tab", "level8.tab", "level4.block.tab", "level2.block.tab", "argmin.lazy",
            "blur.32x4.window_sums", "tables.on"} <= v and "argmin.explicit" not in v
    full = (480 // 32) * (270 // 32)
    assert M.expected_table_windows(c) == {ws: 6 * full * (32 // ws) ** 2 for ws in (32, 16, 8, 4, 2)}
    one = M._c("x", 0, 1080, 1920, 270, 1, tables=M.DEFAULT)
    assert {"big.wave4.r16", "level32.four_wave.plain", "level4.row.plain", "level2.row.plain", "tables.default"} <= M.labels(one)
    # 240 x 136, four members: MapRow<2>'s tile at columns 224 .. 239 is full, its 32-wide tile is not -- and stays out of the table count
    c = M._c("x", 1, 1088, 1920, 136, 4)
    last = M.launches(c)[-1]
    assert last.variant == "level2.row.tab" and last.tile_classes == {"full", "half", "bottom"}      # (240 = 15 x 16: no 16-wide tile crosses the edge)
    assert last.table_windows == 4 * (7 * 4) * 16 * 16
    # R < 16: no tile is full, no tables whatever the flag says
    assert {ln.variant.rsplit(".", 1)[1] for ln in M.launches(M._c("x", 0, 544, 960, 136, 5, R=5))} == {"anyR"}
    # rs 1 with four members: one-wave level 32, four-wave large windows
    assert {"level32.wave.tab", "big.wave4.r16"} <= M.labels(M._c("x", 0, 540, 960, 270, 4))
    # a chain of three levels ends on a large window; the 1388-wide grid has one at the first neighbour-term level
    assert M.argmin_labels(M._c("x", 0, 1080, 1920, 270, 5, it=3)) == {"argmin.lazy", "argmin.explicit"}
    assert M.windows(M._c("x", 0, 568, 1388, 1000, 5))[4] == 64
    assert M.blur_variant(M._c("x", 0, 1082, 1922, 270, 4)) == "blur.16x0" and M.blur_variant(M._c("x", 0, 1082, 1922, 270, 5)) == "blur.32x4.taps"
    assert M.blur_variant(M._c("x", 0, 1080, 1920, 270, 5, blur=7)) == "blur.16x0" and M.blur_variant(M._c("x", 0, 1080, 1920, 270, 5, blur=64)) == "blur.32x0"


def test_matrix_reaches_every_variant_and_tile_class():
    names = [c.name for c in M.CASES]
    assert len(set(names)) == len(names)
    seen = set().union(*(M.labels(c) for c in M.CASES))
    assert seen == M.ALL_VARIANTS, (sorted(M.ALL_VARIANTS - seen), sorted(seen - M.ALL_VARIANTS))
    got = set().union(*(M.pairs(c) for c in M.CASES))
    assert M.required_pairs() <= got, sorted(M.required_pairs() - got)


def test_matrix_holds_what_the_issue_lists():
    """The axes named for the matrix, each with the batch sizes asked for."""
    cs = M.CASES
    assert {4, 5, 7, 13, 16, 32} <= {c.n for c in cs}
    assert {c.n for c in cs if (c.hdr, c.H) in ((0, 1080), (1, 2160))} >= {16}
    assert {16, 11, 5, 2} <= {c.R for c in cs} and {0, 4, 6, 3} <= {c.iterations for c in cs}
    assert {(8, 6), (3, 0), (0, 10), (10, 10)} <= {(c.delta, c.nb) for c in cs}
    for r in (4, 2, 32, 64, 7):
        assert any(c.blur_radius == r and c.n > 4 for c in cs) and any(c.blur_radius == r and c.n == 4 for c in cs), r
    assert any(c.in_stride for c in cs) and sum(c.W == 1388 for c in cs) == 1
    assert sum(c.tables == M.DEFAULT for c in cs) >= 3
    grids = {(M.geometry(c).rs, M.geometry(c).lw, M.geometry(c).lh, c.hdr) for c in cs}
    assert {(2, 480, 270, 0), (2, 480, 270, 1), (3, 480, 270, 1), (3, 240, 136, 1), (2, 240, 136, 0), (1, 480, 270, 0), (1, 480, 270, 1),
            (0, 480, 256, 0), (2, 481, 271, 0), (1, 32, 32, 0), (1, 64, 64, 0), (0, 1388, 568, 0)} <= grids, sorted(grids)
    assert 30 <= len(cs) <= 40


# ------------------------------------------------------------------------------------------------
# the window-sum blur's gather indices
# ------------------------------------------------------------------------------------------------
DIMS = range(64, 161, 2)
RADII = range(2, 65, 2)


def test_blur_window_sum_indices_stay_inside_the_tables():
    """blur_flow_kernel<32, 0> gathers 16 + r windows per tile edge.  One reflection does not bring all of them back into [0, nw) once
    r / 2 + 16 exceeds the windows left of the last tile's origin: the clamp after it does (hf_kernels.hip; the kernel's form is pinned below)."""
    for dim in DIMS:
        for r in RADII:
            idx = M.blur_window_indices(dim, r)
            assert min(idx) >= 0 and max(idx) < dim // 2, (dim, r, min(idx), max(idx))


def test_blur_single_reflection_alone_leaves_the_tables():
    """The formula before the clamp: out of range from r = 38 on a 66-pixel axis (lh = 66, r = 64: -14), in range for every r at 160.  This is
    what the clamp is for; the radius-4 form (20 windows from X0 / 2 - 2, grids of at least 64) needs none."""
    bad = {(dim, r) for dim in DIMS for r in RADII if min(M.blur_window_indices(dim, r, clamp=False)) < 0}
    assert min(r for dim, r in bad if dim == 66) == 38 and min(r for dim, r in bad) == 38
    assert min(M.blur_window_indices(66, 64, clamp=False)) == -14
    assert not any(dim == 160 for dim, r in bad)
    for dim in DIMS:
        idx = M.blur_window_indices(dim, 4, fixed4=True, clamp=False)
        assert min(idx) >= 0 and max(idx) < dim // 2, dim


def test_blur_clamp_changes_no_output_inside_the_grid():
    """Every window an output inside the grid sums is in range after ONE reflection: the clamp only touches a tile's surplus windows."""
    for dim in DIMS:
        nw = dim // 2
        for r in RADII:
            ws = M.blur_windows_of_outputs(dim, r)
            lo, hi = min(ws), max(ws)
            assert -1 - lo < nw and 2 * nw - 1 - hi >= 0, (dim, r, lo, hi)


def test_blur_index_model_is_the_kernels_formula():
    kern = _src("hf_kernels.hip")
    for a, n in (("wa", "nwx"), ("wb", "nwy")):
        single = f"{a} = {a} < 0 ? -1 - {a} : {a} >= L.{n} ? 2 * L.{n} - 1 - {a} : {a};"
        clamped = f"{a} = clampi({a} < 0 ? -1 - {a} : {a} >= L.{n} ? 2 * L.{n} - 1 - {a} : {a}, 0, L.{n} - 1);"
        assert kern.count(single) == 1 and kern.count(clamped) == 1, a      # <32, 4>'s form / <32, 0>'s
        assert kern.index(single) < kern.index("if constexpr (TS == 32 && RFIX == 0)") < kern.index(clamped)
    assert "const int wa0 = X0 / 2 - r / 2, wb0 = Y0 / 2 - r / 2;" in kern and "const int NW = 16 + r;" in kern
    assert "const int wa0 = X0 / 2 - 2, wb0 = Y0 / 2 - 2;" in kern and "constexpr int NW = 20, NS = 17;" in kern


@pytest.mark.parametrize("case", M.CASES, ids=lambda c: c.name)
def test_stale_table_invariant_of_the_matrix(case):
    """Every level that reads the SAD tables follows a level of the same chain that wrote them (hf_calc.hip asserts it on the host)."""
    ws = M.windows(case)
    for k, w in enumerate(ws):
        if w <= 32 and k > 0 and ws[k - 1] <= 32:
            assert ws[k - 1] >= 4
