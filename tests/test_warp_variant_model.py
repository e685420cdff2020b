"""CPU: the model of the warp's launch selection (tests/warp_variant_model.py) is compared with the launchers' own plan functions
(csrc/hf_launch_plan.h, called through tests/launch_plan_probe.cpp) over whole grids of shapes, its model of the staged kernel's workgroup
bodies is pinned to the device code line by line, the compiled instantiations are exactly the ones the model can launch plus a stated list of unreachable ones, and the matrix that
tests/test_warp_variants_gpu.py runs against the oracle reaches every launch label in each of modes 0, 1, 2, the generic kernel in modes
3 to 6, every plane-emission variant and every (element type, plane, workgroup class) pair.  A changed threshold in the launchers or in
warp_wg_body fails here until the matrix has been reconsidered.

Which test judges a label by the oracle or the golden frames (new: the case of the matrix, tests/test_warp_variants_gpu.py)

  label                                          reached before by                                              new case
  fast.u16.vb16.g8.dw.all.w4                     test_fused_fullsize_gpu (one context, 2160p HDR, golden)       all-u16-1088-res136-src0-single
  fast.u8.vb8.g4.dw.one.w4                       test_fused_fullsize_gpu (one context, 1080p SDR, golden)       one-u8-180-res67-src0-*
  fast.u8.vb8.g4.dw.all.w4                       test_batch_1080p_shapes_gpu (12 / 16 members, golden)          all-u8-1080-res270-src0-n11
  fast.u16.vb16.g4.dw.all.w4                     test_fused_fullsize_gpu (1080p HDR x 12)                       all-u16-1088-res272-src0-single
  fast.u8.vb16.g8.dw.all.w4                      test_fused_fullsize_gpu (2160p SDR x 1 / 3, 1440p SDR x 4)     all-u8-1536-res192-src0-single
  fast.u8.vb16.g16.dw.all.w4                     test_fused_fullsize_gpu (4320p SDR x 2)                        all-u8-1536-res96-src0-single
  fast.*.one.w4 with vb8 (dw)                    test_random_gpu, test_parity_gpu (single contexts)             one-*-180-*-src0-*
  every other fast.*.dw.one.w4 (vb16)            none                                                           one-u16-768-*, one-u8-1088-*
  every fast.*.nodw.* (24 labels)                test_timed_kernel_shapes_gpu reaches none (base + 8 bytes      *-src2-*
                                                 stays dword aligned): none
  fast.u8.vb8.g2 / g8 .all, fast.u16.vb8.*.all   none                                                           all-u8-1080-res540 / res135, all-u16-720-*
  fast.u16.vb16.g2.*, fast.u8.vb16.g4.*          none                                                           all-u16-1088-res544-*, all-u8-1536-res384-*
  fast.u16.vb16.g8.*.all.w16, fast.u8...g16..w16 none (batches of two outputs or more are staged now)           w16-*
  staged.u16.rs3                                 test_fused_fullsize_gpu (2160p HDR x 4 / 16; pixels only)      staged-u16-res136-*, split-u16-1088-n30
  staged.u16.rs3.planes, plane.u16.rs3           test_timed_kernel_shapes_gpu, test_deferred_planes_gpu         period-u16-res136-n14
  plane.fallback                                 test_timed_kernel_shapes_gpu (mode 2)                          period-* (modes 0, 1, 2)
  staged.u16.rs4, staged.u8.rs4                  test_fused_fullsize_gpu (4320p x 2, mode 2)                    staged-u16-res68-*, staged-u8-res68-*
  staged.*.rs4.planes, plane.*.rs4               test_deferred_planes_gpu (4320p, planes compared)              period-u16-res68-n14, period-u8-res68-n15
  staged.*.rs5, staged.*.rs6                     none                                                           staged-*-res34-*, staged-*-res17-*
  generic.*, copy.*                              test_parity_gpu, test_ref_live_gpu (golden)                    generic-*, copy-*
  split                                          test_batch_period_gpu (pixels of 32 members)                   split-*
No earlier test read the staged kernel's counters against anything but "> 0.8 if any"; every staged case of the matrix now does, exactly."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import launch_plan_probe  # noqa: E402
import warp_variant_model as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hopperrender_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _ints(text, pattern):
    m = re.findall(pattern, text)
    assert len(m) == 1, (pattern, m)
    return tuple(int(x) for x in (m[0] if isinstance(m[0], tuple) else (m[0],)))


def _once(text, snippet, times=1):
    assert text.count(snippet) == times, (snippet, text.count(snippet))


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return launch_plan_probe.load(tmp_path_factory.mktemp("launch_plan_probe"))


def test_constants_equal_the_sources(probe):
    """The constants of hf_launch_plan.h as the compiled header has them; those of the device code by their lines."""
    k, kern = probe.constants, _src("hf_kernels.hip")
    assert (k["kWarpTX"], k["kWarpTY"]) == (M.WARP_TX, M.WARP_TY)
    assert (k["kWarpWavesSmall"], k["kWarpWavesLarge"]) == (M.WAVES_SMALL, M.WAVES_LARGE)
    assert (k["kWgWaves"], k["kWgRows"], k["kWgChunksPerWave"]) == (M.WG_WAVES, M.WG_ROWS, M.WG_CHUNKS_PER_WAVE)
    assert k["kWgMinWaves"] == M.WG_MIN_WAVES and k["kWarpRounds"] == M.ROUNDS and k["kSmallFrameBytes"] == M.SMALL_FRAME_BYTES
    assert (k["kMaxWarpBatch"], k["kMaxWarpOutputs"], k["kMaxFlowBatch"]) == (M.MAX_WARP_BATCH, M.MAX_WARP_OUTPUTS, M.MAX_FLOW_BATCH)
    assert k["kWarpFastRows"] == M.FAST_ROWS and k["wg_chunks_1"] == M.WG_CHUNKS_PER_WAVE
    assert _ints(kern, r"constexpr int kExtX = (\d+), kExtY = (\d+);") == (M.EXT_X, M.EXT_Y)
    assert _ints(kern, r"constexpr int kWgCells = (\d+);") == (M.WG_CELLS,)
    assert _ints(kern, r"constexpr int VEC = 16 / \(int\)sizeof\(E\), NDW = (\d+), CHUNKS = wg_chunks\(NW \* ROWS / 2\), SZ") == (M.NDW,)
    _once(kern, "constexpr int WR = kWgRows, NW = kWgWaves * 2 / WR;")
    assert M.SMALL_FRAME_BYTES == 1920 * 1088 and M.ROUNDS == 4 * 8192


def test_launch_comparisons_equal_the_sources():
    """What the launch selection rests on outside hf_launch_plan.h: device code and API-layer control flow, by their lines.  (The selection
    itself is compared with the model by calling it: the test_plan_* tests below.)"""
    kern, batch, calc = _src("hf_kernels.hip"), _src("hf_batch.hip"), _src("hf_calc.hip")
    _once(kern, "if (sizeof(E) == 2 && g.rs == 3) plane_fast_task<E, 3, 1>(")
    _once(kern, "else plane_fast_task<E, 4, 1>(")
    _once(batch, "b->defer_planes = !l->dual() && !(l->cfg.flags & HF_FLAG_BATCH_EAGER_PLANES) && hf::warp_period_can_build_planes(l->g, l->pl, n);")
    _once(batch, "if (n_out && calculate_flow && b->defer_planes && mode >= 0 && mode <= 2) {")
    _once(_src("hf_context.hip"), "const int max_iters = ilog2(ws0);")
    _once(calc, "const bool fuse = n_out >= 2 && !(c->cfg.flags & HF_FLAG_NO_FUSED_WARP);")


# ------------------------------------------------------------------------------------------------
# the model against the launchers' own plan functions (hf_launch_plan.h through tests/launch_plan_probe.cpp)
# ------------------------------------------------------------------------------------------------
def max_iters(g):
    """hf_context.hip: log2 of the initial window, the power of two that covers the grid."""
    d = max(g.lw, g.lh)
    return M.ilog2(d if d & (d - 1) == 0 else 1 << d.bit_length())


def _up8(v):
    return -(-v // 8) * 8


def plan_label(g, L):
    if L.family == launch_plan_probe.STAGED:
        return f"staged.{M.ename(g)}.rs{g.rs}" + (".planes" if L.planes else "")
    assert L.family == launch_plan_probe.FAST, L
    return f"fast.{M.ename(g)}.vb{L.vb}.g{L.group}.{'dw' if L.dw else 'nodw'}.{'all' if L.out_chunk > 1 else 'one'}.w{L.waves}"


def check_launch_fields(g, L, ms):
    """The fields of a planned launch that its label does not carry, from the model's tile and block counts."""
    vec, part = L.vb // M.esize(g), ms[L.first:L.first + L.count]
    wpr, n_tiles = M.tile_counts(g, vec)
    max_out = max(m.n_out for m in part)
    assert L.out_chunk in (1, M.MAX_WARP_OUTPUTS) and L.n_chunks == -(-max_out // L.out_chunk)
    assert (L.rows, L.y_groups, L.block) == (M.FAST_ROWS, -(-g.H // M.FAST_ROWS), 64 * L.waves)
    if L.family == launch_plan_probe.STAGED:
        nw = M.WG_WAVES * 2 // M.WG_ROWS
        pb = M.plane_blocks(g) if L.planes else 0
        nb = M.wg_blocks_per_member(g, pb)
        assert (L.vb, L.group, L.dw, L.waves, L.plane_blocks, L.blocks_per_member, L.wpr) == (16, vec, 1, nw, pb, nb, wpr)
        assert (L.max_unit, L.grid, L.lds_bytes) == (nb * L.count + 8, _up8(nb * L.count), 2 * (nw * M.WG_ROWS // 2) * M.WG_CHUNKS_PER_WAVE * 16)
    else:
        assert L.grid == _up8(-(-n_tiles // L.waves) * L.n_chunks * L.count) and L.planes == 0


class Real:
    """The model's launch functions answered by the plan functions: each checks that the model says the same, then returns the REAL answer, so
    whatever M.launches / M.labels build on top of them is built from the launchers' own decisions."""

    def __init__(self, probe):
        self.probe, self.arrays, self.calls = probe, {}, 0
        self.model = {n: getattr(M, n) for n in ("launch_warp_periods", "launch_warp_t", "launch_copy_t", "defers_planes")}

    def members(self, ms, levels, pending):
        key = (tuple(ms), levels, None if pending is None else tuple(pending))
        a = self.arrays.get(key)
        if a is None:
            a = self.arrays[key] = launch_plan_probe.members_array(
                [launch_plan_probe.member(m.n_out, m.ts, m.src_off, m.out_off, levels, wants_plane=bool(pending and pending[i])) for i, m in enumerate(ms)])
        return a

    def launch_warp_periods(self, g, mode, ms, levels, pending=None):
        self.calls += 1
        plan = self.probe.plan_warp(g, mode, self.members(ms, levels, pending), pending is not None, max_iters(g))
        real = [M.Launch(plan_label(g, L), L.first, L.count, L.family == launch_plan_probe.STAGED,
                         tuple(L.first + i for i in range(L.count) if L.planes >> i & 1), len(plan) > 1) for L in plan] or None
        want = self.model["launch_warp_periods"](g, mode, ms, levels, pending)
        assert real == want, ("plan_warp_periods", g, mode, len(ms), ms[:1], levels, pending is not None, real, want)
        for L in plan:
            check_launch_fields(g, L, ms)
        return real

    def launch_warp_t(self, g, mode, m, levels):
        self.calls += 1
        one = M.Member(1, m.ts[:1], m.src_off, m.out_off, m.flow)
        plan = self.probe.plan_warp(g, mode, self.members([one], levels, None))
        if plan:
            check_launch_fields(g, plan[0], [one])
            real = plan_label(g, plan[0])
        else:
            P, vec = self.probe.plan_warp_generic(g, m.out_off), 16 // M.esize(g)
            assert (P.grid_x, P.grid_y, P.block) == (-(-g.W // (64 * vec)), (g.H + (g.H >> 1) + 3) // 4, 256)
            real = f"generic.{M.ename(g)}.{'aligned' if P.aligned else 'unaligned'}"
        want = self.model["launch_warp_t"](g, mode, m, levels)
        assert real == want, ("launch_warp", g, mode, m, levels, real, want)
        return real

    def launch_copy_t(self, g, m):
        self.calls += 1
        P, vec = self.probe.plan_copy(g, m.src_off, m.out_off), 16 // M.esize(g)
        assert (P.grid_x, P.grid_y, P.block) == (-(-g.W // (64 * vec)), (g.H + (g.H >> 1) + 3) // 4, 256)
        real, want = f"copy.{M.ename(g)}.{'aligned' if P.aligned else 'unaligned'}", self.model["launch_copy_t"](g, m)
        assert real == want, ("plan_copy", g, m, real, want)
        return real

    def defers_planes(self, g, n_members):
        self.calls += 1
        real, want = self.probe.can_build_planes(g, max_iters(g), n_members), self.model["defers_planes"](g, n_members)
        assert real == want, ("warp_period_can_build_planes", g, n_members, real, want)
        return real


@pytest.fixture
def real(probe, monkeypatch):
    r = Real(probe)
    for name in r.model:
        monkeypatch.setattr(M, name, getattr(r, name))
    return r


def test_plan_equals_the_model_over_the_sweep(real):
    """Every shape of sweep_labels() in modes 0 to 3: the plan functions decide what the model decides, field by field, and so produce
    exactly the declared labels and no other."""
    seen = sweep_labels()
    assert real.calls > 4 * 105600
    for mode in (0, 1, 2):
        assert seen[mode] == M.MODE_LABELS | M.COPY_LABELS, (mode, sorted(seen[mode] ^ (M.MODE_LABELS | M.COPY_LABELS)))
    assert seen[3] == M.GENERIC_LABELS | M.COPY_LABELS, sorted(seen[3])


def test_plan_equals_the_model_on_the_matrix(real):
    """Every case of the matrix in each of its modes, ahead of the chain and not."""
    seen = set()
    for c in M.CASES:
        for mode in c.modes:
            seen |= M.labels(c, mode)
            for ahead in (False, True):
                if c.path in ("batch", "period"):
                    M.launches(c, mode, ahead_of_chain=ahead)
    assert seen == M.MODE_LABELS | M.COPY_LABELS and real.calls > len(M.CASES)


SWEEP_SIZES = [(180, 320), (360, 640), (720, 1280), (1080, 1920), (1088, 1536), (1088, 2816), (1440, 2560), (2160, 3840), (4320, 7680), (722, 1282)]


def test_deferral_and_phase_layout_equal_the_plan(probe, real):
    """defers_planes against warp_period_can_build_planes and phase_layout against make_phase_layout on the sweep's geometries."""
    deferring = 0
    for hdr in (0, 1):
        for H, W in SWEEP_SIZES:
            for mr in (67, 135, 270, 540, 1080, 4320):
                for si in (0, W + 2, W + 8, W + 64):
                    g = M.geometry(M._c("s", hdr, H, W, mr, si=si))
                    pl = probe.phase_layout(g, max_iters(g))
                    nph = 1 << g.rs
                    assert (pl.mx, pl.lwp) == M.phase_layout(g) and (pl.rs, pl.nph, pl.nph2) == (g.rs, nph, max(1, nph // 2)), g
                    assert pl.bytes == g.H * pl.nph2 * pl.lwp * 4
                    deferring += sum(real.defers_planes(g, n) for n in (0, 1, 2, 3, 4, 10, 11, 15, 16, 17, 32))
    assert deferring > 50


def _both_sides(real, c, modes=(0, 1, 2)):
    """The labels of a case per mode, from the plan (compared with the model on the way)."""
    return [M.labels(c, m) for m in modes]


def test_plan_on_both_sides_of_each_threshold(probe, real):
    P, g1080 = launch_plan_probe, M.geometry(M._c("x", 1, 1080, 1920, 135))
    # 10 and 11 members of 1080p HDR at rs 3
    assert _both_sides(real, M._c("x", 1, 1080, 1920, 135, 10)) == [{"fast.u16.vb16.g8.dw.one.w4"}] * 3
    assert _both_sides(real, M._c("x", 1, 1080, 1920, 135, 11)) == [{"staged.u16.rs3"}] * 3
    # frames of exactly 1920 x 1088 bytes (8-byte threads) and exactly twice that (the last size with one output per thread), and just above
    assert _both_sides(real, M._c("x", 0, 1088, 1920, 272, 1, path="single")) == [{"fast.u8.vb8.g4.dw.one.w4"}] * 3
    assert _both_sides(real, M._c("x", 0, 1090, 1920, 272, 1, path="single")) == [{"fast.u8.vb16.g4.dw.one.w4"}] * 3
    assert _both_sides(real, M._c("x", 1, 1088, 1920, 272, 1, path="single")) == [{"fast.u16.vb16.g4.dw.one.w4"}] * 3
    assert _both_sides(real, M._c("x", 1, 1090, 1920, 272, 1, path="single")) == [{"fast.u16.vb16.g4.dw.all.w4"}] * 3
    assert not real.defers_planes(M.geometry(M._c("x", 0, 1088, 1920, 136)), 16)
    # 16 and 17, 32 and 33, 0 members
    for n, want in ((16, 1), (17, 2), (32, 2), (33, 0), (0, 0)):
        ms = [M.Member(2, (0.0, 1.0), 0, 0, "uniform:9:-5")] * n
        r = real.launch_warp_periods(g1080, 2, ms, (0.0, 255.0))
        assert len(r or []) == want and (not r or [ln.count for ln in r] == [min(16, n), n - 16][:want]), (n, r)
    # n_out 0, 1, 6, 7 -- one member out of range and nothing at all is launched, whichever part it is in
    for n_out, ok in ((0, False), (1, True), (6, True), (7, False)):
        for at in (0, 20):
            ms = [M.Member(2, (0.0, 1.0), 0, 0, "uniform:9:-5")] * 21
            ms[at] = M.Member(n_out, M.T6[:min(n_out, 6)], 0, 0, "uniform:9:-5")
            assert (real.launch_warp_periods(g1080, 2, ms, (0.0, 255.0)) is not None) == ok, (n_out, at)
    # a blend scalar outside [0, 1]; a member without packed flow
    for ts, ok in (((0.0, 1.0), True), ((-0.001, 1.0), False), ((0.0, 1.001), False)):
        assert (real.launch_warp_periods(g1080, 2, [M.Member(2, ts, 0, 0, "uniform:9:-5")], (0.0, 255.0)) is not None) == ok, ts
    assert probe.plan_warp(g1080, 2, [P.member(2, (0.0, 1.0))]) and not probe.plan_warp(g1080, 2, [P.member(2, (0.0, 1.0), has_flow_xy=False)])
    # mode 2 with levels the blend cannot take: white == black, white == 0, NaN -- modes 0 and 1 do not look at them
    for levels in ((16.0, 16.0), (-5.0, 0.0), (0.0, float("nan")), (float("nan"), 255.0)):
        lb = _both_sides(real, M._c("x", 1, 1080, 1920, 135, 3, levels=levels))
        assert lb[0] == lb[1] == {"fast.u16.vb16.g8.dw.one.w4"} and lb[2] == {"generic.u16.aligned"}, (levels, lb)
    # dw is decided per part: only the second launch of 20 members has a source at base + 2
    ms = [M.Member(2, (0.0, 1.0), 0, 0, "uniform:9:-5")] * 19 + [M.Member(2, (0.0, 1.0), 2, 0, "uniform:9:-5")]
    assert [ln.label for ln in real.launch_warp_periods(g1080, 0, ms, (0.0, 255.0))] == ["staged.u16.rs3", "fast.u16.vb16.g8.nodw.one.w4"]
    # a small frame whose outputs are 8- but not 16-byte aligned takes 8-byte threads; at rs 0 neither 8- nor 16-byte threads hold a cell pair
    assert _both_sides(real, M._c("x", 0, 180, 320, 67, 2, out=(8,))) == [{"fast.u8.vb8.g4.dw.one.w4"}] * 3
    assert _both_sides(real, M._c("x", 0, 180, 320, 270, 2, out=(8,))) == [{"generic.u8.unaligned"}] * 3
    # planes: asked for without a layout, with one, with a frame21 that is not 16-byte aligned
    g2160, two = M.geometry(M._c("x", 1, 2160, 3840, 270)), (0.0, 1.0)
    for have_pl, wants, off21, planes in ((False, True, 0, 0), (True, False, 0, 0), (True, True, 0, 0b1111), (True, True, 8, 0b0111)):
        ms = [P.member(2, two, wants_plane=wants) for _ in range(3)] + [P.member(2, two, wants_plane=wants, src21_off=off21)]
        (L,) = probe.plan_warp(g2160, 2, ms, have_pl, max_iters(g2160))
        assert (L.family, L.planes, L.plane_blocks) == (P.STAGED, planes, M.plane_blocks(g2160) if planes else 0), (have_pl, wants, off21, L)
    # one 8K-class shape on each side of fastdiv_exact: (blocks per member x members + 8) x blocks per member against 2^32
    for n, staged in ((12, True), (13, False)):       # 5760 x 7680 HDR at rs 4: 18,900 workgroups a member
        c = M._c("x", 1, 5760, 7680, 360, n, (2,))
        g = M.geometry(c)
        nb = M.wg_blocks_per_member(g, M.plane_blocks(g))
        assert probe.fastdiv_exact(nb * n + 8, nb) == ((nb * n + 8) * nb < 1 << 32) == staged, (n, nb)
        assert _both_sides(real, c) == [{"staged.u16.rs4" if staged else "fast.u16.vb16.g8.dw.all.w16"}] * 3, n


def test_workgroup_decision_equals_the_sources():
    kern = _src("hf_kernels.hip")
    _once(kern, "const int lcw = rs + CZ;")
    _once(kern, "const int lgx = max(0, ilog2c(TW) - lcw), lgy = max(0, ilog2c(TH) - rs);")
    _once(kern, "const int cw = min(1 << lcw, TW), ch = min(1 << rs, TH);")
    _once(kern, "bool it_ok = lg <= ilog2c(kWgCells), it_in = true;")
    _once(kern, "const int cell_x0 = tx0 + ((cell & ((1 << lgx) - 1)) << lcw), cell_y0 = ty0 + ((cell >> lgx) << rs);")
    _once(kern, "if (it_ok && cell_x0 < W && cell_y0 < dim_y) {")
    _once(kern, "const int ly = min(CZ ? ((cell_y0 >> rs) << 1) : (cell_y0 >> rs), lh - 1);")
    _once(kern, "const int lx = min(CZ ? ((cell_x0 >> rs) & ~1) : (cell_x0 >> rs), lw - 1);")
    _once(kern, "const int py = clampi(ly - (oy12 >> rs), 0, lh - 1), px = clampi(lx - (ox12 >> rs), 0, lw - 1);")
    _once(kern, "const int dxe = CZ ? (dx & ~1) : dx;")
    _once(kern, "const int x_lo = cell_x0 + dxe, x_hi = x_lo + cw - VEC, y_lo = cell_y0 + dy, y_hi = y_lo + ch - ROWS;")
    _once(kern, "const int bx_lo = (x_lo + kExtX) * SZ, bx_hi = (x_hi + kExtX) * SZ, by_lo = y_lo + kExtY, by_hi = y_hi + kExtY;")
    _once(kern, "bool ok = bx_lo >= 0 && bx_hi + 4 * NDW + 4 <= 0xFFFF && by_lo >= 0 && by_hi + ROWS <= 0xFFFF;")
    _once(kern, "if (CZ) ok = ok && x_hi + VEC <= W - 2;")
    _once(kern, "it_in = it_in && x_lo >= 1 && x_hi + VEC - 1 + CZ <= W - 2 && y_lo >= 1 && y_hi + ROWS - 1 <= dim_y - 2;")
    _once(kern, "if (ok) {\n                    lo = pk_mm_u16<false>(lo, ((uint32_t)by_lo << 16) | (uint32_t)bx_lo);")
    _once(kern, "if (need_a) w.x = item((int)roundf((float)ox12 * s12t), CZ ? (int)roundf((float)oy12 * s12t * 0.5f) : (int)roundf((float)oy12 * s12t), lo_a, hi_a);")
    _once(kern, "if (need_b) w.y = item(-(int)roundf((float)ox21 * s21t), -(CZ ? (int)roundf((float)oy21 * s21t * 0.5f) : (int)roundf((float)oy21 * s21t)), lo_b, hi_b);")
    body = kern[kern.index("void warp_wg_body("):kern.index("static_assert(sizeof(Geom) + sizeof(WarpBatchArgs)")]
    _once(body, "constexpr bool need_a = MODE != 1, need_b = MODE != 0;")
    _once(kern, "a.s12v[i] = p.ts[i]; a.s21v[i] = 1.0f - p.ts[i];")
    _once(kern, "const bool present = valid_mask != 0, full = __builtin_amdgcn_ballot_w64(lane_valid && cx0 + VEC <= W) == ~0ull;")
    _once(kern, "const bool lane_valid = trow < (chroma ? uv_tiles : y_tiles) && cx0 < g.W && rg < (chroma ? uv_groups : y_groups);")
    _once(kern, "sh.state[wave] = !present ? 2 : full ? 1 : 0; sh.item[wave] = (ok_all ? 1 : 0) | (in_all ? 2 : 0);")
    _once(kern, "wg_ok = wg_ok && sh.state[w] != 0 && (sh.item[w] & 1) != 0;")
    _once(kern, "wg_in = wg_in && (sh.item[w] & 2) != 0;")
    _once(kern, "int cmin_a = 0, ymin_a = 0, C_a = 1, R_a = 0, cmin_b = 0, ymin_b = 0, C_b = 1, R_b = 0;")
    for s in "ab":
        _once(kern, f"cmin_{s} = (int)(l{s} & 0xFFFFu) >> 4; ymin_{s} = (int)(l{s} >> 16);")
        _once(kern, f"C_{s} = (int)(((h{s} & 0xFFFCu) + 4u * NDW + 3u) >> 4) - cmin_{s} + 1; R_{s} = (int)(h{s} >> 16) + ROWS - 1 - ymin_{s} + 1;")
    _once(kern, "wg_ok = ((R_a * C_a + 63) & ~63) <= CHUNKS && ((R_b * C_b + 63) & ~63) <= CHUNKS && C_a <= 64 && C_b <= 64;")
    _once(body, "wg_ok = __builtin_amdgcn_readfirstlane((int)wg_ok) != 0;\n    // this lane's own word and cell")
    _once(body, "if (!wg_ok) {   // workgroup-uniform: no barrier follows\n        if (runs_ok && wg_in && full) {")
    _once(body, "const bool zone = x0 < 1 || (!CZ && x0 + VEC - 1 > W - 2);")      # stage(): the chunks of an edge window gathered element by element
    _once(kern, "atomicAdd(counters + kCounterWarp + (wg_ok ? 0 : (runs_ok && wg_in && full) ? 1 : 2), 1u);")
    _once(kern, "const int yb = (y_tiles + NW - 1) / NW, ub = (uv_tiles + NW - 1) / NW;")
    _once(kern, "if (brow >= (chroma ? ub : yb)) return;")


def test_geometry_is_the_oracles():
    from oracle import oracle
    for c in M.CASES:
        g, o = M.geometry(c), oracle.make_geom(c.hdr, c.H, c.W, c.in_stride, c.out_stride, c.max_res)
        assert tuple(g) == (o.hdr, o.H, o.W, o.in_stride, o.out_stride, o.rs, o.lw, o.lh), c.name


def test_model_on_known_shapes():
    ts = (0.0, 0.1988, 0.5, 0.7992, 0.998)
    c = M._c("x", 1, 2160, 3840, 270, 4, (5,), ts=ts)
    g = M.geometry(c)
    assert [ln.label for ln in M.launches(c, 2)] == ["staged.u16.rs3"] and M.defers_planes(g, 4) and not M.defers_planes(g, 2)
    assert M.labels(c._replace(path="period"), 2) == {"staged.u16.rs3.planes", "plane.u16.rs3"}
    assert M.labels(c._replace(path="period", src_align=(0, 8)), 2) == {"staged.u16.rs3.planes", "plane.u16.rs3", "plane.fallback"}
    assert M.labels(c._replace(path="period"), 3) == {"generic.u16.aligned"}
    # the 3060 workgroups of a 2160p HDR member: uniform slow / fast motion, and the "half and half" field of test_fused_fullsize_gpu
    for kind, want in (("uniform:9:-5", (3026, 0, 34)), ("uniform:230:-140", (0, 2236, 824)), ("half", (1530, 960, 570))):
        assert M.wg_member(g, M.flow_field(kind, g), ts, 2)[1] == want, kind
    cl, cnt, deep = M.wg_member(g, M.flow_field("uniform:60:40", g), M.DEEP, 2)
    assert cnt == (3026, 0, 34) and deep == 60
    assert all(cs != {"staged.interior"} for p in ("y", "uv") for row in (cl[p][0], cl[p][-1]) for cs in row)
    # one context: 1080p SDR takes 8-byte threads with one output each, 2160p HDR all outputs per thread; a 4320p context's fused period is staged
    assert M.labels(M._c("x", 0, 1080, 1920, 270, 1, (5,), path="single"), 2) == {"fast.u8.vb8.g4.dw.one.w4"}
    assert M.labels(M._c("x", 1, 2160, 3840, 270, 1, (5,), path="single"), 2) == {"fast.u16.vb16.g8.dw.all.w4"}
    assert M.labels(M._c("x", 1, 4320, 7680, 270, 1, (5,), path="single"), 2) == {"staged.u16.rs4"}
    assert M.labels(M._c("x", 1, 4320, 7680, 270, 1, (1,), path="single"), 2) == {"fast.u16.vb16.g8.dw.all.w16"}
    # the batch sizes at which 1080p changes shape: 11 members of 1080p HDR at rs 3 are staged, 10 are not
    assert M.labels(M._c("x", 1, 1080, 1920, 135, 11), 2) == {"staged.u16.rs3"}
    assert M.labels(M._c("x", 1, 1080, 1920, 135, 10), 2) == {"fast.u16.vb16.g8.dw.one.w4"}
    assert M.labels(M._c("x", 0, 1080, 1920, 270, 16), 2) == {"fast.u8.vb8.g4.dw.all.w4"}
    assert M.labels(M._c("x", 0, 1080, 1920, 270, 32), 0) == {"fast.u8.vb8.g4.dw.all.w4", "split"}
    # an output that is not 8-byte aligned sends the whole batch member by member to the generic kernel
    assert M.labels(M._c("x", 0, 1080, 1920, 270, 4, out=(0, 2)), 2) == {"fast.u8.vb8.g4.dw.one.w4", "generic.u8.unaligned"}


def compiled_instantiations():
    from hopperrender_amd import build
    nm = "nm" if subprocess.run(["which", "nm"], capture_output=True).returncode == 0 else "/opt/rocm/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-C", build.LIB_FLOW], capture_output=True, text=True, check=True).stdout
    return set(re.findall(r"__device_stub__((?:warp_fast|warp_wg|warp|copy)_kernel<[^>]*>)\(", out))


def sweep_labels():
    """Every label the model produces over sizes 180p .. 4320p, max_res 67 .. 4320, strides, alignments, 1 .. 32 members, 1 .. 6 outputs."""
    sizes = SWEEP_SIZES
    seen = {m: set() for m in (0, 1, 2, 3)}
    for hdr in (0, 1):
        for H, W in sizes:
            for mr in (67, 135, 270, 540, 1080, 4320):
                for si, so in ((0, 0), (W + 2, 0), (0, W + 8), (W + 64, W + 64)):
                    for src, out in ((0, 0), (2, 0), (4, 0), (0, 8), (0, 2)):
                        for n, outs, path in ((1, 1, "single1"), (1, 2, "single"), (1, 6, "single"), (1, 1, "copy"), (2, 3, "batch"), (11, 1, "batch"),
                                              (16, 6, "batch"), (17, 2, "batch"), (32, 5, "batch"), (11, 2, "period"), (16, 6, "period")):
                            c = M._c("s", hdr, H, W, mr, n, (outs,), path=path, si=si, so=so, src=(src,), out=(out,))
                            for mode in seen:
                                seen[mode] |= M.labels(c, mode)
    for mode in (0, 1, 2):      # a member of a plane-building launch whose frames are not 16-byte aligned
        seen[mode] |= M.labels(M._c("s", 1, 2160, 3840, 270, 4, (2,), path="period", src=(0, 4)), mode)
    return seen


def test_compiled_instantiations_are_the_models(native_lib):
    """nm on the built library: every warp_fast / warp_wg / warp / copy kernel instantiation is one the model can launch, or is listed as
    unreachable with its reason; and a sweep of the model produces no label outside the declared sets."""
    compiled = compiled_instantiations()
    assert len(compiled) == 72 + 6 + 4 + 4, len(compiled)
    by_mode = {mode: {M.instantiation(lb, mode) for lb in M.FAST_LABELS | M.STAGED_LABELS} for mode in (0, 1, 2)}
    launchable = set().union(*by_mode.values()) | {M.instantiation(lb, 0) for lb in M.GENERIC_LABELS | M.COPY_LABELS}
    assert launchable.isdisjoint(M.UNREACHABLE) and all(M.UNREACHABLE.values())
    assert compiled == launchable | set(M.UNREACHABLE), (sorted(compiled - launchable - set(M.UNREACHABLE)), sorted((launchable | set(M.UNREACHABLE)) - compiled))
    assert len(M.UNREACHABLE) == 6
    seen = sweep_labels()
    for mode in (0, 1, 2):
        assert seen[mode] == M.MODE_LABELS | M.COPY_LABELS, (mode, sorted(seen[mode] ^ (M.MODE_LABELS | M.COPY_LABELS)))
    assert seen[3] == M.GENERIC_LABELS | M.COPY_LABELS, sorted(seen[3])


def test_matrix_reaches_every_label_in_every_mode():
    names = [c.name for c in M.CASES]
    assert len(set(names)) == len(names) and all(c.path in M.PATHS for c in M.CASES)
    for mode in (0, 1, 2):
        seen = set().union(*(M.labels(c, mode) for c in M.CASES if mode in c.modes and c.path != "copy"))
        assert seen == M.MODE_LABELS, (mode, sorted(M.MODE_LABELS - seen), sorted(seen - M.MODE_LABELS))
    for mode in (3, 4, 5, 6):
        seen = set().union(*(M.labels(c, mode) for c in M.CASES if mode in c.modes))
        assert seen == M.GENERIC_LABELS, (mode, sorted(seen))
    assert set().union(*(M.labels(c, 2) for c in M.CASES if c.path == "copy")) == M.COPY_LABELS
    # every family once through the real chain
    period = set().union(*(M.labels(c, m) for c in M.CASES if c.path == "period" for m in c.modes))
    assert {lb.split(".")[0] for lb in period} >= {"fast", "staged", "generic", "plane"}
    # blend scalars 0 and 1 exactly, member-specific counts of 1 to 6
    assert all({0.0, 1.0} <= set(c.ts) or c.ts == M.DEEP for c in M.CASES)
    assert {m.n_out for c in M.CASES if c.path == "batch" and len(set(c.outs)) > 1 for m in M.members(c)} == set(range(1, 7))


def test_matrix_reaches_every_workgroup_class():
    """Every (element type, plane, class) pair in some staged case; cells smaller than, equal to and taller than the 32-row tile; a staged edge
    window deeper than 56 elements in the mirror zone for both element types; every staged case has all three counters above zero somewhere."""
    pairs, cells, deep, totals = set(), set(), {}, [0, 0, 0]
    for c in M.CASES:
        g = M.geometry(c)
        for mode in c.modes:
            if mode > 2 or c.path == "period" or not any(ln.staged for ln in M.launches(c, mode)):
                continue
            cnt, seen, d = M.case_counts(c, mode)
            pairs |= seen
            cells.add((M.ename(g), "smaller" if g.rs < 5 else "equal" if g.rs == 5 else "taller"))
            deep[M.ename(g)] = max(deep.get(M.ename(g), 0), d if c.ts == M.DEEP else 0)
            totals = [a + b for a, b in zip(totals, cnt)]
            per_member = M.wg_blocks_per_member(g, 0) // max(-(-(g.H // 2) // 64), (-(-g.H // 32) + 1) // 2)     # = 3 x tile columns
            assert sum(cnt) > 0 and per_member == 3 * -(-g.W // (16 * 16 // M.esize(g)))
    assert pairs == M.required_pairs(), (sorted(M.required_pairs() - pairs), sorted(pairs - M.required_pairs()))
    assert cells == {(e, k) for e in ("u8", "u16") for k in ("smaller", "equal", "taller")}
    assert deep["u8"] >= 56 and deep["u16"] >= 56 and max(deep.values()) <= M.EXT_X, deep
    assert all(t > 1000 for t in totals), totals


def test_matrix_reaches_every_plane_variant():
    seen = set()
    for c in M.CASES:
        if c.path != "period":
            continue
        g = M.geometry(c)
        for mode in c.modes:
            lns = M.launches(c, mode)
            if any(ln.label.endswith(".planes") for ln in lns):
                assert M.defers_planes(g, c.members) and all(0 < len(ln.planes) < ln.count for ln in lns), c.name
                seen |= {(lb, mode) for lb in M.labels(c, mode) if lb.startswith("plane.")}
            else:
                assert not M.defers_planes(g, c.members) or mode > 2, c.name
    assert seen == {(lb, m) for lb in M.EXTRA_LABELS - {"split"} for m in (0, 1, 2)}, sorted(seen)


def test_roundf_and_float32_scalars():
    """The kernel's arithmetic: float32 products, halves away from zero; s21 = 1.0f - t in float32."""
    assert list(M._roundf(np.array([0.5, -0.5, 1.5, -1.5, 2.4999998, -2.5], np.float32))) == [1, -1, 2, -2, 2, -3]
    t = np.float32(0.7992)
    assert float(np.float32(1.0) - t) != 1.0 - 0.7992
    assert int(M._roundf(np.float32(-5) * np.float32(0.5) * np.float32(1.0))[()]) == -3
