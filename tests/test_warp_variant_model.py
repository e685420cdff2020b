"""CPU: the model of the warp's launch selection and of the staged kernel's workgroup bodies (tests/warp_variant_model.py) is pinned to the
sources, the compiled instantiations are exactly the ones the model can launch plus a stated list of unreachable ones, and the matrix that
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


def test_constants_equal_the_sources():
    kern, kern_h = _src("hf_kernels.hip"), _src("hf_kernels.h")
    assert _ints(kern, r"constexpr int kWarpTX = (\d+), kWarpTY = (\d+);") == (M.WARP_TX, M.WARP_TY)
    assert _ints(kern, r"constexpr int kWarpWavesSmall = (\d+), kWarpWavesLarge = (\d+);") == (M.WAVES_SMALL, M.WAVES_LARGE)
    assert _ints(kern, r"constexpr int kWgWaves = (\d+), kWgRows = (\d+), kWgChunksPerWave = (\d+);") == (M.WG_WAVES, M.WG_ROWS, M.WG_CHUNKS_PER_WAVE)
    a, b = _ints(kern, r"constexpr long kWgMinWaves = (\d+) \* (\d+);")
    assert a * b == M.WG_MIN_WAVES
    assert _ints(kern, r"constexpr int kExtX = (\d+), kExtY = (\d+);") == (M.EXT_X, M.EXT_Y)
    assert _ints(kern, r"constexpr int kWgCells = (\d+);") == (M.WG_CELLS,)
    assert _ints(kern_h, r"constexpr int kMaxWarpBatch = (\d+);") == (M.MAX_WARP_BATCH,)
    assert _ints(kern_h, r"constexpr int kMaxWarpOutputs = (\d+);") == (M.MAX_WARP_OUTPUTS,)
    assert _ints(kern_h, r"constexpr int kMaxFlowBatch = (\d+);") == (M.MAX_FLOW_BATCH,)
    assert _ints(kern, r"constexpr int VEC = 16 / \(int\)sizeof\(E\), NDW = (\d+), CHUNKS = wg_chunks\(NW \* ROWS / 2\), SZ") == (M.NDW,)
    _once(kern, "const int rows = 2;  // rows per thread")
    _once(kern, "constexpr int wg_chunks(int nw) { return nw * kWgChunksPerWave; }")
    _once(kern, "constexpr int WR = kWgRows, NW = kWgWaves * 2 / WR;")
    assert M.SMALL_FRAME_BYTES == 1920 * 1088 and M.ROUNDS == 4 * 8192


def test_launch_comparisons_equal_the_sources():
    kern, kern_h, batch, calc = _src("hf_kernels.hip"), _src("hf_kernels.h"), _src("hf_batch.hip"), _src("hf_calc.hip")
    # the two 1920 x 1088 bounds and the "* 2" one
    _once(kern, "return (size_t)g.W * g.H * sizeof(E) <= (size_t)1920 * 1088;")
    _once(kern, "if (cell < VEC || (size_t)g.W * g.H * esz <= (size_t)1920 * 1088) return false;")
    _once(kern, "const bool small_frame = (size_t)g.W * g.H * sizeof(E) <= (size_t)1920 * 1088 * 2;")
    assert len(re.findall(r"1920 \* 1088", re.sub(r"//.*", "", kern))) == 3
    # warp_fast_shape
    _once(kern, "const int group = cell < VEC ? cell : VEC;", 2)
    _once(kern, "bool fast = mode >= 0 && mode <= 2 && (g.in_stride % 2) == 0 && (g.out_stride % VEC) == 0 &&")
    _once(kern, "g.W >= 2 * VEC && group >= 2 && VEC % group == 0 && VEC / group <= 4;")
    _once(kern, "dw = ((size_t)g.in_stride * sizeof(E)) % 4 == 0 && ((size_t)g.W * sizeof(E)) % 4 == 0 && ((size_t)g.H * g.in_stride * sizeof(E)) % 4 == 0;")
    _once(kern, "const bool sane = a.white != a.black && a.white != 0.0f && a.white == a.white && a.black == a.black;")
    _once(kern, "fast = fast && a.mode == mode && (mode != 2 || sane) && a.flow_xy && a.n_out >= 1 && a.n_out <= kMaxWarpOutputs;")
    _once(kern, "fast = fast && a.s12v[i] >= 0.0f && a.s12v[i] <= 1.0f && (((uintptr_t)a.outv[i]) & (VB - 1)) == 0;")
    _once(kern, "dw = dw && (((uintptr_t)a.frame12 | (uintptr_t)a.frame21) & 3) == 0;")
    # launch_warp_fast: outputs per thread, the staged condition, waves per workgroup
    _once(kern, "const int y_groups = (g.H + rows - 1) / rows, uv_groups = ((g.H >> 1) + rows - 1) / rows;")
    _once(kern, "const int n_tiles = wpr * ((y_groups + kWarpTY - 1) / kWarpTY + (uv_groups + kWarpTY - 1) / kWarpTY);")
    _once(kern, "const int out_chunk = small_frame && (long)n_tiles * b.n < 4 * 8192 ? 1 : kMaxWarpOutputs;")
    _once(kern, "const int n_chunks = (max_out + out_chunk - 1) / out_chunk;")
    _once(kern, "if constexpr (VB == 16) if (group == VEC && dw && out_chunk > 1 && max_out >= 2 && (long)n_tiles * b.n >= kWgMinWaves &&\n"
                "                                fastdiv_exact((uint64_t)nb_max * b.n + 8, nb_max)) {")
    _once(kern_h, "inline bool fastdiv_exact(uint64_t max_u, uint32_t d) { return max_u * d < (1ull << 32); }")
    _once(kern, "const uint32_t nb_max = (uint32_t)wg_blocks_per_member(wpr, (y_tiles_ + NW - 1) / NW, (uv_tiles_ + NW - 1) / NW, plane_blocks);")
    _once(kern, "const int plane_blocks = ((g.lw >> 2) * (2 * NW * kWarpTY * WR) + 64 * NW - 1) / (64 * NW);")
    _once(kern, "return (wpr * 3 + plane_blocks) * wg_super_rows(yb, ub);")
    _once(kern, "int wg_super_rows(int yb, int ub) { return ub > (yb + 1) / 2 ? ub : (yb + 1) / 2; }")
    _once(kern, "const int wpb = out_chunk > 1 && (long)n_tiles * n_chunks * b.n >= 4 * 8192 ? warp_max_waves(sizeof(E), group, VB) : kWarpWavesSmall;")
    _once(kern, "return vb == 16 && group * (int)elem == 16 ? kWarpWavesLarge : kWarpWavesSmall; }")
    # planes: who gets one, which task builds it, when a batch defers
    _once(kern, "bool emit = pl && plane_emission_geometry(g, *pl);")
    _once(kern, "if (!emit || (((uintptr_t)bb.s[m].frame21) & 15) != 0) bb.s[m].plane21 = nullptr;")
    _once(kern, "return g.rs >= 3 && g.rs <= 4 && pl.rs == g.rs && (lw << g.rs) == g.W && lw == g.lw && (lw & 3) == 0 && pl.mx <= lw && (pl.mx & 3) == 0 &&\n"
                "           (pl.lwp & 3) == 0 && ((size_t)g.in_stride * esz) % 16 == 0 && ((size_t)g.H * g.in_stride * esz) % 16 == 0 && (g.H & 1) == 0;")
    _once(kern, "if (sizeof(E) == 2 && g.rs == 3) plane_fast_task<E, 3, 1>(")
    _once(kern, "else plane_fast_task<E, 4, 1>(")
    _once(kern, "return n_tiles * per_launch >= kWgMinWaves && g.H == (g.lh << g.rs) && plane_emission_geometry(g, pl);")
    _once(kern, "const int per_launch = n_members < kMaxWarpBatch ? n_members : kMaxWarpBatch;")
    _once(batch, "b->defer_planes = !l->dual() && !(l->cfg.flags & HF_FLAG_BATCH_EAGER_PLANES) && hf::warp_period_can_build_planes(l->g, l->pl, n);")
    _once(batch, "if (n_out && calculate_flow && b->defer_planes && mode >= 0 && mode <= 2) {")
    flow = _src("hf_flow.hip")
    _once(flow, "const int reach = (max_iterations + 1) * 64 + 8;")
    _once(flow, "pl.mx = (((reach >> g.rs) + 2 + 3) / 4) * 4;")
    _once(flow, "pl.lwp = ((g.lw + 2 * pl.mx + 4 + 31) / 32) * 32;")
    _once(_src("hf_context.hip"), "const int max_iters = ilog2(ws0);")
    # launch_warp_fast_any, launch_warp_t, launch_warp_periods, launch_copy_t, one context's period
    _once(kern, "if (small && launch_warp_fast<E, 8>(g, b, stream, ev0, ev1)) return true;")
    _once(kern, "return launch_warp_fast<E, 16>(g, b, stream, ev0, ev1, pl, planes_built);")
    _once(kern, "return (warp_small_frame<E>(g) && warp_fast_shape<E, 8>(g, b, dw)) || warp_fast_shape<E, 16>(g, b, dw);")
    _once(kern, "const bool aligned = (g.out_stride % VEC) == 0 && (((uintptr_t)a.out) & 15) == 0;")
    _once(kern, "const bool aligned = (g.in_stride % VEC) == 0 && (g.out_stride % VEC) == 0 &&\n"
                "                         (((uintptr_t)src | (uintptr_t)out) & 15) == 0;")
    _once(kern, "for (int first = 0; first < n; first += kMaxWarpBatch) {", 2)
    _once(kern, "b.n = n - first < kMaxWarpBatch ? n - first : kMaxWarpBatch;")
    _once(kern, "if (n < 1 || n > kMaxFlowBatch) return false;")
    _once(calc, "const bool fuse = n_out >= 2 && !(c->cfg.flags & HF_FLAG_NO_FUSED_WARP);")
    # launch_warp_t passes no counters: a single context's one-output launch is not counted (and is never staged: max_out >= 2)
    _once(kern, "b.n = 1; b.counters = nullptr; b.s[0] = a;")


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
    sizes = [(180, 320), (360, 640), (720, 1280), (1080, 1920), (1088, 1536), (1088, 2816), (1440, 2560), (2160, 3840), (4320, 7680), (722, 1282)]
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
