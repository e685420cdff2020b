// hopperrender_amd/csrc/hf_launch_plan.h -- which kernel a launch runs, and with what grid: the ONE place the selection lives.
//
// Host-only and HIP-free (plain g++ -std=c++17, no ROCm include path): the plain structs the decisions read, their constants and pure
// plan functions -- same inputs, same result; pointers are looked at for null-ness and alignment bits only, never dereferenced; no
// allocation, no strings, no I/O: a plan is a stack value on the launch path.  The launchers of hf_kernels.hip / hf_flow.hip turn a plan
// into template arguments; tests/launch_plan_probe.cpp exposes the same functions to tests/test_warp_variant_model.py and
// tests/test_chain_variant_model.py, which compare them with the Python models over whole grids of shapes.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define HF_PLAN_HD __host__ __device__ __forceinline__
#else
#define HF_PLAN_HD inline
#endif

namespace hf {

// Geometry shared by all kernels (reference ctor, opticalFlowCalcSDR.cpp:206-222).
struct Geom {
    int hdr;             // 0: uint8 elements, 1: uint16 elements
    int H, W;            // full-resolution luma size
    int in_stride;       // elements
    int out_stride;      // elements
    int rs;              // resolution scalar
    int lw, lh;          // low-res grid
};

// Division of a wave-uniform index by a launch constant on the SCALAR unit: u / d == mulhi(u, ceil(2^32 / d)) while u * d < 2^32.
// Left to the compiler a uniform u / d is ~25 VECTOR instructions (v_rcp_iflag_f32, v_mul_hi_u32 ...) and every workgroup of the
// batched kernels decodes its unit index with three of them before it can start.  Every launcher builds its dividers with the largest
// index the launch decodes (make_fastdiv(d, max_u)): where the multiply-high form would not be exact -- grids far beyond 8K -- the
// divider carries magic == 0 and the kernel takes the plain division (a uniform branch; tests/test_fastdiv_math.py).
struct FastDiv { uint32_t d, magic; };
inline bool fastdiv_exact(uint64_t max_u, uint32_t d) { return max_u * d < (1ull << 32); }
inline FastDiv make_fastdiv(uint32_t d, uint64_t max_u) {
    return FastDiv{d, d > 1 && fastdiv_exact(max_u, d) ? (uint32_t)(((1ull << 32) + d - 1) / d) : 0u};
}

constexpr int kMaxFlowBatch = 32;      // contexts per hf_batch (FlowBatch, hf_kernels.h)
constexpr int kMaxWarpBatch = 16;      // members per fused warp launch (its per-member arguments are 168 bytes; a launch carries 4 KB)
constexpr int kMaxWarpOutputs = 6;     // outputs of one source period at 24 -> 120 fps (HopperRender.cpp:944-948)

// Phase-plane layout of a frame (hf_flow.hip).  ONE plane of 4-byte elements, one element per grid column, per pair of
// luma phases and per full-resolution luma row:
//     PP[y][ph2][j] = Y[y][x] | Y[y][x + 1] << 8 | U[y >> 1][x & ~1] << 16 | V[y >> 1][x & ~1] << 24      (top 8 bits each)
//     x = (j << rs) + 2 * ph2, mirrored once at the frame edge; j in [-mx, lwp - mx).
// A candidate sample of `PX` consecutive grid pixels is PX consecutive elements: one DWORD-ALIGNED 16-byte load (luma and
// chroma together), whatever the candidate offset is.  (Round 1 kept byte planes for luma and 2-byte planes for chroma:
// their 4- and 8-byte strips started at arbitrary byte offsets, and a vector load that is not dword-aligned takes a 3-4x
// slower path through the texture addresser -- the chain kernels ran at 78 % TA busy.)
struct PhaseLayout {
    int rs, nph, nph2;       // 2^rs luma phases, max(1, nph/2) phase pairs
    int mx;                  // left margin in grid units (covers every reachable offset, reflection baked in)
    int lwp;                 // row pitch in elements (multiple of 4)
    size_t bytes;            // H * nph2 * lwp * 4
};
inline PhaseLayout make_phase_layout(const Geom& g, int max_iterations) {
    PhaseLayout pl{};
    pl.rs = g.rs;
    pl.nph = 1 << g.rs;
    pl.nph2 = pl.nph > 1 ? pl.nph / 2 : 1;
    const int reach = (max_iterations + 1) * 64 + 8;   // |offset| <= iterations * (R/2)^2, + one candidate, R <= 16
    pl.mx = (((reach >> g.rs) + 2 + 3) / 4) * 4;        // multiple of 4: margin groups line up with the 4-column groups
    pl.lwp = ((g.lw + 2 * pl.mx + 4 + 31) / 32) * 32;   // a strip may start at column lw + mx; rows start on a 128-byte line
    pl.bytes = (size_t)g.H * pl.nph2 * pl.lwp * sizeof(uint32_t);
    return pl;
}

// Offsets of one refinement level: one (x, y) pair per window of size `window`.
struct FlowLevel {
    int window, log2w;       // window size (power of two >= 2)
    int nwx, nwy;            // windows per grid row / column
    int16_t* tx;             // [nwy][nwx] X offsets after this level (nullptr: level does not exist = all zero)
    int16_t* ty;             // [nwy][nwx] Y offsets after this level
};

// All outputs of one source period of one context (launch_warp_periods, hf_kernels.h).
struct WarpPeriod {
    const void* frame12;
    const void* frame21;
    const int16_t* flow;
    const uint32_t* flow_xy;
    int n_out;
    void* outs[kMaxWarpOutputs];
    float ts[kMaxWarpOutputs];
    float black, white;      // already scaled for HDR
    uint32_t* plane21 = nullptr;   // deferred phase plane: build the full plane of frame21 here if the launch can (see below)
    uint32_t* counters = nullptr;  // diagnostic counters of the launch (member 0's are used), nullptr: none
};

// ------------------------------------------------------------------------------------------
// warp: constants
// ------------------------------------------------------------------------------------------
// Wave tile = kWarpTX lanes x kWarpTY row groups: (16 x VEC) elements wide, (4 x ROWS) rows high -- at 2160p HDR 128 pixels
// x 8 rows = 16 flow cells of one cell row.  (Round 1 used 64 lanes along x: 7.5 tiles per 3840-pixel row, of which the
// first and the last contain lanes whose runs reach into the mirror zone of warpFrameKernelSDR.h:12-20, so 27 % of all
// waves executed the per-element edge path next to the run path -- that, not the interior code, was most of the
// 1,940 VALU instructions per wave.  With 128-pixel tiles 2 of 30 tiles per row are edge tiles.)
constexpr int kWarpTX = 16, kWarpTY = 4;
// Waves (= consecutive wave tiles of a tile row) per workgroup of warp_fast_kernel, chosen per launch: 4, or 16 for the batched periods of
// large frames.  Measured on MI355X, 2160p HDR pipeline (32 pair streams = 2 batches of 16), k frames/s: 67.0 / 67.6 / 68.9 / 68.7 /
// 67.8 / 68.8 / 70.0 with 4 / 5 / 6 / 8 / 10 / 15 / 16 waves (+2.6 % with one batch stream); a single period is 46 us with 4
// and 52 us with 16 (760 workgroups for 256 CUs), and the short one-output waves of frames up to 1080p lose 8 % with 16.
constexpr int kWarpWavesSmall = 4, kWarpWavesLarge = 16;
// (only the one-flow-cell-per-thread instances are compiled for 1,024-thread workgroups = at most 128 VGPRs: the others need more)
constexpr int warp_max_waves(size_t elem, int group, int vb) { return vb == 16 && group * (int)elem == 16 ? kWarpWavesLarge : kWarpWavesSmall; }
// rows per thread of warp_fast_kernel (divides the 2^rs rows of a flow cell); measured on MI355X, 2160p HDR blend: 1 row 25.9 us, 2 rows
// 24.3 us, 4 rows 30.2 us (re-measured with the final kernel, fused period HBM-cold: 2 rows 51.1 us, 4 rows 59.3 us -- halving the
// per-element scalar work does not pay for halving the number of waves)
constexpr int kWarpFastRows = 2;
// Frames up to 1080p 8-bit take 8 bytes per thread and row (twice the waves; 1080p SDR, 5-output period: 18.9 us against 26.8 us with
// 16-byte threads, in a batch of 16: 114.3 k frames/s against 100.2 k); up to twice that, one output per thread unless the launch
// has rounds of waves to spare.
constexpr size_t kSmallFrameBytes = (size_t)1920 * 1088;
constexpr long kWarpRounds = 4 * 8192;            // "rounds of waves to spare": >= 4 rounds of 8,192 resident waves
// Shape of the staged kernel warp_wg_kernel (all measured on the 2160p HDR pipeline, 2 batch streams of 16, k frames/s -- DESIGN.md appendix C):
//   waves (= vertically stacked wave tiles) per workgroup: 68.8-70.0 without staging, 71.9-72.5 / 72.9-73.4 / 73.9-74.1 / 66.7-67.8 / 61.3
//   with 2 / 3 / 4 / 6 / 16 waves;  rows per thread: 2 (4 rows = half the waves: alone 672 vs 663 us per 16 members, pipeline 69.4 vs
//   72.4: the other stream's chain waits longer for the fewer, longer waves);  window budget 160 / 176 / 192 / 224 / 256 chunks per wave:
//   192 best (smaller: more fallbacks; larger: one workgroup per CU less)
constexpr int kWgWaves = 4, kWgRows = 2, kWgChunksPerWave = 192;
constexpr long kWgMinWaves = 4 * 8192;            // the staged kernel only for launches of several rounds of waves (batched periods): ONE
                                                  // member's period alone is 12 % slower that way (two barriers and a serial prologue per
                                                  // workgroup with nothing to overlap them), so single launches keep the global path
constexpr int wg_chunks(int nw) { return nw * kWgChunksPerWave; }   // 16-byte chunks per source window (12 KB for 4 waves)

// The grid of warp_wg_kernel (the kernel decodes it with the same two functions): per member, super rows of
// (3 tile columns' worth of warp workgroups + plane_blocks plane-building ones).
HF_PLAN_HD int wg_super_rows(int yb, int ub) { return ub > (yb + 1) / 2 ? ub : (yb + 1) / 2; }
HF_PLAN_HD int wg_blocks_per_member(int wpr, int yb, int ub, int plane_blocks) {
    return (wpr * 3 + plane_blocks) * wg_super_rows(yb, ub);
}

// ------------------------------------------------------------------------------------------
// warp: predicates
// ------------------------------------------------------------------------------------------
inline size_t elem_size(const Geom& g) { return g.hdr ? 2 : 1; }
inline bool small_frame(const Geom& g, int times = 1) { return (size_t)g.W * g.H * elem_size(g) <= kSmallFrameBytes * times; }
// a thread of vb bytes per row holds whole flow cells (a run group = the cell where it is narrower)
inline int warp_group(const Geom& g, int vb) { const int vec = vb / (int)elem_size(g), cell = 1 << g.rs; return cell < vec ? cell : vec; }
inline bool one_cell_per_thread(const Geom& g, int vb) { return warp_group(g, vb) == vb / (int)elem_size(g); }
inline int warp_tiles_per_row(const Geom& g, int vb) { const int tw = kWarpTX * (vb / (int)elem_size(g)); return (g.W + tw - 1) / tw; }
inline int warp_tile_rows(int dim_y, int rows) { return ((dim_y + rows - 1) / rows + kWarpTY - 1) / kWarpTY; }
inline long warp_n_tiles(const Geom& g, int vb) {   // wave tiles of a frame, both planes, with kWarpFastRows (== kWgRows) rows per thread
    return (long)warp_tiles_per_row(g, vb) * (warp_tile_rows(g.H, kWarpFastRows) + warp_tile_rows(g.H >> 1, kWarpFastRows));
}
inline bool staged_rounds(long n_tiles, int members) { return n_tiles * members >= kWgMinWaves; }
// Does the fast plane build (hf_phase_plane.h plane_fast_task) apply to frames of this geometry?  Whole grid columns (W == lw << rs), tasks
// of 4 columns, margins one reflection deep at most and in whole tasks, 16-byte task loads and stores, an instantiated rs, whole chroma
// rows.  The geometry part of hf_flow.hip launch_prep_fast's answer: the 16-byte alignment of each frame's base is the launch's own test.
inline bool plane_fast_geometry(const Geom& g, const PhaseLayout& pl) {
    const int lw = g.W >> g.rs;
    return (lw << g.rs) == g.W && lw == g.lw && (lw & 3) == 0 && pl.mx <= lw && (pl.mx & 3) == 0 && (pl.lwp & 3) == 0 &&
           ((size_t)g.in_stride * elem_size(g)) % 16 == 0 && g.rs <= 4 && (g.H & 1) == 0;
}
// Can the staged kernel build the phase planes of its members' frame21 (emit_plane_rows)?  The geometry part of the answer: the two
// instantiations of its tasks, a chroma plane that starts on a 16-byte boundary, and the conditions of the fast plane build.
inline bool plane_emission_geometry(const Geom& g, const PhaseLayout& pl) {
    return g.rs >= 3 && g.rs <= 4 && pl.rs == g.rs && ((size_t)g.H * g.in_stride * elem_size(g)) % 16 == 0 && plane_fast_geometry(g, pl);
}

// Static part of the deferred-plane decision for a batch of n_members contexts of geometry g (hf_batch decides once whether it defers
// its planes): one flow cell per 16-byte thread, no 8-byte threads.  (Frames that take warp_fast_kernel -- 1080p and smaller -- keep their
// eager planes: plane-building workgroups in THAT launch were built and measured in round 5, bit-exact and 2 % slower than the stand-alone
// plane kernel there: 131.3-131.7 k against 134.0-134.5 k frames/s at 1080p SDR -- the frame is small enough to be re-read from L2, and the
// deferred order adds the grid-sample launch; tools/attic/r05/deferred_planes_fast_kernel.diff)
inline bool warp_period_can_build_planes(const Geom& g, const PhaseLayout& pl, int n_members) {
    if (!one_cell_per_thread(g, 16) || small_frame(g)) return false;
    const int per_launch = n_members < kMaxWarpBatch ? n_members : kMaxWarpBatch;
    return staged_rounds(warp_n_tiles(g, 16), per_launch) && g.H == (g.lh << g.rs) && plane_emission_geometry(g, pl);
}

// ------------------------------------------------------------------------------------------
// warp: the plan
// ------------------------------------------------------------------------------------------
enum WarpFamily { kWarpNone = 0, kWarpFast = 1, kWarpStaged = 2 };
// One launch of members [first, first + count) of a set of periods: everything its dispatcher needs.
struct WarpLaunch {
    int family;                  // kWarpFast: warp_fast_kernel<E, group, rows, mode, vb, dw>;  kWarpStaged: warp_wg_kernel<E, mode, kWgWaves * 2 / kWgRows, kWgRows>
    int first, count;
    int vb, group, dw;           // bytes per thread and row, elements of a run group, dword-aligned source loads possible
    int rows, y_groups;          // rows per thread, luma row groups
    int out_chunk, n_chunks;     // outputs of the period one thread produces, chunks of outputs per tile
    int waves;                   // per workgroup
    uint32_t grid, block;
    // kWarpStaged only
    int plane_blocks;            // plane-building workgroups per super row (0: the launch builds no planes)
    int blocks_per_member, wpr;  // the dividers: per_member = (blocks_per_member, max_unit), per_sr = (wpr * 3 + plane_blocks, blocks_per_member),
    uint64_t max_unit;           //              wpr = (wpr, wpr * 3 + plane_blocks)
    uint32_t lds_bytes;          // dynamic LDS: the two source windows
    uint32_t planes;             // bit m: member first + m gets the phase plane of its frame21 built by this launch
};
// A set of 1 .. kMaxFlowBatch periods: one or two launches of at most kMaxWarpBatch members (kernel-argument space).  n_launches == 0:
// some member's shape does not qualify and NOTHING is launched -- all parts are planned before the first one goes out.
struct WarpPlan {
    int n_launches;
    WarpLaunch launch[kMaxFlowBatch / kMaxWarpBatch];
};

// Does the fast kernel with vb bytes per thread and row apply to every member of the part?  dw: dword-aligned source loads possible.
inline bool warp_fast_shape(const Geom& g, int count, const WarpPeriod* p, int mode, int vb, bool& dw) {
    const size_t esz = elem_size(g);
    const int vec = vb / (int)esz, group = warp_group(g, vb);
    bool fast = mode >= 0 && mode <= 2 && (g.in_stride % 2) == 0 && (g.out_stride % vec) == 0 &&
                g.W >= 2 * vec && group >= 2 && vec % group == 0 && vec / group <= 4;   // (group >= 2: a chroma run is made of element PAIRS)
    // dword-aligned source loads (load_run_dw) need dword-aligned frames and rows that end on a dword
    dw = ((size_t)g.in_stride * esz) % 4 == 0 && ((size_t)g.W * esz) % 4 == 0 && ((size_t)g.H * g.in_stride * esz) % 4 == 0;
    for (int m = 0; m < count && fast; m++) {
        const WarpPeriod& a = p[m];
        // blend shortcuts of the fast kernel need 0 <= t <= 1 and levels that cannot produce NaN;
        // chroma runs are read with element-pair granularity: needs an even input stride
        const bool sane = a.white != a.black && a.white != 0.0f && a.white == a.white && a.black == a.black;
        fast = fast && (mode != 2 || sane) && a.flow_xy && a.n_out >= 1 && a.n_out <= kMaxWarpOutputs;
        for (int i = 0; i < a.n_out && fast; i++)
            fast = fast && a.ts[i] >= 0.0f && a.ts[i] <= 1.0f && (((uintptr_t)a.outs[i]) & (uintptr_t)(vb - 1)) == 0;
        dw = dw && (((uintptr_t)a.frame12 | (uintptr_t)a.frame21) & 3) == 0;
    }
    return fast;
}

// One part with vb bytes per thread and row; family kWarpNone: not this shape.
inline WarpLaunch plan_warp_launch(const Geom& g, int first, int count, const WarpPeriod* p, int mode, int vb, const PhaseLayout* pl) {
    WarpLaunch L{};
    bool dw = false;
    if (!warp_fast_shape(g, count, p, mode, vb, dw)) return L;
    L.first = first; L.count = count; L.vb = vb; L.group = warp_group(g, vb); L.dw = dw;
    L.rows = kWarpFastRows;
    L.y_groups = (g.H + L.rows - 1) / L.rows;
    const int wpr = warp_tiles_per_row(g, vb);
    const long n_tiles = warp_n_tiles(g, vb);
    int max_out = 1;
    for (int m = 0; m < count; m++) max_out = p[m].n_out > max_out ? p[m].n_out : max_out;
    // outputs per thread: everything for large frames; one for frames up to 1080p (measured, fused 5-output period, us:
    // 1080p SDR 23.6 / 21.9 / 20.3 / 18.9 and 1080p HDR 19.0 / 19.1 with 6 / 3 / 2 / 1 outputs per thread; 2160p HDR
    // 45.9 / 46.6 hot, 50.8 / 52.1 HBM-cold with 6 / 1)
    // ... unless the launch has rounds of waves to spare (batched periods): then every thread produces all outputs there too
    // (1080p SDR 24 -> 60, 2 batches of 16: 107.9 -> 114.2 k frames/s)
    L.out_chunk = small_frame(g, 2) && n_tiles * count < kWarpRounds ? 1 : kMaxWarpOutputs;
    L.n_chunks = (max_out + L.out_chunk - 1) / L.out_chunk;
    // one LDS window per workgroup of kWgWaves stacked wave tiles (warp_wg_kernel): one flow cell per 16-byte thread, all outputs of the
    // period per thread, dword-aligned frames, launches of several rounds of waves (inside the pipeline the staged launch is 10 % shorter
    // than the global path -- 1,385 vs 1,545-1,595 us per 16 members, round 3)
    constexpr int NW = kWgWaves * 2 / kWgRows;     // waves per workgroup (tile height kWgWaves x 8 rows)
    const int yb = (warp_tile_rows(g.H, kWgRows) + NW - 1) / NW, ub = (warp_tile_rows(g.H >> 1, kWgRows) + NW - 1) / NW;
    const int plane_blocks = ((g.lw >> 2) * (2 * NW * kWarpTY * kWgRows) + 64 * NW - 1) / (64 * NW);   // (groups of 4 columns) x (luma rows of a super row) tasks
    // (its workgroups decode their unit index with scalar multiply-high divisions, exact while units x blocks per member < 2^32: frames
    //  far beyond 8K take the fast kernel)
    const uint32_t nb_max = (uint32_t)wg_blocks_per_member(wpr, yb, ub, plane_blocks);
    if (vb == 16 && one_cell_per_thread(g, vb) && dw && L.out_chunk > 1 && max_out >= 2 && staged_rounds(n_tiles, count) &&
        fastdiv_exact((uint64_t)nb_max * count + 8, nb_max)) {
        L.family = kWarpStaged;
        // deferred phase planes: members that ask for one (plane21) get it from this launch if geometry and alignment allow
        if (pl && plane_emission_geometry(g, *pl))
            for (int m = 0; m < count; m++)
                if (p[m].plane21 && (((uintptr_t)p[m].frame21) & 15) == 0) L.planes |= 1u << m;
        L.plane_blocks = L.planes ? plane_blocks : 0;
        L.wpr = wpr;
        L.blocks_per_member = wg_blocks_per_member(wpr, yb, ub, L.plane_blocks);
        L.max_unit = (uint64_t)L.blocks_per_member * count + 8;   // (units of a launch incl. the padding of its grid to a multiple of 8)
        L.waves = NW;
        L.grid = (uint32_t)((L.blocks_per_member * count + 7) / 8) * 8; L.block = 64 * NW;
        L.lds_bytes = (uint32_t)(2 * wg_chunks(NW * kWgRows / 2) * 16);
        return L;
    }
    L.family = kWarpFast;
    // large workgroups only where the launch keeps every CU supplied with them (>= 4 rounds of 8,192 resident waves)
    L.waves = L.out_chunk > 1 && n_tiles * L.n_chunks * count >= kWarpRounds ? warp_max_waves(elem_size(g), L.group, vb) : kWarpWavesSmall;
    const int n_blocks = ((int)n_tiles + L.waves - 1) / L.waves;
    L.grid = (uint32_t)((n_blocks * L.n_chunks * count + 7) / 8) * 8; L.block = 64 * L.waves;
    return L;
}

// The launches of n periods of one geometry in `mode`.  Per part (dw, too, is decided per part, not per batch): frames up to 1080p 8-bit
// try 8-byte threads first and fall through to 16.  launch_warp (one context, one output) asks with a one-output period.
inline WarpPlan plan_warp_periods(const Geom& g, int n, const WarpPeriod* periods, int mode, const PhaseLayout* pl) {
    WarpPlan P{};
    if (n < 1 || n > kMaxFlowBatch) return P;
    int parts = 0;
    for (int first = 0; first < n; first += kMaxWarpBatch, parts++) {
        const int count = n - first < kMaxWarpBatch ? n - first : kMaxWarpBatch;
        for (int m = 0; m < count; m++)
            if (periods[first + m].n_out < 1 || periods[first + m].n_out > kMaxWarpOutputs) return WarpPlan{};
        WarpLaunch L{};
        if (small_frame(g)) L = plan_warp_launch(g, first, count, periods + first, mode, 8, nullptr);
        if (L.family == kWarpNone) L = plan_warp_launch(g, first, count, periods + first, mode, 16, pl);
        if (L.family == kWarpNone) return WarpPlan{};
        P.launch[parts] = L;
    }
    P.n_launches = parts;
    return P;
}

// A source period of more than kMaxWarpOutputs outputs (24 fps -> 144 Hz and above) is a few launches of the same kernels.  THE rule of the
// split, for a lone context (any n_out) and a batch alike (hf_calc.hip interpolate_period): chunk c of a member holds its outputs
// [c * kMaxWarpOutputs, min((c + 1) * kMaxWarpOutputs, n_out)) -- period_chunk_count of them: every output in exactly one chunk, in order;
// chunk 0 holds every member that has an output at all; a period has period_chunks(largest n_out) chunks, none when nobody has an output.
constexpr int period_chunk_count(int n_out, int c) {
    return n_out - c * kMaxWarpOutputs < 0 ? 0 : n_out - c * kMaxWarpOutputs < kMaxWarpOutputs ? n_out - c * kMaxWarpOutputs : kMaxWarpOutputs;
}
constexpr int period_chunks(int n_out) { return n_out < 1 ? 0 : (n_out - 1) / kMaxWarpOutputs + 1; }
// The rule as a table, for a batch's calls: an n_out outside [0, kMaxPeriodOutputsWide] is clamped here and refused by their argument checks.
constexpr int kMaxPeriodOutputsWide = 24;   // HF_MAX_PERIOD_OUTPUTS_WIDE (23.976 fps -> 480 Hz: 21)
constexpr int kMaxPeriodChunks = period_chunks(kMaxPeriodOutputsWide);
struct PeriodChunks {
    int n_chunks;
    uint8_t count[kMaxPeriodChunks][kMaxFlowBatch];   // outputs of member m in chunk c (0: the member sits the chunk out)
};
inline PeriodChunks plan_period_chunks(int n, const int* n_out) {
    PeriodChunks P{};
    for (int m = 0; m < n && m < kMaxFlowBatch; m++) {
        const int total = n_out[m] > kMaxPeriodOutputsWide ? kMaxPeriodOutputsWide : n_out[m];
        for (int c = 0; c < period_chunks(total); c++) P.count[c][m] = (uint8_t)period_chunk_count(total, c);
        if (period_chunks(total) > P.n_chunks) P.n_chunks = period_chunks(total);
    }
    return P;
}

// The order of one hf_batch_run_period_auto period behind its update (hf_batch.hip batch_run_period_auto follows it step by step).  Every
// chunk has three launches -- its warps, the predicated copy of the members whose period turned out to be a cut, under a planar output side
// its conversion -- in that order; the copy needs the decision, which needs the chain.  The warps need neither, so on a batch that defers
// its phase planes (defers) and whose leader asked for it (flag: HF_FLAG_BATCH_AUTO_DEFERRED) the warps of chunk 0 go out AHEAD of the chain
// and build the planes the chain reads, exactly where hf_batch_run_period sends them ahead: some member's older plane still lacks its full
// build (pending), a warp mode (0 .. 2), every member has an output -- chunk 0 then holds every member.  Its copy and conversion wait for
// the decision; the later chunks are whole.  In every other case: chain, decision, then chunk by chunk.  chunks: plan_period_chunks'
// n_chunks; a period without any output still has its one (empty) chunk, whose copy launch goes out as it always has.  A launch that has
// nothing to do in a period (no planar output, no member with outputs in the chunk) is skipped by the host, not by the plan.
enum PeriodStepKind { kStepEarlyWarps = 0, kStepChain = 1, kStepDecide = 2, kStepWarps = 3, kStepCopy = 4, kStepConvert = 5 };
struct PeriodStep { uint8_t kind, chunk; };
constexpr int kMaxAutoPeriodSteps = 2 + 3 * kMaxPeriodChunks;
struct AutoPeriodPlan {
    int n_steps;
    int early;                              // chunk 0's warps are the first step
    PeriodStep step[kMaxAutoPeriodSteps];
};
constexpr AutoPeriodPlan plan_auto_period(bool defers, bool flag, bool pending, int mode, bool all_have, int chunks) {
    AutoPeriodPlan P{};
    const int n_chunks = chunks < 1 ? 1 : chunks > kMaxPeriodChunks ? kMaxPeriodChunks : chunks;
    P.early = defers && flag && pending && mode >= 0 && mode <= 2 && all_have && chunks >= 1;
    if (P.early) P.step[P.n_steps++] = PeriodStep{kStepEarlyWarps, 0};
    P.step[P.n_steps++] = PeriodStep{kStepChain, 0};
    P.step[P.n_steps++] = PeriodStep{kStepDecide, 0};
    for (int c = 0; c < n_chunks; c++) {
        if (!(P.early && c == 0)) P.step[P.n_steps++] = PeriodStep{kStepWarps, (uint8_t)c};
        P.step[P.n_steps++] = PeriodStep{kStepCopy, (uint8_t)c};
        P.step[P.n_steps++] = PeriodStep{kStepConvert, (uint8_t)c};
    }
    return P;
}
// which of a chunk's three launches a call of interpolate_period (hf_calc.hip) issues
enum PeriodParts { kPartWarps = 1, kPartCopy = 2, kPartConvert = 4, kPartsAll = 7 };

// warp_kernel / copy_kernel <E, 16 / sizeof(E), aligned>: 16-byte stores, 256-thread workgroups.
struct PlanePassPlan {
    int aligned;
    uint32_t grid_x, grid_y, block;
};
inline PlanePassPlan plan_plane_pass(const Geom& g, bool aligned) {
    const int vec = 16 / (int)elem_size(g);
    return PlanePassPlan{aligned ? 1 : 0, (uint32_t)((g.W + 64 * vec - 1) / (64 * vec)), (uint32_t)((g.H + (g.H >> 1) + 3) / 4), 256u};
}
inline PlanePassPlan plan_warp_generic(const Geom& g, const void* out) {
    return plan_plane_pass(g, (g.out_stride % (16 / (int)elem_size(g))) == 0 && (((uintptr_t)out) & 15) == 0);
}
inline PlanePassPlan plan_copy(const Geom& g, const void* src, const void* out) {
    const int vec = 16 / (int)elem_size(g);
    return plan_plane_pass(g, (g.in_stride % vec) == 0 && (g.out_stride % vec) == 0 && (((uintptr_t)src | (uintptr_t)out) & 15) == 0);
}

// ------------------------------------------------------------------------------------------
// chain and blur
// ------------------------------------------------------------------------------------------
// Batches up to this size run the two finest levels with one row per lane (MapRow).  Chain alone, us per batched chain with a block /
// a row per lane: 1 pair 79.5 / 71.3, 2 pairs 94.6 / 86.8, 4 pairs 122.4 / 119.2, 8 pairs 169.3 / 173.8.
constexpr int kRowPerLaneMaxBatch = 4;
#ifndef HF_LEVEL32_ONE_WAVE_MIN_BATCH
#define HF_LEVEL32_ONE_WAVE_MIN_BATCH 4
#endif
constexpr int kLevel32OneWaveMinBatch = HF_LEVEL32_ONE_WAVE_MIN_BATCH;   // batches from this size on: level 32 as one wave per window
// Waves per workgroup of a large-window step.  A chain alone (2160p HDR, 16 pairs): 4 waves 214 us, 1 wave 224 us (more atomics, and the Y
// launch's candidate rows come out of L2 instead of LDS).  Inside a throughput pipeline the other queues' kernels hold most of every CU and
// a single wave finds room sooner: same-box A-B with one-wave workgroups 1080p SDR + 1.4-3 %, 2160p SDR + 2.5 %, 64 pairs + 0.9 %, 1080p HDR
// + 0.3 %, 2160p HDR (bandwidth-bound) +- 0; 360p (rs = 1) - 1.5 %.  A throughput driver's batches at rs >= 2 take one wave.  (Measured,
// round 6; before level 32 became a one-wave launch too, 2160p HDR lost 2 % with them; a 16 x 16 one-wave Y tile with staged rows was no
// better than the plain one.)
#ifndef HF_BIG_ONE_WAVE_MIN_BATCH
#define HF_BIG_ONE_WAVE_MIN_BATCH 4
#endif
constexpr int kBigWavesPerBlock = 4, kBigOneWaveMinBatch = HF_BIG_ONE_WAVE_MIN_BATCH, kBigOneWaveMinRs = 2;
constexpr int kBlurWindowSumMinDim = 64;   // the blur's window-sum forms need a grid of at least 64 x 64 (blur_flow_kernel re-tests it)

// Per level: the SAD tables are written by every small level that has a successor's worth of blocks (windows 32 .. 4) and read by every
// small level behind a small level.  levels: the chain's (only their window sizes are read); tables: the chain keeps tables at all.
struct SadUse { int read, write; };
constexpr SadUse plan_sad_tables(const FlowLevel* levels, int k, bool tables) {
    const bool small = levels[k].window <= 32;
    return SadUse{tables && small && k > 0 && levels[k - 1].window <= 32, tables && small && levels[k].window >= 4};
}

// A level of windows <= 32 (flow_level_small_kernel<window, window <= 16, rows1, tabk>, or flow_level32_wave_kernel<tabk>).
struct SmallLevelPlan {
    int one_wave32;          // level 32 as one wave per window
    int rows1;               // one row per lane (MapRow) instead of a block (Map)
    int tile_w;              // tile width (the tile is 32 rows high)
    int waves;               // one-wave workgroups per tile (1: the tile is one workgroup)
    int tabk;                // the SAD-table bodies
    uint32_t block;
};
constexpr SmallLevelPlan plan_flow_level_small(int n, int window, int R, bool tables_present, bool sad_read, bool sad_write) {
    SmallLevelPlan P{};
    P.one_wave32 = window == 32 && n >= kLevel32OneWaveMinBatch;
    P.rows1 = n <= kRowPerLaneMaxBatch && window <= 4;
    P.tile_w = P.rows1 && window == 2 ? 16 : 32;          // (32 x 32 tiles at every level but MapRow<2>: 16 x 32)
    // windows <= 16 never span waves: one-wave workgroups, see flow_level_small_kernel (Map<4> covers a tile with two waves)
    P.waves = window == 32 ? 1 : window == 4 && !P.rows1 ? 2 : 4;
    P.tabk = tables_present && R == 16 && (sad_read || sad_write);
    P.block = window == 32 && !P.one_wave32 ? 256u : 64u;
    return P;
}
// A large-window step: waves per workgroup (flow_big_partial_kernel<1 | kBigWavesPerBlock>).
constexpr int plan_flow_big_waves(int n, int rs) { return n >= kBigOneWaveMinBatch && rs >= kBigOneWaveMinRs ? 1 : kBigWavesPerBlock; }

enum BlurKernel { kBlur32x4WindowSums = 0, kBlur32x4Taps = 1, kBlur32x0 = 2, kBlur16x0 = 3 };   // the first two are blur_flow_kernel<32, 4>
struct BlurPlan {
    int kernel;
    int tile;                // outputs per workgroup: tile x tile
    uint32_t grid_x, grid_y;
    size_t lds_bytes;
};
inline BlurPlan plan_blur(const Geom& g, int n, const FlowLevel& L, int radius) {
    // the window-sum form of blur_flow_kernel<32, 4> applies (same test as in the kernel): then 32 x 32 tiles are the faster ones at every batch size
    const bool window_sums = L.tx && L.ty && L.log2w == 1 && !(g.lw & 1) && !(g.lh & 1) && g.lw >= kBlurWindowSumMinDim && g.lh >= kBlurWindowSumMinDim &&
                             L.nwx * 2 == g.lw && L.nwy * 2 == g.lh;
    BlurPlan P{};
    if (radius == 4 && (n > 4 || window_sums)) {   // the reference's radius: 32 x 32 outputs per workgroup, taps unrolled (with the tap loops a single
                                                   // pair is faster with four times the workgroups: 4.3 vs 6.0 us)
        const int T = 32 + 8;
        P.kernel = window_sums ? kBlur32x4WindowSums : kBlur32x4Taps; P.tile = 32;
        P.lds_bytes = (size_t)T * (T + 1) * sizeof(uint32_t) + 2 * (size_t)T * 32 * sizeof(int);   // 16.8 KB (odd row pitch, see the kernel)
    } else if (window_sums && radius >= 2 && radius <= 64 && !(radius & 1)) {   // any even radius in the window-sum form (blur_flow_kernel<32, 0>)
        const int nw = 16 + radius;
        P.kernel = kBlur32x0; P.tile = 32;
        P.lds_bytes = (size_t)nw * nw * sizeof(uint32_t) + 2 * (size_t)nw * 17 * sizeof(int) + 2 * 17 * 17 * sizeof(int);   // 18 KB at radius 32, 39 KB at 64
    } else {
        const int T = 16 + 2 * radius;
        P.kernel = kBlur16x0; P.tile = 16;
        P.lds_bytes = (size_t)T * (T + 1) * sizeof(uint32_t) + 2 * (size_t)T * 16 * sizeof(int);
    }
    P.grid_x = (uint32_t)((g.lw + P.tile - 1) / P.tile); P.grid_y = (uint32_t)((g.lh + P.tile - 1) / P.tile);
    return P;
}

}  // namespace hf
