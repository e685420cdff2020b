// tests/launch_plan_probe.cpp -- the launch plan functions of csrc/hf_launch_plan.h behind extern "C", for ctypes (tests/launch_plan_probe.py).
// Includes ONLY that header and is compiled with plain g++, no ROCm include path: the compile is the proof that the header is HIP-free.
// Pointers are fabricated from alignment offsets and presence flags -- the plan functions never dereference them.
#include "hf_launch_plan.h"

using namespace hf;

namespace {
Geom geom(const int* v) { return Geom{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]}; }   // hdr H W in_stride out_stride rs lw lh
template <typename T> T* fake(uintptr_t base, uint32_t off) { return reinterpret_cast<T*>(base + off); }
}

extern "C" {

struct ProbeMember {
    int n_out;
    float ts[kMaxWarpOutputs];
    uint32_t out_off[kMaxWarpOutputs];     // byte offsets of the outputs / sources from a 4 KB-aligned base
    uint32_t src12_off, src21_off;
    int has_flow_xy, wants_plane;
    float black, white;
};

enum { kProbeLaunchFields = 19, kProbeMaxMembers = 64 };

void hfp_constants(long long* o) {
    const long long v[] = {kWarpTX, kWarpTY, kWarpWavesSmall, kWarpWavesLarge, kWgWaves, kWgRows, kWgChunksPerWave, kWgMinWaves, kMaxWarpBatch,
                           kMaxWarpOutputs, kMaxFlowBatch, (long long)kSmallFrameBytes, kWarpRounds, kWarpFastRows, kRowPerLaneMaxBatch,
                           kLevel32OneWaveMinBatch, kBigOneWaveMinBatch, kBigOneWaveMinRs, kBigWavesPerBlock, kBlurWindowSumMinDim,
                           wg_chunks(1), kProbeLaunchFields, (long long)sizeof(ProbeMember)};
    for (unsigned i = 0; i < sizeof(v) / sizeof(v[0]); i++) o[i] = v[i];
}

// Returns n_launches; out[launch][kProbeLaunchFields] in the order of WarpLaunch's members.
int hfp_plan_warp(const int* gv, int n, const ProbeMember* ms, int mode, int have_pl, int max_iters, long long* out) {
    static WarpPeriod periods[kProbeMaxMembers];
    const Geom g = geom(gv);
    for (int m = 0; m < n && m < kProbeMaxMembers; m++) {
        WarpPeriod p{};
        const uintptr_t base = 0x10000000u + 0x100000u * (uintptr_t)m;
        p.frame12 = fake<const void>(base, ms[m].src12_off); p.frame21 = fake<const void>(base + 0x40000u, ms[m].src21_off);
        p.flow = fake<const int16_t>(base + 0x80000u, 0);
        p.flow_xy = ms[m].has_flow_xy ? fake<const uint32_t>(base + 0x90000u, 0) : nullptr;
        p.n_out = ms[m].n_out;
        for (int i = 0; i < kMaxWarpOutputs; i++) { p.outs[i] = fake<void>(base + 0xA0000u + 0x1000u * i, ms[m].out_off[i]); p.ts[i] = ms[m].ts[i]; }
        p.black = ms[m].black; p.white = ms[m].white;
        p.plane21 = ms[m].wants_plane ? fake<uint32_t>(base + 0xB0000u, 0) : nullptr;
        periods[m] = p;
    }
    const PhaseLayout pl = make_phase_layout(g, max_iters);
    const WarpPlan P = plan_warp_periods(g, n, periods, mode, have_pl ? &pl : nullptr);
    for (int i = 0; i < P.n_launches; i++) {
        const WarpLaunch& L = P.launch[i];
        const long long v[kProbeLaunchFields] = {L.family, L.first, L.count, L.vb, L.group, L.dw, L.rows, L.y_groups, L.out_chunk, L.n_chunks, L.waves,
                                                 L.grid, L.block, L.plane_blocks, L.blocks_per_member, L.wpr, (long long)L.max_unit, L.lds_bytes, L.planes};
        for (int k = 0; k < kProbeLaunchFields; k++) out[i * kProbeLaunchFields + k] = v[k];
    }
    return P.n_launches;
}

int hfp_can_build_planes(const int* gv, int max_iters, int n_members) {
    const Geom g = geom(gv);
    return warp_period_can_build_planes(g, make_phase_layout(g, max_iters), n_members);
}

void hfp_phase_layout(const int* gv, int max_iters, long long* o) {
    const PhaseLayout pl = make_phase_layout(geom(gv), max_iters);
    o[0] = pl.rs; o[1] = pl.nph; o[2] = pl.nph2; o[3] = pl.mx; o[4] = pl.lwp; o[5] = (long long)pl.bytes;
}

// o[0]: the fast plane build applies to frames of this geometry (their bases' alignment aside); o[1]: the staged warp launch can build planes
void hfp_plane_fast_geometry(const int* gv, int max_iters, long long* o) {
    const Geom g = geom(gv);
    const PhaseLayout pl = make_phase_layout(g, max_iters);
    o[0] = plane_fast_geometry(g, pl); o[1] = plane_emission_geometry(g, pl);
}

static void plane_pass(const PlanePassPlan& P, long long* o) { o[0] = P.aligned; o[1] = P.grid_x; o[2] = P.grid_y; o[3] = P.block; }
void hfp_plan_warp_generic(const int* gv, uint32_t out_off, long long* o) { plane_pass(plan_warp_generic(geom(gv), fake<void>(0x10000000u, out_off)), o); }
void hfp_plan_copy(const int* gv, uint32_t src_off, uint32_t out_off, long long* o) {
    plane_pass(plan_copy(geom(gv), fake<const void>(0x10000000u, src_off), fake<void>(0x20000000u, out_off)), o);
}

int hfp_fastdiv_exact(unsigned long long max_u, uint32_t d) { return fastdiv_exact(max_u, d); }
int hfp_wg_blocks_per_member(int wpr, int yb, int ub, int plane_blocks) { return wg_blocks_per_member(wpr, yb, ub, plane_blocks); }

void hfp_plan_flow_level_small(int n, int window, int R, int tables_present, int sad_read, int sad_write, long long* o) {
    const SmallLevelPlan P = plan_flow_level_small(n, window, R, tables_present != 0, sad_read != 0, sad_write != 0);
    o[0] = P.one_wave32; o[1] = P.rows1; o[2] = P.tile_w; o[3] = P.waves; o[4] = P.tabk; o[5] = P.block;
}
int hfp_plan_flow_big_waves(int n, int rs) { return plan_flow_big_waves(n, rs); }
void hfp_plan_sad_tables(const int* windows, int n_levels, int k, int tables, long long* o) {
    FlowLevel levels[32] = {};
    for (int i = 0; i < n_levels && i < 32; i++) levels[i].window = windows[i];
    const SadUse s = plan_sad_tables(levels, k, tables != 0);
    o[0] = s.read; o[1] = s.write;
}
// last: the chain's last level (has_tables 0: the level does not exist)
void hfp_plan_blur(const int* gv, int n, int has_tables, int log2w, int nwx, int nwy, int radius, long long* o) {
    FlowLevel L{};
    L.window = 1 << log2w; L.log2w = log2w; L.nwx = nwx; L.nwy = nwy;
    L.tx = has_tables ? fake<int16_t>(0x10000000u, 0) : nullptr; L.ty = has_tables ? fake<int16_t>(0x20000000u, 0) : nullptr;
    const BlurPlan P = plan_blur(geom(gv), n, L, radius);
    o[0] = P.kernel; o[1] = P.tile; o[2] = P.grid_x; o[3] = P.grid_y; o[4] = (long long)P.lds_bytes;
}

}  // extern "C"
