// hopperrender_amd/csrc/hf_kernels.h -- internal launch interface of the gfx950 kernels.
//
// Every launcher only ENQUEUES work on `stream` (no allocation, no synchronisation) so the
// whole flow chain can be captured into a hipGraph (cdna_hip_programming.md Guideline 9).
// Citations are relative to the reference's HopperRender/ directory.
#pragma once
#include <hip/hip_runtime.h>
#ifdef __HIPCC__
#include <hip/hip_ext.h>
#endif
#include <stdint.h>
#include "hf_launch_plan.h"   // Geom, PhaseLayout, FlowLevel, WarpPeriod, FastDiv, the launch constants and plan functions (host-only)

// Device debug build (`python -m hopperrender_amd.build --debug-bounds` => -DHF_DEBUG_BOUNDS, library libhopperflow_dbg.so): every
// gather index of the kernels (frame / phase-plane / flow-table / LDS-window reads) is checked against its buffer; a violation is
// RECORDED -- count + site, block and thread of the first one, in a __device__ record of the translation unit -- and the kernel goes on
// (a record the host reads with hf_debug_bounds_violations() is more robust than a trap: a trapped queue takes the device printf
// buffer and the whole context with it).  This replaces the GPU AddressSanitizer the pool cannot offer (the
// reference's own out-of-range case is the single reflection of calcDeltaSumsKernelSDR.h:86-95).  The product build compiles the
// checks away.
#ifdef HF_DEBUG_BOUNDS
#ifdef __HIPCC__
namespace hf { namespace {
__device__ unsigned int g_dbg_bounds[5];   // [0] violations, [1..4] site / block / thread / line of the first one (one record per translation unit)
__device__ __forceinline__ void dbg_bounds_record(int site, int line) {
    if (atomicAdd(&g_dbg_bounds[0], 1u) == 0u) {
        g_dbg_bounds[1] = (unsigned)site; g_dbg_bounds[2] = (unsigned)blockIdx.x; g_dbg_bounds[3] = (unsigned)threadIdx.x; g_dbg_bounds[4] = (unsigned)line;
    }
}
} }
#define HF_DBG_CHECK(cond, site) do { if (!(cond)) ::hf::dbg_bounds_record((site), __LINE__); } while (0)
#else
#define HF_DBG_CHECK(cond, site) do { } while (0)
#endif
#else
#define HF_DBG_CHECK(cond, site) do { } while (0)
#endif

namespace hf {

// ---- per-launch device timestamps without a profiler (hf_batch_timeline_*, include/hopperflow.h) ----
// `rocprofv3 --kernel-trace` makes the four batch streams host-issue-bound (its per-dispatch cost), so its timeline is not the timed
// run's.  Instead every launch of the library can carry the start / stop events of its own dispatch (hipExtLaunchKernelGGL: the same
// timestamps the kernel trace reads): while a thread has a LaunchObserver installed, HF_LAUNCH hands each launch a pair of events from it
// and notes the kernel's name; otherwise it is the plain launch.  Installed only by hf_batch_run_period of a batch whose timeline is on.
struct LaunchObserver {
    virtual bool next(const char* kernel_name, hipEvent_t* start, hipEvent_t* stop) = 0;   // false: out of records, launch unobserved
protected:
    ~LaunchObserver() = default;
};
extern thread_local LaunchObserver* t_launch_observer;

#ifdef __HIPCC__
#define HF_LAUNCH(NAME, KERNEL, GRID, BLOCK, LDS, STREAM, ...)                                                     \
    do {                                                                                                            \
        hipEvent_t hf_e0_ = nullptr, hf_e1_ = nullptr;                                                              \
        if (::hf::t_launch_observer && ::hf::t_launch_observer->next((NAME), &hf_e0_, &hf_e1_))                    \
            hipExtLaunchKernelGGL(KERNEL, GRID, BLOCK, LDS, STREAM, hf_e0_, hf_e1_, 0, __VA_ARGS__);                \
        else                                                                                                        \
            hipLaunchKernelGGL(KERNEL, GRID, BLOCK, LDS, STREAM, __VA_ARGS__);                                      \
    } while (0)
#endif

// The device half of FastDiv (hf_launch_plan.h).
#ifdef __HIPCC__
__device__ __forceinline__ uint32_t fastdiv(uint32_t u, const FastDiv f) { return f.magic ? __umulhi(u, f.magic) : f.d > 1 ? u / f.d : u; }
#endif

// Device-side diagnostic counters of a context (hf_debug_counters_enable): u32 [kCounterWords]
//   [0 .. 2]                       period-warp workgroups by path: staged window, interior-global, generic (warp_wg_kernel)
//   [8 + 4 k + 2 axis + {0, 1}]    level k of the chain: windows of its table tiles, those of them that reused their SAD vectors
constexpr int kCounterWarp = 0, kCounterLevels = 8, kCounterWords = 8 + 4 * 16;
// A large-window step whose argmin has not been taken yet: the NEXT launch resolves it in its prologue
// (every workgroup recomputes the 16-way argmin of the window it lies in; the workgroup at the window's
// origin also stores the result in the level table) instead of a separate tiny launch.  Only used for
// steps without a neighbour term (levels < 4), so nothing in the consuming launch reads the table entry.
struct PendingArgmin {
    int active;
    int axis;                // axis of the pending step
    int capture_delta;       // pending step is the first of the chain: emit m_totalFrameDelta
    int use_neighbors;       // the pending step has a neighbour term (level >= 4): only the explicit argmin launch handles it
    FlowLevel lvl;           // level of the pending step (its table receives the result)
    FlowLevel lvl_prev;      // level before it (offset the candidates were relative to); tx == nullptr: zero
    const uint32_t* sums;    // [n_windows][16] raw SAD sums of the pending step
};

// One level (or one axis of a level for windows > 32) of the refinement chain
// (calcDeltaSums + determineLowestLayer + adjustOffsetArray of the reference).
struct FlowStep {
    const uint32_t* pp1;     // frame N-1 phase plane (candidates are sampled here)
    const uint32_t* pp2;     // frame N phase plane (its phase 0 = the grid samples)
    PhaseLayout pl;
    FlowLevel cur, prev;     // prev.tx == nullptr on the first level
    uint32_t* sums;          // [n_windows][16] raw SAD sums (windows > 32 only)
    uint32_t* total_delta;   // device slot of m_totalFrameDelta
    int axis;                // windows > 32: 0 = X step, 1 = Y step
    int R;                   // search radius = candidate count (2..16)
    int use_neighbors;       // iteration >= 4 (calcDeltaSumsKernelSDR.h:3,112)
    int delta_scalar, neighbor_scalar;
    int capture_delta;       // first step of the chain: emit m_totalFrameDelta
    uint32_t delta_divisor;  // lh*lw*10 (SDR) / lh*lw*6 (HDR)
    PendingArgmin pend;      // previous large-window step still to be resolved (see above)
    // ---- SAD tables: exact reuse of candidate SADs across steps (hf_flow.hip "SAD TABLES") ----
    FlowLevel prev2;         // the level before `prev` (tx == nullptr: none, all zero): prev - prev2 = what the parent window chose
    uint32_t* sadtab;        // [2 axes][sad_nby][sad_nbx][8]: the 16 candidate SADs (u16 pairs) of every 2x2 grid block as the last step
                             // of that axis that computed them left them; nullptr: reuse off (HF_FLAG_NO_SAD_REUSE)
    int sad_nbx, sad_nby;
    int sad_read;            // the previous level's launch left valid tables for every full tile (this is not the chain's first small level)
    int sad_write;           // this launch refreshes them where it computes (windows 32 .. 4)
    int y_rows_lds;          // this launch has dynamic LDS for the candidate rows of its Y steps (ysads_tile_lds / ysads_win8_lds)
    uint32_t* still_count;   // device: windows of the 32-level that chose d = 0 on both axes in this chain (the content hint, hf_calc.hip), or nullptr
    uint32_t* counters;      // diagnostic counters (hopperflow_diag.h hf_debug_counters, layout kCounter* below), nullptr: none
    int level_index;         // k of this level (its counter slot)
    // allocation bases of the per-level tables and of the window sums: a batched launch carries member 0's FlowStep and rebases it
    int16_t* tables_base;
    uint32_t* sums_base;
};

// The refinement chains of up to kMaxFlowBatch independent frame pairs of the SAME geometry and parameters run as
// one set of launches: every kernel of the chain takes the whole batch and blockIdx.z selects the pair.  One
// 480x270 chain is 135..1080 workgroups of latency-bound work per launch -- far too little for 256 CUs -- and
// the device runs at most a handful of HW queues side by side, so a throughput driver (SURVEY.md 8(e):
// independent pairs) gets its parallelism from the batch, not from more streams.  n == 1 is the drop-in path.
struct FlowBatch {
    int n;
    FlowStep s[kMaxFlowBatch];
};
struct BlurItem {
    FlowLevel last;          // offsets of the last level (tx == nullptr: all zero)
    int16_t* blurred;        // out [2][lh][lw]
    uint32_t* packed;        // out x | y << 16 per grid point (what the fast warp kernel reads)
    uint32_t* zero;          // window sums the (last) kernel of the chain clears for the next chain, or nullptr
    uint32_t* still_count;   // FlowStep::still_count of the chain: published to *still_out (mapped host memory) and cleared, or nullptr
    uint32_t* still_out;
};
struct BlurBatch {
    int n;
    BlurItem s[kMaxFlowBatch];
};

// Re-lay the freshly uploaded frames of n >= 1 contexts of one geometry as phase planes (once per frame) in one launch.
struct PrepBatch {
    int n;
    const void* frame[kMaxFlowBatch];
    uint32_t* pp[kMaxFlowBatch];
};
void launch_prep_frames(const Geom& g, const PhaseLayout& pl, const PrepBatch& b, hipStream_t stream);
// Deferred plane build: only the grid samples of the new frames (phase pair 0 of the rows cy << rs -- all the chain reads of the
// NEWER frame's plane); the full plane follows from the next period's warp launch (launch_warp_periods) or launch_prep_frames.
void launch_prep_grid(const Geom& g, const PhaseLayout& pl, const PrepBatch& b, hipStream_t stream);
// Windows <= 32: X and Y step of one level in a single launch.
void launch_flow_level_small(const Geom& g, const FlowBatch& b, hipStream_t stream);
// Windows > 32, one axis: partial SAD sums (atomics), then argmin + table update.
void launch_flow_big_partial(const Geom& g, const FlowBatch& b, hipStream_t stream);
void launch_flow_big_argmin(const Geom& g, const FlowBatch& b, hipStream_t stream);
// m_offsetArray view ([2][lh][lw] int16) of the last level, for parity taps.
void launch_expand_offsets(const Geom& g, const FlowLevel& last, int16_t* out, hipStream_t stream);
// blurFlowKernel with a runtime radius (4 == reference); in: offsets of the last level, out: [2][lh][lw].
// zero_count: elements of BlurItem::zero to clear.
void launch_blur_flow(const Geom& g, const BlurBatch& b, int radius, int zero_count, hipStream_t stream);
void launch_pack_flow(const Geom& g, const int16_t* flow, uint32_t* packed, hipStream_t stream);
// All outputs of one source period in ONE launch (fast path only: modes 0-2 etc.), for up to kMaxFlowBatch contexts of
// the same geometry at once; returns false when the shape of a member does not qualify and the caller must fall back to
// one launch_warp per output.
// pl + planes_built[n] (optional): members whose period carries a plane21 pointer get the full phase plane of their frame21 built
// by the launch itself when it is the workgroup-staged kernel and geometry / alignment allow (planes_built[m] says so); everyone
// else's plane stays untouched and has to be built by launch_prep_frames.
bool launch_warp_periods(const Geom& g, int n, const WarpPeriod* periods, int mode, hipStream_t stream,
                         hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr, const PhaseLayout* pl = nullptr,
                         bool* planes_built = nullptr);
// (warp_period_can_build_planes, the static part of that decision which hf_batch takes once, is in hf_launch_plan.h.)
// warpFrameKernel, both planes in one launch.  black/white already scaled for HDR.
void launch_warp(const Geom& g, const void* frame12, const void* frame21, const int16_t* flow, const uint32_t* flow_xy,
                 void* out, float t, int mode, float black, float white, hipStream_t stream,
                 hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);  // events: timestamps of the dispatch itself
// Warp disagreement maps (hf_kernels.hip; hf_warp_disagreement_map_enqueue): for each of n_t <= kMaxDisagreementOutputs blending scalars,
// per tile of the error maps' grid, sse / sad / max of |a - b| with a / b what output modes 0 / 1 of launch_warp would store at an element.
// One launch, no frame written; maps = n_t maps of hf_error_tile [3][th][tw], 16-byte aligned, every entry of which the launch stores.
// false: nothing launched (n_t or tile out of range).
constexpr int kMaxDisagreementOutputs = 24;
bool launch_warp_disagreement(const Geom& g, const void* frame12, const void* frame21, const int16_t* flow, const uint32_t* flow_xy,
                              int n_t, const float* t, int tile, void* maps, hipStream_t stream);
// Guarded blend (hf_kernels.hip; hf_guarded_blend_enqueue): behind launch_warp_disagreement with the same sources, t and tile on the same
// stream, into outs[k] (a frame of g.out_stride each) the mode-2 output of launch_warp at t[k] mixed with the cross-fade by the weights
// that map k's luma sad and the thresholds give.  One launch per chunk of kMaxWarpOutputs outputs.  black/white already scaled for HDR.
// false: nothing launched (n_t, tile or thresholds out of range).
bool launch_guarded_blend(const Geom& g, const void* frame12, const void* frame21, const int16_t* flow, const uint32_t* flow_xy,
                          int n_t, const float* t, int tile, int lo_q4, int hi_q4, const void* maps, void* const* outs,
                          float black, float white, hipStream_t stream);
// copyFrameKernel, both planes in one launch.
void launch_copy(const Geom& g, const void* src, void* out, float black, float white, hipStream_t stream);
// Planar 4:2:0 frames at the device boundary (hf_planar.hip; HF_FLAG_PLANAR_IN / HF_FLAG_PLANAR_OUT): planar (Y, U, V planes) <-> the
// semi-planar NV12 / P010 frame, H rows of `stride` elements, padding included; HDR values are LSB-aligned on the planar side (<< 6 in,
// >> 6 out, wrapping in 16 bits).  Source and destination must not overlap.
void launch_planar_in(int hdr, int H, int stride, const void* planar, void* semi, hipStream_t stream);
void launch_planar_out(int hdr, int H, int stride, const void* semi, void* planar, hipStream_t stream);
// The same for n frames of one shape in ONE launch (hf_batch; HF_FLAG_BATCH_PLANAR_IN / HF_FLAG_BATCH_PLANAR_OUT): pair i reads src and
// writes dst.  In: planar -> semi-planar, n <= kMaxFlowBatch; out: semi-planar -> planar, n <= kMaxPlanarOutPairs.  n == 0: no launch.
struct PlanarPair {
    const void* src;
    void* dst;
};
constexpr int kMaxPlanarOutPairs = kMaxFlowBatch * kMaxWarpOutputs;
void launch_planar_in_batch(int hdr, int H, int stride, int n, const PlanarPair* pairs, hipStream_t stream);
void launch_planar_out_batch(int hdr, int H, int stride, int n, const PlanarPair* pairs, hipStream_t stream);
bool dbg_bounds_read_planar(unsigned out[5], bool reset);
// Frame error sums (hf_metrics.hip; hf_frame_error*): pair i of n <= kMaxErrorPairs compares frames a[i] and b[i] -- H rows of W elements,
// strides in elements per side, both NV12 / P010 or both planar -- into slots[i], which the caller zeroed on the same stream.  The layout
// of hf_frame_error (include/hopperflow.h).  false: nothing launched (n out of range, a frame beyond 2^32 work items).
struct FrameErrorSlot {
    uint64_t sse[3], sad[3], n_differ[3], count[3];   // index 0 Y, 1 U, 2 V
    uint32_t max_abs[3], reserved;
};
constexpr int kMaxErrorPairs = 192;
bool launch_frame_errors(int hdr, int H, int W, int stride_a, int stride_b, bool planar, int n, const void* const* a, const void* const* b,
                         FrameErrorSlot* slots, hipStream_t stream);
// Per-tile error maps (hf_metrics.hip; hf_frame_error_map*): the same pairs, strides and layouts; maps = n maps of hf_error_tile
// [3][th][tw] (include/hopperflow.h), 16-byte aligned, every entry of which the launch stores -- nothing to zero.  false: nothing launched
// (tile not 16, 32 or 64, n out of range, a frame beyond 2^32 work items).
bool launch_frame_error_map(int hdr, int H, int W, int stride_a, int stride_b, bool planar, int tile, int n, const void* const* a,
                            const void* const* b, void* maps, hipStream_t stream);
// Windowed SSIM (hf_metrics.hip; hf_frame_ssim*): the same pairs, strides and layouts as launch_frame_errors; per plane the summed and the
// largest loss 2^32 - round(ssim 2^32) over the 8 x 8 windows at stride 4 and their number, with the integer constants c1, c2 of the peak
// (include/hopperflow.h has the definition).  The layout of hf_frame_ssim; slots zeroed by the caller on the same stream.
struct FrameSsimSlot {
    uint64_t sum_loss_q32[3], max_loss_q32[3], count[3];   // index 0 Y, 1 U, 2 V
};
bool launch_frame_ssim(int hdr, int H, int W, int stride_a, int stride_b, bool planar, long long c1, long long c2, int n, const void* const* a,
                       const void* const* b, FrameSsimSlot* slots, hipStream_t stream);
// Per-tile SSIM maps (hf_metrics.hip; hf_frame_ssim_map*): the same pairs, strides, layouts and constants as launch_frame_ssim, the tile
// grid of launch_frame_error_map; maps = n maps of hf_ssim_tile [3][th][tw] in one device buffer, every entry of which the launch
// stores (no memset, no atomics).  false: nothing launched (n or tile out of range).
bool launch_frame_ssim_map(int hdr, int H, int W, int stride_a, int stride_b, bool planar, long long c1, long long c2, int tile, int n,
                           const void* const* a, const void* const* b, void* maps, hipStream_t stream);
bool dbg_bounds_read_metrics(unsigned out[5], bool reset);
// Scene-cut copy periods of a batch, decided on the device (hf_scene.hip; hf_batch_run_period_auto).  One record per member and period:
// the layout of hf_scene_record (include/hopperflow.h).
struct SceneRecord {
    uint32_t frame_count, total_delta;
    int32_t kind, average, d1, d2;
};
struct SceneState;   // hf_scene.h
// scene_decide: one thread per member, behind the chain's last launch.  A member with push set reads *total_delta once and pushes it
// (scene_push, hf_scene.h); every member gets kinds[m] = 1 warp / 0 copy and one record at records[m * ring + slot[m]] (mapped host memory).
struct SceneDecideArgs {
    int n;
    const uint32_t* total_delta[kMaxFlowBatch];   // FlowStep::total_delta of the member (mapped host memory the chain published to)
    uint32_t frame_count[kMaxFlowBatch];          // m_frameCount of the period
    uint32_t threshold[kMaxFlowBatch];
    uint32_t slot[kMaxFlowBatch];                 // record slot of this period in the member's ring
    int8_t cap[kMaxFlowBatch];                    // scene_history_cap of the member
    int8_t push[kMaxFlowBatch];                   // m_frameCount >= 3: the chain's delta joins the history
    int8_t clear[kMaxFlowBatch];                  // the member was (re-)armed since its last period: the history starts over first
    int8_t force[kMaxFlowBatch];                  // -1: decide, 0: copy, 1: warp
};
void launch_scene_decide(const SceneDecideArgs& a, SceneState* states, int32_t* kinds, SceneRecord* records, uint32_t ring, hipStream_t stream);
// The predicated copy behind a period's warps: a member whose kinds[m] is 0 gets each of its n_out outputs overwritten with what copy_kernel
// writes (the valid columns of every row, levels applied); workgroups of the other members leave after one load.
struct SceneCopyArgs {
    int n;
    struct Member {
        const void* src;                          // the ring frame copyFrame shows (opticalFlowCalcSDR.cpp:173)
        void* outs[kMaxWarpOutputs];
        int n_out;
        float black, white;                       // already scaled for HDR
    } m[kMaxFlowBatch];
};
void launch_scene_copy(const Geom& g, const SceneCopyArgs& a, const int32_t* kinds, hipStream_t stream);
bool dbg_bounds_read_scene(unsigned out[5], bool reset);
// Debug-bounds records of the two kernel translation units (hf_kernels.hip / hf_flow.hip): out[0] += violations, out[1..4] = the first
// one's site / block / thread / source line; reset: zero the records.  Return false in a build without HF_DEBUG_BOUNDS.
bool dbg_bounds_read_kernels(unsigned out[5], bool reset);
bool dbg_bounds_read_flow(unsigned out[5], bool reset);
// Self-test: a kernel with 64 out-of-range "indices" (scratch: >= 65 ints of device memory): a checking build records 64 violations of site 999.
void launch_bounds_selftest(int* scratch, hipStream_t stream);
// v_rcp_f32 of the device (parity tooling: the reference's levels use it through OpenCL's fdiv).
void launch_rcp_probe(const float* in, float* out, int n, hipStream_t stream);

}  // namespace hf
