// hopperrender_amd/csrc/hf_ctx.h -- internal: the context and batch objects behind the C ABI of include/hopperflow.h and the helpers the
// translation units of that ABI share.  The ABI is split by concern:
//   hf_context.hip   context lifetime and state: hf_create / hf_destroy (detectDevices, buffers: opticalFlowCalcSDR.cpp:206-325), parameters,
//                    statistics, profiling spans, parity taps, device-memory helpers, hf_debug_live_resources (the counts of the owners below)
//   hf_calc.hip      the five virtuals of one context: updateFrame, calculateOpticalFlow (the refinement chain as a cached hipGraph), warpFrames,
//                    copyFrame, downloadFrame, and the fused period calls.  update_frames() there is the ONE host path of a frame update, for
//                    n >= 1 contexts: hf_update_frame / _device / _device_ref and, behind its own H2D, hf_update_frame_async are its n = 1
//                    cases, a batch's update the same call over its members.  calculate_flow() there is the ONE host path of a chain, for n >= 1
//                    contexts on a stream: hf_calculate_optical_flow is its n = 1 case, a batch's chain the same call on the batch's stream.
//                    interpolate_period() there is the ONE host path of a source period's warps, for n >= 1 contexts chunk by chunk (targets,
//                    fused or member-by-member warps, predicated copy, planar conversion): hf_interpolate_period is its n = 1 case
//   hf_batch.hip     hf_batch: the same calls for up to 32 contexts of one geometry as one set of launches (throughput drivers), and whole
//                    clips through a batch with the warp-or-copy decision taken on the device (hf_batch_run_period_auto, hf_scene.hip)
//   hf_metrics.hip   the four frame metrics on the device -- error sums, windowed SSIM, per-tile error maps, per-tile SSIM maps (hf_frame_error*,
//                    hf_frame_ssim*, hf_frame_error_map*, hf_frame_ssim_map*): their kernels, ONE frame layout and launcher tail on the host,
//                    ONE slot enqueue / read and ONE map shape / enqueue behind the ten calls
//   hf_async_io.hip  pinned asynchronous H2D / D2H on side streams (hf_update_frame_async: the H2D, then update_frames;
//                    hf_download_frame_async, hf_wait_*)
//
// Host orchestration restated from the reference's opticalFlowCalcSDR.cpp / opticalFlowCalcHDR.cpp (cited per function); the
// architecture differs on purpose:
//   * every uploaded frame is re-laid out once as mirror-padded phase planes, so the candidates of a run
//     of grid pixels are consecutive bytes (hf_flow.hip);
//   * offsets are kept per window in one small table per level, not per pixel;
//   * ONE launch per level (X and Y step fused) for windows <= 32, two per axis for larger windows
//     (reference: fill + calcDeltaSums + determineLowestLayer + adjustOffsetArray = 4 enqueues per step,
//     2.6-8.3 MB of fills);
//   * m_totalFrameDelta is produced on the device and copied to pinned memory inside the graph
//     (reference: blocking 4-byte readback in the middle of the chain, opticalFlowCalcSDR.cpp:91-94);
//   * the whole chain replays as one hipGraph, keyed by the scalars, the table mode and every context's ring / flow-buffer phase (ChainGraphs).
//
// OWNERSHIP, the one rule: a member or local of an owner type below (DevBuf, HostBuf, Stream, Event, GraphExec) is OURS -- created by the
// kind's helper, released when the owner goes; a raw pointer or handle is a VIEW of something an owner (or the caller) holds.  Nothing
// else in csrc/ creates or releases a device resource, but hf_device_malloc / hf_host_malloc_pinned and their frees (the caller's memory)
// and the timeline's process-lifetime reference events (hf_batch.hip g_tl_reference).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <shared_mutex>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/config.h"
#include "../../include/hopperflow.h"
#include "../../include/hopperflow_diag.h"
#include "hf_kernels.h"
#include "hf_scene.h"

namespace hfi {

constexpr int kMinSearchRadius = MIN_SEARCH_RADIUS;    // include/config.h (reference config.h:8)
constexpr int kMaxSearchRadius = MAX_SEARCH_RADIUS;    // config.h:9
constexpr int kCalcTimeInterval = CALC_TIME_INTERVAL;  // config.h:17
static_assert(kMaxSearchRadius <= 16, "the chain kernels keep 16 candidates per step in registers");
constexpr int kMaxSteps = 32;          // 2 * log2(max window)

extern std::shared_mutex g_capture_mutex;   // shared: a stream capture is in progress; exclusive: a legacy-stream copy (util_copy)

// ---- the owner types (the rule: top of this file).  Each kind has one creation helper, which returns the hipError_t and fills the owner
// only on success, and one stateless deleter; both count the kind in g_live (hf_debug_live_resources, hf_context.hip).  Nothing on a
// period's steady-state path creates or destroys a resource, so no hot call touches the counts. ----
enum LiveKind { kLiveDeviceBuffers, kLivePinnedBuffers, kLiveStreams, kLiveEvents, kLiveGraphExecs, kLiveKinds };
extern std::atomic<int64_t> g_live[kLiveKinds];
inline void count_live(LiveKind k, int64_t d) { g_live[k].fetch_add(d, std::memory_order_relaxed); }

template <LiveKind K, auto Release> struct Deleter { template <typename H> void operator()(H h) const { (void)Release(h); count_live(K, -1); } };
using FreeDevice = Deleter<kLiveDeviceBuffers, hipFree>;
template <typename T> using DevBuf = std::unique_ptr<T, FreeDevice>;                                    // device memory
template <typename T> using HostBuf = std::unique_ptr<T, Deleter<kLivePinnedBuffers, hipHostFree>>;   // pinned or mapped host memory
using Stream = std::unique_ptr<std::remove_pointer_t<hipStream_t>, Deleter<kLiveStreams, hipStreamDestroy>>;
using Event = std::unique_ptr<std::remove_pointer_t<hipEvent_t>, Deleter<kLiveEvents, hipEventDestroy>>;
using GraphExec = std::unique_ptr<std::remove_pointer_t<hipGraphExec_t>, Deleter<kLiveGraphExecs, hipGraphExecDestroy>>;

template <typename T>
hipError_t alloc_device(DevBuf<T>& out, size_t bytes) {
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess) { out.reset(static_cast<T*>(p)); count_live(kLiveDeviceBuffers, 1); }
    return e;
}
template <typename T>
hipError_t alloc_host(HostBuf<T>& out, size_t bytes, unsigned flags) {
    void* p = nullptr;
    const hipError_t e = hipHostMalloc(&p, bytes, flags);
    if (e == hipSuccess) { out.reset(static_cast<T*>(p)); count_live(kLivePinnedBuffers, 1); }
    return e;
}
// a non-blocking stream; priority: of that priority (hf_batch_create)
inline hipError_t create_stream(Stream& out, const int* priority = nullptr) {
    hipStream_t s = nullptr;
    const hipError_t e = priority ? hipStreamCreateWithPriority(&s, hipStreamNonBlocking, *priority) : hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    if (e == hipSuccess) { out.reset(s); count_live(kLiveStreams, 1); }
    return e;
}
inline hipError_t create_event(Event& out, unsigned flags = hipEventDefault) {
    hipEvent_t ev = nullptr;
    const hipError_t e = hipEventCreateWithFlags(&ev, flags);
    if (e == hipSuccess) { out.reset(ev); count_live(kLiveEvents, 1); }
    return e;
}
inline hipError_t instantiate_graph(GraphExec& out, hipGraph_t graph) {
    hipGraphExec_t x = nullptr;
    const hipError_t e = hipGraphInstantiate(&x, graph, nullptr, nullptr, 0);
    if (e == hipSuccess) { out.reset(x); count_live(kLiveGraphExecs, 1); }
    return e;
}
}  // namespace hfi

// The instantiated hipGraphs of the refinement chain of one context, or of one batch (hf_calc.hip calculate_flow).  What a capture bakes in,
// and why a replay is still right:
//   * in the key: search radius, delta and neighbour scalar (kernel arguments), the table mode (which kernels run), and per context
//     ring_phase * 2 + blur_phase -- which of its three phase planes are frames N-1 / N and which flow buffer the chain writes;
//   * constant for the context's life: iterations and blur radius (hf_config), HF_FLAG_NO_LAZY_ARGMIN, the levels and every device pointer but
//     the rotating ones above (tables, window sums, SAD tables, the mapped m_totalFrameDelta slot); a batch's members never change;
//   * clears the cache when it changes: the diagnostic counters pointer (hf_debug_counters_enable: the context's and its batch's) and the stream
//     of the capture (hf_batch_create / hf_batch_destroy).  The key is a fixed-size array: a lookup, every period of every stream, allocates nothing.
struct ChainGraphs {
    static constexpr size_t kMaxEntries = 96;     // bound of the cache (parameters poked by a settings UI): a full one starts over
    using Key = std::array<int, 4 + hf::kMaxFlowBatch>;   // R, delta scalar, neighbour scalar, table mode, then one phase per context, rest -1
    std::map<Key, hfi::GraphExec> map;
    hipGraphExec_t find(const Key& k) const { auto it = map.find(k); return it == map.end() ? nullptr : it->second.get(); }
    hipGraphExec_t insert(const Key& k, hfi::GraphExec exec) { if (map.size() >= kMaxEntries) clear(); return map.emplace(k, std::move(exec)).first->second.get(); }
    void clear() { map.clear(); }
};

struct hf_ctx {
    hf::Geom g{};
    hf_config cfg{};
    int device = 0;
    hipStream_t stream = nullptr;                      // stream the context issues on (a batch's shared stream while it is a member)
    hfi::Stream own_stream;                            // the stream this context created
    hipStream_t warp_stream = nullptr;                 // == stream unless HF_FLAG_DUAL_STREAM
    hfi::Stream own_warp_stream;                       // HF_FLAG_DUAL_STREAM: this context's second stream
    hfi::Event ev_chain_done, ev_warps_done;
    struct hf_batch* batch = nullptr;                  // the batch this context is a member of
    hfi::Event ev_flow[2];                             // recorded behind the chain that wrote blurred[i] (swapped with it)
    bool ev_flow_valid[2] = {false, false};
    bool dual() const { return (cfg.flags & HF_FLAG_DUAL_STREAM) != 0; }
    bool on_warp_stream = false;                       // warp stream currently ordered after `stream`
    std::string err;

    // public fields of the reference object (opticalFlowCalc.h:27-48)
    hf_params p{};
    uint32_t total_frame_delta = 0;
    double ofc_calc_time = 0, ofc_avg = 0, ofc_peak = 0, ofc_sum = 0, warp_calc_time = 0;
    int ofc_count = 0;

    // device memory (reference buffers: opticalFlowCalcSDR.cpp:272-280)
    size_t in_bytes = 0, out_bytes = 0, plane_elems = 0;
    void* ring[3] = {nullptr, nullptr, nullptr};       // m_inputFrameArray, ring[2] = newest: views of ring_store or of caller memory
    hfi::DevBuf<void> ring_store[3];                   // the context's own frame buffers, rotating with the ring
    hfi::DevBuf<uint32_t> pp[3];                       // phase plane of each ring frame (hf_flow.hip)
    bool plane_pending[3] = {false, false, false};     // deferred build (hf_batch_run_period): pp[i] holds only the grid samples so far
    hf::PhaseLayout pl{};
    hfi::DevBuf<void> out_frame;                       // m_outputFrameArray
    void* out_target = nullptr;                        // where warp/copy write (out_frame, an output-ring slot or the caller's)
    hfi::DevBuf<int16_t> tables;                       // per-level window offsets (replaces the per-pixel m_offsetArray); FlowLevel::tx / ty point into it
    size_t tables_bytes = 0;
    std::vector<hf::FlowLevel> levels;                 // level k = window size initial_window >> k
    hf::FlowLevel last_level{};                        // level the last chain ended on (tx == nullptr: no step ran)
    hfi::DevBuf<int16_t> off_view;                     // scratch [2][lh][lw] for hf_read_offsets
    hfi::DevBuf<int16_t> blurred[2];                   // m_blurredOffsetArray
    hfi::DevBuf<uint32_t> blurred_xy[2];               // the same flow packed x | y << 16 (fast warp path)
    hfi::DevBuf<uint32_t> sadtab;                      // SAD tables (hf_flow.hip): [2][sad_nby][sad_nbx][8] u16 pairs; empty: HF_FLAG_NO_SAD_REUSE
    size_t sadtab_bytes = 0;
    int sad_nbx = 0, sad_nby = 0;
    // Content hint of the SAD tables: how many windows of the 32-level chose d = 0 on both axes in the last chains (device counter, published
    // by the chain's last kernel into h_total_delta[1]); below ~30 % of them the tables cost more than they return and the chain runs without
    bool tab_mode = true;                              // the next chain keeps SAD tables
    float still_share = -1.f;                          // smoothed share of such windows (< 0: no chain has reported yet)
    hfi::DevBuf<uint32_t> still_count;
    hfi::DevBuf<uint32_t> counters;                    // diagnostic counters (hf_debug_counters_enable), device, hf::kCounterWords u32
    hfi::DevBuf<uint32_t> sums;                        // [kMaxSteps][n_windows_max][16]
    size_t sums_bytes = 0;
    size_t sums_stride = 0;                            // elements per step
    uint32_t* d_total_delta = nullptr;                 // device view of h_total_delta (mapped pinned memory)
    hfi::HostBuf<uint32_t> h_total_delta;              // pinned host slot the chain writes m_totalFrameDelta into
    hfi::DevBuf<float> d_probe;
    hfi::DevBuf<hf::FrameErrorSlot> error_slots;       // hf_frame_error* (hf_metrics.hip): HF_ERROR_SLOTS + 1 result slots, allocated on first use
    hfi::DevBuf<hf::FrameSsimSlot> ssim_slots;         // hf_frame_ssim* (hf_metrics.hip): HF_SSIM_SLOTS + 1 slots of their own, allocated on first use

    // asynchronous host I/O (hf_update_frame_async / hf_download_frame_async): side streams, created lazily and all at once (io_init)
    static constexpr int kOutRing = 3;
    hfi::Stream io_in, io_out;
    hfi::Event ev_h2d, ev_last_launch, ev_out_ready;
    hfi::Event ev_slot_prep[3];                                  // prep of ring_store[i] finished (rotates with the ring)
    hfi::Event ev_d2h[kOutRing];
    bool d2h_pending[kOutRing] = {false, false, false};
    hfi::DevBuf<void> out_ring[kOutRing];                        // output-ring slots 1 and 2; slot 0 is out_frame and [0] stays empty: out_at()
    void* out_at(int i) const { return i ? out_ring[i].get() : out_frame.get(); }
    int out_idx = 0;
    bool have_last_launch = false;
    // completion of the asynchronous readbacks, for streaming hosts (hf_wait_download): one event per download, ring of kDlRing
    static constexpr int kDlRing = 64;
    hfi::Event ev_dl[kDlRing];
    uint64_t dl_issued = 0;
    hfi::Event ev_flow_done;                           // behind the last chain of an asynchronous context (hf_wait_flow)
    bool flow_done_recorded = false;

    // planar frames at the boundary (HF_FLAG_PLANAR_IN / _OUT, hf_planar.hip); every buffer is allocated on first use
    hfi::DevBuf<void> in_stage[3];                               // planar host frames land here (rotates with ring_store / ev_slot_prep)
    hfi::DevBuf<void> out_stage[kOutRing];                       // planar frames the readbacks read ([i] paired with output-ring slot i)
    std::vector<hfi::DevBuf<void>> period_stage;                 // semi-planar targets of a period's warps where its output side is planar
                                                                 // (ensure_period_stages: kMaxWarpOutputs at the most, reused chunk by chunk)
    bool planar_in() const { return (cfg.flags & HF_FLAG_PLANAR_IN) != 0; }
    bool planar_out() const { return (cfg.flags & HF_FLAG_PLANAR_OUT) != 0; }

    int ring_phase = 0;   // number of rotations mod 3 (graph key)
    int blur_phase = 0;   // number of swaps mod 2
    bool have_flow = false;
    bool delta_pending = false;
    int last_iterations = 0, initial_window = 0;

    // timing (reference spans: opticalFlowCalcSDR.cpp:36-41,119-127)
    hfi::Event ev_upload, ev_flow_end, ev_warp_start, ev_warp_end;
    hfi::Event ev_user0, ev_user1;
    bool upload_recorded = false, flow_timing_pending = false, warp_started = false;

    ChainGraphs graphs;

    // HF_FLAG_PROFILE: event pairs around warp / copy / flow-chain launches
    struct Span { hfi::Event b, e; int kind; hipStream_t stream; int frames = 1; };
    std::vector<hfi::Event> ev_pool;
    std::vector<Span> spans;
    hf_profile prof{};
    int prof_every[3] = {1, 1, 1};   // sampling interval per span kind (warp, copy, flow chain)
    unsigned prof_seen[3] = {0, 0, 0};
    bool profiling() const { return (cfg.flags & HF_FLAG_PROFILE) != 0; }

    bool async() const { return (cfg.flags & HF_FLAG_ASYNC) != 0; }
    bool timing() const { return (cfg.flags & HF_FLAG_NO_TIMING) == 0; }   // record the reference's timing events
};

// Per-launch device timestamps of a batch (hf_batch_timeline_*): the start / stop events of every dispatch the batch issues while it is on.
struct hf_timeline final : hf::LaunchObserver {
    struct Rec { const char* name; hipEvent_t b, e; int period; };
    std::vector<Rec> recs;
    std::vector<hfi::Event> events;      // 2 per record, created when the timeline is switched on
    hfi::Event anchor;                   // recorded when it is switched on: the records are read against it, it against the process's reference
    double anchor_ms = 0.0;
    size_t capacity = 0;
    int skip = 0;                        // hf_batch_run_period calls still to pass unobserved before the recording starts
    bool active = false;                 // records left: hf_batch_run_period observes its launches and issues the chain eagerly (no graph replay)
    int period = 0;                      // hf_batch_run_period calls since it was switched on
    uint64_t dropped = 0;                // launches issued while on but out of records (cannot happen: it switches itself off when full)
    bool next(const char* name, hipEvent_t* s, hipEvent_t* e) override {
        if (recs.size() >= capacity) { dropped++; return false; }
        *s = events[2 * recs.size()].get(); *e = events[2 * recs.size() + 1].get();
        recs.push_back(Rec{name, *s, *e, period});
        return true;
    }
};

// ---- batches (throughput drivers; include/hopperflow.h) ----
struct hf_batch {
    hf_timeline tl;
    std::vector<hf_ctx*> members;
    std::vector<hipStream_t> own_streams;   // views of the members' own streams, restored by hf_batch_destroy
    std::vector<hipStream_t> own_warp_streams;
    std::vector<hfi::Stream> warp_streams;  // HF_FLAG_DUAL_STREAM members: shared streams their warps are issued on
    hfi::Stream stream;                     // the batch's own (highest-priority) stream, shared by all members while the batch exists
    ChainGraphs graphs;
    bool defer_planes = false;              // hf_batch_run_period: grid samples at update, full plane of frame N-1 from the warp launch
    bool auto_deferred = false;             // ... and hf_batch_run_period_auto too: the leader's HF_FLAG_BATCH_AUTO_DEFERRED on a batch that defers
    // planar 4:2:0 frames at the batch's boundary (the leader's HF_FLAG_BATCH_PLANAR_IN / _OUT; hf_planar.hip): new frames are converted
    // into the members' ring slots, caller-owned outputs out of the members' period_stage frames, by one launch each
    bool planar_in = false, planar_out = false;
    // hf_batch_run_period_auto (hf_scene.hip): allocated by the first hf_batch_scene_set
    static constexpr uint32_t kSceneRing = 128;          // records a member can hold between two hf_batch_scene_read calls
    struct SceneMember {
        bool armed = false, clear = false;  // clear: (re-)armed since its last period -- the next scene_decide launch starts its history over
        int cap = 0;                        // hf::scene_history_cap(source_frame_time)
        uint32_t threshold = 0;
        uint64_t written = 0, read = 0;     // records appended / handed out so far (slot = index % kSceneRing)
    };
    std::vector<SceneMember> scene;
    hfi::DevBuf<hf::SceneState> scene_states;   // device [kMaxFlowBatch]
    hfi::DevBuf<int32_t> scene_kinds;           // device [kMaxFlowBatch]: 1 warp / 0 copy of the period in flight
    hfi::HostBuf<hf::SceneRecord> scene_records;   // mapped host memory [kMaxFlowBatch][kSceneRing] ...
    hf::SceneRecord* scene_records_dev = nullptr;  // ... and its device view
    std::string err;
};

namespace hfi {

// hf_context.hip
int fail(hf_ctx* c, int code, const char* fmt, ...);
int set_device(hf_ctx* c);
int initial_window(int lw, int lh);
int ilog2(int v);
int effective_iterations(const hf_ctx* c);
Event pool_event(hf_ctx* c);
int span_begin(hf_ctx* c, int kind, hipStream_t stream = nullptr);
int span_open(hf_ctx* c, int kind);
void span_end(hf_ctx* c, int idx);
void span_cancel(hf_ctx* c, int idx);
void collect_spans(hf_ctx* c);
int sync_ctx(hf_ctx* c);
int util_copy(int device_index, void* dst, const void* src, size_t bytes, hipMemcpyKind kind);

// hf_calc.hip
int enqueue_flow_chain(const hf_ctx* const* cs, int n, hipStream_t s);
int calculate_flow(hf_ctx* const* cs, int n, hipStream_t s, ChainGraphs* graphs, bool warmup_keeps_flow);
bool choose_tab_mode(hf_ctx* const* cs, int n);
int ensure_older_planes(hf_ctx* const* cs, int n, hipStream_t s);
void finish_flow_timing(hf_ctx* c);
int enter_warp_stream(hf_ctx* c);
int leave_warp_stream(hf_ctx* c);
// how the new frames of an update arrive: a host or device frame to copy, a device frame to reference, or a frame the caller's H2D on the
// context's io_in stream has put into its slot already (ev_h2d recorded behind it)
enum class FrameSource { Host, Device, DeviceRef, Staged };
int update_frames(hf_batch* b, hf_ctx* const* cs, int n, const void* const* src, FrameSource how, bool planar, bool defer, const char* who);
int check_flow_params(hf_ctx* c);
int after_flow_enqueued(hf_ctx* c, hipStream_t s);
int check_period_args(hf_ctx* c, const char* who, int n_out, int max_n_out, const float* t, int mode);
struct OutputLevels { float black, white; };
OutputLevels output_levels(const hf_ctx* c);
void* copy_source(const hf_ctx* c);
int ensure_period_stages(hf_ctx* c, int n);
int interpolate_period(hf_batch* b, hf_ctx* const* cs, int n, int row, const int* n_out, const float* t, void* const* device_out, int mode,
                       bool before_chain = false, bool* launched = nullptr, hf::SceneCopyArgs* copy = nullptr, int first_chunk = 0,
                       int first_parts = hf::kPartsAll);
int download_common(hf_ctx* c, void* dst, hipMemcpyKind kind);

// hf_batch.hip
int batch_fail(hf_batch* b, int code, const std::string& msg);
int batch_update(hf_batch* b, const void* const* device_frames, bool defer);
int batch_check_flow_params(hf_batch* b);
int batch_calculate(hf_batch* b, bool warmup_keeps_flow);
int batch_interpolate(hf_batch* b, int row, const int* n_out, const float* t, void* const* device_out, int mode, bool before_chain, bool* launched,
                      hf::SceneCopyArgs* copy = nullptr, int first_chunk = 0, int first_parts = hf::kPartsAll);

// hf_async_io.hip
int io_init(hf_ctx* c);
int ensure_in_stage(hf_ctx* c);
int ensure_out_stage(hf_ctx* c);
int out_slot(const hf_ctx* c, const void* target);
int guard_output_slot(hf_ctx* c, const void* target, hipStream_t launch_stream);
int note_launch(hf_ctx* c, hipStream_t launch_stream);

}  // namespace hfi

#define HF_HIP(c, call)                                                                              \
    do {                                                                                             \
        hipError_t _e = (call);                                                                      \
        if (_e != hipSuccess)                                                                        \
            return fail((c), _e == hipErrorOutOfMemory ? HF_ERR_OUT_OF_MEMORY : HF_ERR_HIP,          \
                        "HIP error %d (%s) in %s at %s:%d", (int)_e, hipGetErrorString(_e), #call,  \
                        __FILE__, __LINE__);                                                         \
    } while (0)

#define HF_CHECK_CTX(c) \
    if (!(c)) return fail(nullptr, HF_ERR_INVALID_ARGUMENT, "null context")
