// hopperrender_amd/csrc/hf_batch.hip -- hf_batch (include/hopperflow.h): up to 32 contexts of identical geometry and parameters issue their
// phase planes, refinement chains and fused period warps as ONE set of launches on one stream (independent frame pairs);
// results per member are those of the single-context calls of hf_calc.hip, whose host paths (update_frames, calculate_flow,
// interpolate_period) issue them.  Here is what is a batch's own: argument checks, streams, timeline, scene state.  Layout of the ABI: hf_ctx.h.

#include "hf_ctx.h"

using namespace hfi;

static thread_local std::string g_batch_error;

namespace hfi {

int batch_fail(hf_batch* b, int code, const std::string& msg) {
    (b ? b->err : g_batch_error) = "[HopperRender] " + msg;
    return code;
}

// hf_batch_update_frames_device_ref: update_frames (hf_calc.hip, which states defer) over the members, their frames referenced -- or, planar,
// converted into the members' own slots
int batch_update(hf_batch* b, const void* const* device_frames, bool defer) {
    if (!b) return batch_fail(nullptr, HF_ERR_INVALID_ARGUMENT, "null batch");
    if (!device_frames) return batch_fail(b, HF_ERR_INVALID_ARGUMENT, "hf_batch_update_frames_device_ref: null argument");
    if (hipSetDevice(b->members[0]->device) != hipSuccess) return batch_fail(b, HF_ERR_HIP, "hipSetDevice failed");
    return update_frames(b, b->members.data(), (int)b->members.size(), device_frames, FrameSource::DeviceRef, b->planar_in, defer,
                         "hf_batch_update_frames_device_ref");
}

// What hf_batch_calculate_optical_flow checks before it enqueues anything: valid flow parameters, equal in all members.
int batch_check_flow_params(hf_batch* b) {
    hf_ctx* l = b->members[0];
    for (hf_ctx* m : b->members) {
        if (int rc = check_flow_params(m)) return batch_fail(b, rc, m->err);
        if (m->p.search_radius != l->p.search_radius || m->p.delta_scalar != l->p.delta_scalar || m->p.neighbor_scalar != l->p.neighbor_scalar)
            return batch_fail(b, HF_ERR_INVALID_ARGUMENT, "hf_batch_calculate_optical_flow: members differ in search radius / delta / neighbor scalar");
    }
    return HF_OK;
}

// HF_FLAG_BATCH_PLANAR_OUT: every member's stages for its n_out (hf_calc.hip ensure_period_stages).  Allocates, so a call runs it before
// its first enqueue; an n_out outside [0, row] is left to the check that reports it.
int batch_ensure_out_stages(hf_batch* b, int row, const int* n_out) {
    if (!b->planar_out || !n_out) return HF_OK;
    if (hipSetDevice(b->members[0]->device) != hipSuccess) return batch_fail(b, HF_ERR_HIP, "hipSetDevice failed");
    for (size_t m = 0; m < b->members.size(); m++)
        if (ensure_period_stages(b->members[m], n_out[m] > row ? 0 : n_out[m])) {
            (void)hipGetLastError();
            return batch_fail(b, HF_ERR_OUT_OF_MEMORY, "cannot allocate a planar output stage");
        }
    return HF_OK;
}

// The warps of one source period of every member: what a batch refuses, all of it before the first enqueue, then interpolate_period
// (hf_calc.hip), which states before_chain, launched, copy, first_chunk and first_parts.  t and device_out are [batch size][row] arrays.
int batch_interpolate(hf_batch* b, int row, const int* n_out, const float* t, void* const* device_out, int mode, bool before_chain, bool* launched,
                      hf::SceneCopyArgs* copy, int first_chunk, int first_parts) {
    if (launched) *launched = false;
    if (!b) return batch_fail(nullptr, HF_ERR_INVALID_ARGUMENT, "null batch");
    if (!n_out || !t || !device_out) return batch_fail(b, HF_ERR_INVALID_ARGUMENT, "hf_batch_interpolate_period: null argument");
    hf_ctx* l = b->members[0];
    const int n = (int)b->members.size();
    if (int rc = check_period_args(l, "hf_batch_interpolate_period", 0, -1, nullptr, mode)) return batch_fail(b, rc, l->err);   // the mode, ahead of all else
    if (row < 1 || row > HF_MAX_PERIOD_OUTPUTS_WIDE)
        return batch_fail(b, HF_ERR_INVALID_ARGUMENT, "hf_batch_interpolate_period: row outside [1, " + std::to_string(HF_MAX_PERIOD_OUTPUTS_WIDE) + "]");
    if (hipSetDevice(l->device) != hipSuccess) return batch_fail(b, HF_ERR_HIP, "hipSetDevice failed");
    for (int m = 0; m < n; m++) {
        hf_ctx* c = b->members[m];
        if (!c) return batch_fail(b, HF_ERR_INVALID_ARGUMENT, "null context");
        if (c->io_in) return batch_fail(b, HF_ERR_STATE, "hf_batch_interpolate_period: a member uses asynchronous host I/O");
        if (int rc = check_period_args(c, "hf_batch_interpolate_period", n_out[m], row, t + (size_t)m * row, mode)) return batch_fail(b, rc, c->err);
    }
    if (int rc = batch_ensure_out_stages(b, row, n_out)) return rc;   // (the stages: allocated before anything of this call is enqueued)
    static_assert(hf::kMaxPeriodOutputsWide == HF_MAX_PERIOD_OUTPUTS_WIDE && hf::kMaxWarpOutputs == HF_MAX_PERIOD_OUTPUTS, "the header's limits are the plan's");
    return interpolate_period(b, b->members.data(), n, row, n_out, t, device_out, mode, before_chain, launched, copy, first_chunk, first_parts);
}

// the launches a period of `chunks` chunks adds to a one-chunk period's: per further chunk up to two fused warp launches (17 members and
// more), the predicated copy and the planar conversion
int timeline_reserve(int chunks) { return 32 + (chunks > 1 ? 4 * (chunks - 1) : 0); }

namespace {
// timeline on: every launch of a period call carries its own start / stop events (hf_kernels.h HF_LAUNCH)
struct ObserverGuard {
    hf_batch* b;
    // chunks: of the period about to be issued (plan_period_chunks).  The end of the last period left room for a one-chunk period; a wider one
    // needs timeline_reserve(chunks) free records, or the recording ends here
    explicit ObserverGuard(hf_batch* x, int chunks = 1) : b(nullptr) {
        if (!x->tl.active) return;
        if (x->tl.skip > 0) { x->tl.skip--; return; }      // armed, not recording yet
        if (chunks > 1 && x->tl.recs.size() + (size_t)timeline_reserve(chunks) > x->tl.capacity) { x->tl.active = false; return; }
        b = x;
        hf::t_launch_observer = &b->tl;
    }
    ~ObserverGuard() {
        if (!b) return;
        hf::t_launch_observer = nullptr;
        b->tl.period++;
        if (b->tl.recs.size() + 32 > b->tl.capacity) b->tl.active = false;   // no room for another whole period: back to graph replays
    }
};
}  // namespace

}  // namespace hfi

extern "C" {

const char* hf_batch_last_error(const hf_batch* b) { return b ? b->err.c_str() : g_batch_error.c_str(); }

int hf_batch_create(hf_ctx* const* members, int n, hf_batch** out) {
    if (!members || !out || n < 1) return batch_fail(nullptr, HF_ERR_INVALID_ARGUMENT, "hf_batch_create: bad argument");
    *out = nullptr;
    if (n > hf::kMaxFlowBatch) return batch_fail(nullptr, HF_ERR_INVALID_ARGUMENT, "hf_batch_create: at most " + std::to_string(hf::kMaxFlowBatch) + " members");
    hf_ctx* l = members[0];
    for (int i = 0; i < n; i++) {
        hf_ctx* m = members[i];
        if (!m) return batch_fail(nullptr, HF_ERR_INVALID_ARGUMENT, "hf_batch_create: null member");
        if (m->planar_in() || m->planar_out())
            return batch_fail(nullptr, HF_ERR_INVALID_ARGUMENT, "hf_batch_create: HF_FLAG_PLANAR_IN / HF_FLAG_PLANAR_OUT contexts cannot join a batch");
        for (int j = 0; j < i; j++) if (members[j] == m) return batch_fail(nullptr, HF_ERR_INVALID_ARGUMENT, "hf_batch_create: duplicate member");
        if (m->batch) return batch_fail(nullptr, HF_ERR_STATE, "hf_batch_create: member " + std::to_string(i) + " already belongs to a batch");
        const hf::Geom &a = l->g, &b = m->g;
        const bool same = a.hdr == b.hdr && a.H == b.H && a.W == b.W && a.in_stride == b.in_stride && a.out_stride == b.out_stride &&
                          a.rs == b.rs && m->device == l->device && m->cfg.iterations == l->cfg.iterations &&
                          m->cfg.blur_radius == l->cfg.blur_radius && !m->sadtab == !l->sadtab;
        if (!same) return batch_fail(nullptr, HF_ERR_INVALID_ARGUMENT, "hf_batch_create: members differ in geometry, device, iterations, blur radius or HF_FLAG_NO_SAD_REUSE");
        if (!m->async() || m->io_in || m->dual() != l->dual())
            return batch_fail(nullptr, HF_ERR_INVALID_ARGUMENT, "hf_batch_create: members must be HF_FLAG_ASYNC contexts (all single-stream or all HF_FLAG_DUAL_STREAM) without async host I/O");
    }
    // planar frames at the batch's boundary: the leader's flags, like HF_FLAG_BATCH_EAGER_PLANES
    const bool planar_in = (l->cfg.flags & HF_FLAG_BATCH_PLANAR_IN) != 0, planar_out = (l->cfg.flags & HF_FLAG_BATCH_PLANAR_OUT) != 0;
    if ((planar_in && (l->g.in_stride & 1)) || (planar_out && (l->g.out_stride & 1)))
        return batch_fail(nullptr, HF_ERR_INVALID_ARGUMENT, "hf_batch_create: a planar side needs an even stride (input " + std::to_string(l->g.in_stride) +
                                                            ", output " + std::to_string(l->g.out_stride) + ")");
    if ((planar_in || planar_out) && l->dual())
        return batch_fail(nullptr, HF_ERR_INVALID_ARGUMENT, "hf_batch_create: HF_FLAG_BATCH_PLANAR_IN / HF_FLAG_BATCH_PLANAR_OUT with HF_FLAG_DUAL_STREAM members: "
                                                            "their warps run beside the batch stream, which the conversion launches are ordered on");
    if (hipSetDevice(l->device) != hipSuccess) return batch_fail(nullptr, HF_ERR_HIP, "hf_batch_create: hipSetDevice failed");
    for (int i = 0; i < n; i++)   // before any member is touched: a failure leaves every context as it was
        if (int rc = sync_ctx(members[i])) return batch_fail(nullptr, rc, "hf_batch_create: member sync failed: " + members[i]->err);
    std::unique_ptr<hf_batch> b(new (std::nothrow) hf_batch());   // (its streams: built here, before any member is touched; all or nothing)
    if (!b) return batch_fail(nullptr, HF_ERR_OUT_OF_MEMORY, "hf_batch_create: host allocation failed");
    // A stream of the batch's own, of the HIGHEST priority.  Not for the priority: the runtime keeps one pool of hardware queues
    // per priority level and hands a new stream the queue of its pool with the fewest users.  The members' streams (and
    // everybody else's) are normal-priority ones, so the batch streams of a process are alone in their pool and the first
    // GPU_MAX_HW_QUEUES of them sit on different hardware queues whatever was created before.  (With the leader's stream, two
    // batches whose leaders were 32 streams apart shared ONE queue and ran strictly one after the other: 64 x 32 at 103 k
    // instead of 115 k frames/s; a normal-priority stream of the batch's own did the same at 48 x 24.)
    // Side effect (include/hopperflow.h): the priority is real -- batch work is scheduled ahead of the normal-priority streams
    // of the process.  HF_FLAG_BATCH_NORMAL_PRIORITY on the leader opts out (and gives up the private queue pool).
    {
        int prio_low = 0, prio_high = 0;
        const bool want_high = !(l->cfg.flags & HF_FLAG_BATCH_NORMAL_PRIORITY) && hipDeviceGetStreamPriorityRange(&prio_low, &prio_high) == hipSuccess;
        if (!want_high || create_stream(b->stream, &prio_high) != hipSuccess) {
            (void)hipGetLastError();
            if (create_stream(b->stream) != hipSuccess) return batch_fail(nullptr, HF_ERR_HIP, "hf_batch_create: cannot create the batch stream");
        }
    }
    if (l->dual()) {
        // the members' warps go to a few shared streams (round robin) instead of one stream per member: the device
        // runs only a handful of hardware queues side by side (DESIGN.md "Hardware queues")
        const int nws = n < 3 ? n : 3;
        for (int i = 0; i < nws; i++) {
            Stream ws;
            if (create_stream(ws) != hipSuccess) return batch_fail(nullptr, HF_ERR_HIP, "hf_batch_create: cannot create a warp stream");
            b->warp_streams.push_back(std::move(ws));
        }
    }
    for (int i = 0; i < n; i++) {
        hf_ctx* m = members[i];
        b->members.push_back(m);
        b->own_streams.push_back(m->stream);
        b->own_warp_streams.push_back(m->warp_stream);
        // one stream for the whole batch: the members' prep / warp launches and the batched chain stay in program order
        m->graphs.clear();   // captured on the member's own stream
        m->stream = b->stream.get();
        m->warp_stream = m->dual() ? b->warp_streams[(size_t)i % b->warp_streams.size()].get() : b->stream.get();
        m->batch = b.get();
    }
    // Deferred phase planes: where the batched period warp is the workgroup-staged kernel it can build the full plane of the frame
    // it reads anyway (plane-building workgroups of warp_wg_kernel, hf_kernels.hip); hf_batch_run_period then only samples the grid
    // at update time.
    b->defer_planes = !l->dual() && !(l->cfg.flags & HF_FLAG_BATCH_EAGER_PLANES) && hf::warp_period_can_build_planes(l->g, l->pl, n);
    for (int i = 0; i < n; i++) b->defer_planes = b->defer_planes && !(members[i]->cfg.flags & HF_FLAG_NO_FUSED_WARP);
    // ... and hf_batch_run_period_auto keeps that order where the leader asks for it (hf_launch_plan.h plan_auto_period)
    b->auto_deferred = b->defer_planes && (l->cfg.flags & HF_FLAG_BATCH_AUTO_DEFERRED) != 0;
    b->planar_in = planar_in;
    b->planar_out = planar_out;
    *out = b.release();
    return HF_OK;
}

void hf_batch_destroy(hf_batch* b) {
    if (!b) return;
    if (!b->members.empty()) hipSetDevice(b->members[0]->device);
    for (hf_ctx* m : b->members) leave_warp_stream(m);   // the batch stream waits for every member's last warps
    if (b->stream) hipStreamSynchronize(b->stream.get());
    for (const Stream& ws : b->warp_streams) hipStreamSynchronize(ws.get());
    // Nothing of the batch is in flight from here on: the order in which its owners (streams, timeline events, scene state) go does not matter.
    b->graphs.clear();
    for (size_t i = 0; i < b->members.size(); i++) {
        hf_ctx* m = b->members[i];
        m->graphs.clear();
        if (b->planar_out) m->period_stage.clear();   // the stages of the batch's planar outputs
        m->stream = b->own_streams[i];
        m->warp_stream = b->own_warp_streams[i];
        m->on_warp_stream = false;
        m->batch = nullptr;
    }
    delete b;
}

int hf_batch_update_frames_device_ref(hf_batch* b, const void* const* device_frames) { return batch_update(b, device_frames, false); }

}  // extern "C"

namespace hfi {

// hf_batch_calculate_optical_flow: calculate_flow (hf_calc.hip) of the members on the batch's stream; HF_FLAG_NO_GRAPH of a member does not count.
// Under the timeline the chain goes out launch by launch, each with the events of its own dispatch (a graph replay has no per-node timestamps).
int batch_calculate(hf_batch* b, bool warmup_keeps_flow) {
    if (!b) return batch_fail(nullptr, HF_ERR_INVALID_ARGUMENT, "null batch");
    hf_ctx* l = b->members[0];
    if (hipSetDevice(l->device) != hipSuccess) return batch_fail(b, HF_ERR_HIP, "hipSetDevice failed");
    if (int rc = batch_check_flow_params(b)) return rc;
    const bool observed = hf::t_launch_observer == &b->tl;
    if (int rc = calculate_flow(b->members.data(), (int)b->members.size(), b->stream.get(), observed ? nullptr : &b->graphs, warmup_keeps_flow))
        return batch_fail(b, rc == HF_ERR_OUT_OF_MEMORY ? HF_ERR_HIP : rc, l->err);   // (a batch has always reported a HIP error of its chain as HF_ERR_HIP)
    return HF_OK;
}

}  // namespace hfi

extern "C" {

int hf_batch_calculate_optical_flow(hf_batch* b) { return batch_calculate(b, false); }

int hf_batch_size(const hf_batch* b) { return b ? (int)b->members.size() : 0; }

}  // extern "C"

namespace hfi {

// hf_batch_run_period / hf_batch_run_period_wide: t and device_out are [batch size][row] arrays
int batch_run_period(hf_batch* b, const void* const* device_frames, int calculate_flow, int row, const int* n_out, const float* t,
                     void* const* device_out, int mode) {
    if (!b) return batch_fail(nullptr, HF_ERR_INVALID_ARGUMENT, "null batch");
    if (row < 1 || row > HF_MAX_PERIOD_OUTPUTS_WIDE)   // (not an argument of the three separate calls' update or chain: refused before either)
        return batch_fail(b, HF_ERR_INVALID_ARGUMENT, "hf_batch_run_period: row outside [1, " + std::to_string(HF_MAX_PERIOD_OUTPUTS_WIDE) + "]");
    if (int rc = batch_ensure_out_stages(b, row, n_out)) return rc;   // (allocation: ahead of the first enqueue)
    const int chunks = n_out ? hf::plan_period_chunks((int)b->members.size(), n_out).n_chunks : 0;
    ObserverGuard observer_guard(b, chunks);
    if (device_frames) if (int rc = batch_update(b, device_frames, b->defer_planes)) return rc;
    // Deferred phase planes: a period whose older frame still lacks its full plane issues its warps FIRST (they do not depend on
    // this period's chain) and lets that launch build the plane; same results as the order of the three calls.  Of a period of several
    // chunks only chunk 0, which holds every member, goes first.
    bool warped = false;
    if (n_out && calculate_flow && b->defer_planes && mode >= 0 && mode <= 2) {
        // The early warps must not write the caller's output buffers in a period whose flow calculation is going to be refused: the three
        // separate calls would have stopped at the chain, before any warp.  So the chain's own argument checks come first.
        if (int rc = batch_check_flow_params(b)) return rc;
        bool pending = false;
        for (hf_ctx* m : b->members) pending = pending || m->plane_pending[1];
        // (an argument error of this early attempt -- nothing enqueued, `warped` false -- is not reported here: the period then takes the usual
        //  order below, which reports the same error where the three separate calls would, after the update and the chain; a launch that was
        //  enqueued and failed is reported at once)
        if (pending) if (int rc = batch_interpolate(b, row, n_out, t, device_out, mode, true, &warped)) { if (warped) return rc; }
    }
    if (calculate_flow) if (int rc = hf_batch_calculate_optical_flow(b)) return rc;
    if (n_out && (!warped || chunks > 1)) if (int rc = batch_interpolate(b, row, n_out, t, device_out, mode, false, nullptr, nullptr, warped ? 1 : 0)) return rc;
    return HF_OK;
}

}  // namespace hfi

extern "C" {

int hf_batch_interpolate_period(hf_batch* b, const int* n_out, const float* t, void* const* device_out, int mode) {
    return batch_interpolate(b, HF_MAX_PERIOD_OUTPUTS, n_out, t, device_out, mode, false, nullptr);
}

int hf_batch_interpolate_period_wide(hf_batch* b, int row, const int* n_out, const float* t, void* const* device_out, int mode) {
    return batch_interpolate(b, row, n_out, t, device_out, mode, false, nullptr);
}

int hf_batch_run_period(hf_batch* b, const void* const* device_frames, int calculate_flow, const int* n_out, const float* t,
                        void* const* device_out, int mode) {
    return batch_run_period(b, device_frames, calculate_flow, HF_MAX_PERIOD_OUTPUTS, n_out, t, device_out, mode);
}

int hf_batch_run_period_wide(hf_batch* b, const void* const* device_frames, int calculate_flow, int row, const int* n_out, const float* t,
                             void* const* device_out, int mode) {
    return batch_run_period(b, device_frames, calculate_flow, row, n_out, t, device_out, mode);
}

int hf_batch_defers_planes(const hf_batch* b) { return b && b->defer_planes ? 1 : 0; }

int hf_batch_planar(const hf_batch* b) { return b ? (b->planar_in ? 1 : 0) | (b->planar_out ? 2 : 0) : 0; }

// ---- timeline: start / stop of every dispatch of a batch on the device's clock, no profiler attached ----
namespace {
std::mutex g_tl_mutex;
// per device: the zero of every batch's timeline in this process.  The one deliberate exception to hf_ctx.h's ownership rule: the events
// live as long as the process, so they stay raw, are never released and are not counted by hf_debug_live_resources.
std::map<int, hipEvent_t> g_tl_reference;
}
int hf_batch_timeline_enable(hf_batch* b, int max_launches, int skip_periods) {
    if (!b) return batch_fail(nullptr, HF_ERR_INVALID_ARGUMENT, "null batch");
    hf_ctx* l = b->members[0];
    if (hipSetDevice(l->device) != hipSuccess) return batch_fail(b, HF_ERR_HIP, "hipSetDevice failed");
    if (max_launches < 0 || max_launches > (1 << 20) || skip_periods < 0 || (max_launches > 0 && max_launches < 32))
        return batch_fail(b, HF_ERR_INVALID_ARGUMENT, "hf_batch_timeline_enable: max_launches must be 0 or in [32, 2^20] (a period needs up to 32 free records), skip_periods >= 0");
    if (hipStreamSynchronize(b->stream.get()) != hipSuccess) return batch_fail(b, HF_ERR_HIP, "hipStreamSynchronize failed");
    b->tl.active = false;
    b->tl.recs.clear();
    b->tl.period = 0;
    b->tl.dropped = 0;
    b->tl.capacity = 0;
    if (max_launches == 0) {
        b->tl.events.clear();
        return HF_OK;
    }
    {
        std::lock_guard<std::mutex> lock(g_tl_mutex);
        if (!g_tl_reference.count(l->device)) {
            Event ref;   // an owner until it is recorded, so that a failure releases it; then the process's (release(): uncounted from there on)
            if (create_event(ref) != hipSuccess || hipEventRecord(ref.get(), b->stream.get()) != hipSuccess || hipEventSynchronize(ref.get()) != hipSuccess)
                return batch_fail(b, HF_ERR_HIP, "hf_batch_timeline_enable: cannot record the reference event");
            g_tl_reference[l->device] = ref.release();
            count_live(kLiveEvents, -1);
        }
        // This recording's own anchor on the reference's clock.  hipEventElapsedTime is a float: minutes after the reference it resolves
        // tens of microseconds, so a record is read against the anchor (a short, exact span) and only the anchor against the reference.
        float anchor_ms = 0.f;
        if ((!b->tl.anchor && create_event(b->tl.anchor) != hipSuccess) || hipEventRecord(b->tl.anchor.get(), b->stream.get()) != hipSuccess ||
            hipEventSynchronize(b->tl.anchor.get()) != hipSuccess || hipEventElapsedTime(&anchor_ms, g_tl_reference[l->device], b->tl.anchor.get()) != hipSuccess)
            return batch_fail(b, HF_ERR_HIP, "hf_batch_timeline_enable: cannot record the anchor event");
        b->tl.anchor_ms = (double)anchor_ms;
    }
    while (b->tl.events.size() < 2 * (size_t)max_launches) {
        Event e;
        if (create_event(e) != hipSuccess) return batch_fail(b, HF_ERR_OUT_OF_MEMORY, "hf_batch_timeline_enable: hipEventCreate failed");
        b->tl.events.push_back(std::move(e));
    }
    b->tl.recs.reserve((size_t)max_launches);
    b->tl.capacity = (size_t)max_launches;
    b->tl.skip = skip_periods;
    b->tl.active = true;
    return HF_OK;
}

int hf_batch_timeline_read(hf_batch* b, hf_timeline_record* out, int capacity, int* n_records) {
    if (!b) return batch_fail(nullptr, HF_ERR_INVALID_ARGUMENT, "null batch");
    if (!n_records || (capacity > 0 && !out)) return batch_fail(b, HF_ERR_INVALID_ARGUMENT, "hf_batch_timeline_read: null argument");
    hf_ctx* l = b->members[0];
    if (hipSetDevice(l->device) != hipSuccess) return batch_fail(b, HF_ERR_HIP, "hipSetDevice failed");
    if (hipStreamSynchronize(b->stream.get()) != hipSuccess) return batch_fail(b, HF_ERR_HIP, "hipStreamSynchronize failed");
    for (const Stream& ws : b->warp_streams)      // HF_FLAG_DUAL_STREAM members: the per-member warps of an observed period run there
        if (hipStreamSynchronize(ws.get()) != hipSuccess) return batch_fail(b, HF_ERR_HIP, "hipStreamSynchronize (warp stream) failed");
    hipEvent_t ref = nullptr;
    {
        std::lock_guard<std::mutex> lock(g_tl_mutex);
        auto it = g_tl_reference.find(l->device);
        if (it != g_tl_reference.end()) ref = it->second;
    }
    *n_records = (int)b->tl.recs.size();
    if (!ref) return b->tl.recs.empty() ? HF_OK : batch_fail(b, HF_ERR_STATE, "hf_batch_timeline_read: no reference event");
    const int n = *n_records < capacity ? *n_records : capacity;
    for (int i = 0; i < n; i++) {
        const hf_timeline::Rec& r = b->tl.recs[(size_t)i];
        float t0 = 0.f, t1 = 0.f, d = 0.f;
        hf_timeline_record& o = out[i];
        std::memset(&o, 0, sizeof(o));
        std::strncpy(o.kernel, r.name, sizeof(o.kernel) - 1);
        o.period = r.period;
        if (hipEventElapsedTime(&t0, b->tl.anchor.get(), r.b) != hipSuccess || hipEventElapsedTime(&t1, b->tl.anchor.get(), r.e) != hipSuccess ||
            hipEventElapsedTime(&d, r.b, r.e) != hipSuccess) {
            (void)hipGetLastError();      // events of a launch that failed or never ran: flag the record, keep the others
            o.flags = 1;
            continue;
        }
        o.start_ms = b->tl.anchor_ms + (double)t0;
        o.end_ms = b->tl.anchor_ms + (double)t1;
        o.duration_ms = (double)d;
    }
    return HF_OK;
}

uint64_t hf_batch_timeline_dropped(const hf_batch* b) { return b ? b->tl.dropped : 0; }

int hf_batch_sync(hf_batch* b) {
    if (!b) return batch_fail(nullptr, HF_ERR_INVALID_ARGUMENT, "null batch");
    for (hf_ctx* m : b->members)
        if (int rc = hf_sync(m)) return batch_fail(b, rc, m->err);
    return HF_OK;
}

// ---- whole clips through a batch: warp or copy per member and period, decided on the device (hf_scene.hip) ----
int hf_batch_scene_set(hf_batch* b, int member, int64_t source_frame_time, int32_t threshold) {
    if (!b) return batch_fail(nullptr, HF_ERR_INVALID_ARGUMENT, "null batch");
    const int n = (int)b->members.size();
    if (member < 0 || member >= n) return batch_fail(b, HF_ERR_INVALID_ARGUMENT, "hf_batch_scene_set: member outside [0, batch size)");
    hf_ctx* l = b->members[0];
    if (hipSetDevice(l->device) != hipSuccess) return batch_fail(b, HF_ERR_HIP, "hipSetDevice failed");
    if (!b->scene_records) {   // first use: the members' histories and kinds on the device, their record rings in mapped host memory
        const size_t nrec = (size_t)hf::kMaxFlowBatch * hf_batch::kSceneRing;
        DevBuf<hf::SceneState> st;   // all or nothing: into the batch only when every step has succeeded
        DevBuf<int32_t> kinds;
        HostBuf<hf::SceneRecord> recs;
        hf::SceneRecord* recs_dev = nullptr;
        const bool ok = alloc_device(st, hf::kMaxFlowBatch * sizeof(hf::SceneState)) == hipSuccess &&
                        alloc_device(kinds, hf::kMaxFlowBatch * sizeof(int32_t)) == hipSuccess &&
                        alloc_host(recs, nrec * sizeof(hf::SceneRecord), hipHostMallocMapped) == hipSuccess &&
                        hipHostGetDevicePointer((void**)&recs_dev, recs.get(), 0) == hipSuccess &&
                        hipMemsetAsync(st.get(), 0, hf::kMaxFlowBatch * sizeof(hf::SceneState), b->stream.get()) == hipSuccess &&
                        hipMemsetAsync(kinds.get(), 0, hf::kMaxFlowBatch * sizeof(int32_t), b->stream.get()) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            return batch_fail(b, HF_ERR_OUT_OF_MEMORY, "hf_batch_scene_set: cannot allocate the scene-change state");
        }
        std::memset(recs.get(), 0, nrec * sizeof(hf::SceneRecord));
        b->scene_states = std::move(st); b->scene_kinds = std::move(kinds); b->scene_records = std::move(recs); b->scene_records_dev = recs_dev;
        b->scene.assign((size_t)n, hf_batch::SceneMember{});
    }
    hf_batch::SceneMember& sm = b->scene[(size_t)member];
    sm.armed = true;
    sm.clear = true;   // NewSegment: the next scene_decide launch starts the member's history over (stream order, nothing to wait for)
    sm.cap = hf::scene_history_cap(source_frame_time > 0 ? source_frame_time : 417083);   // hf_filter_create's default
    sm.threshold = (uint32_t)(threshold < 0 ? DEFAULT_SCENE_CHANGE_THRESHOLD : threshold);
    return HF_OK;
}

}  // extern "C"

namespace hfi {

// hf_batch_run_period_auto / hf_batch_run_period_auto_wide: t and device_out are [batch size][row] arrays
int batch_run_period_auto(hf_batch* b, const void* const* device_frames, int row, const int* n_out, const float* t, void* const* device_out,
                          int mode, const int32_t* force_kind) {
    if (!b) return batch_fail(nullptr, HF_ERR_INVALID_ARGUMENT, "null batch");
    hf_ctx* l = b->members[0];
    const int n = (int)b->members.size();
    // everything that can be refused is refused before anything is enqueued
    if (!device_frames || !n_out || !t || !device_out) return batch_fail(b, HF_ERR_INVALID_ARGUMENT, "hf_batch_run_period_auto: null argument");
    if (int rc = check_period_args(l, "hf_batch_run_period_auto", 0, -1, nullptr, mode)) return batch_fail(b, rc, l->err);
    if (row < 1 || row > HF_MAX_PERIOD_OUTPUTS_WIDE)
        return batch_fail(b, HF_ERR_INVALID_ARGUMENT, "hf_batch_run_period_auto: row outside [1, " + std::to_string(HF_MAX_PERIOD_OUTPUTS_WIDE) + "]");
    if (b->defer_planes && !b->auto_deferred)
        return batch_fail(b, HF_ERR_STATE, "hf_batch_run_period_auto: this batch defers its phase planes, so a period's warps are issued ahead of its chain and the "
                                           "decision does not exist yet; create the leader with HF_FLAG_BATCH_EAGER_PLANES");
    if (l->dual())
        return batch_fail(b, HF_ERR_STATE, "hf_batch_run_period_auto: HF_FLAG_DUAL_STREAM members warp on streams of their own, beside the chain that decides; "
                                           "create the members without HF_FLAG_DUAL_STREAM");
    for (int m = 0; m < n; m++) {
        if (!device_frames[m]) return batch_fail(b, HF_ERR_INVALID_ARGUMENT, "hf_batch_run_period_auto: null frame");
        if (b->members[m]->io_in) return batch_fail(b, HF_ERR_STATE, "hf_batch_run_period_auto: a member uses asynchronous host I/O");
        if (int rc = check_period_args(b->members[m], "hf_batch_run_period_auto", n_out[m], row, t + (size_t)m * row, mode))
            return batch_fail(b, rc, b->members[m]->err);
        if (force_kind && (force_kind[m] < -1 || force_kind[m] > 1))
            return batch_fail(b, HF_ERR_INVALID_ARGUMENT, "hf_batch_run_period_auto: force_kind outside {-1, 0, 1}");
        if (b->scene.empty() || !b->scene[(size_t)m].armed)
            return batch_fail(b, HF_ERR_STATE, "hf_batch_run_period_auto: member " + std::to_string(m) + " was never armed; call hf_batch_scene_set for every member first");
        if (b->scene[(size_t)m].written - b->scene[(size_t)m].read >= hf_batch::kSceneRing)
            return batch_fail(b, HF_ERR_STATE, "hf_batch_run_period_auto: the record ring of member " + std::to_string(m) + " is full (" +
                                               std::to_string(hf_batch::kSceneRing) + " periods); call hf_batch_sync and hf_batch_scene_read more often");
    }
    if (int rc = batch_check_flow_params(b)) return rc;
    // HF_FLAG_BATCH_PLANAR_OUT: warps and the predicated copy write the stages; one conversion launch behind both, per chunk
    if (int rc = batch_ensure_out_stages(b, row, n_out)) return rc;
    const int chunks = hf::plan_period_chunks(n, n_out).n_chunks;
    ObserverGuard observer_guard(b, chunks);
    // a batch that defers its planes (and whose leader carries HF_FLAG_BATCH_AUTO_DEFERRED: the others were refused above) samples only the
    // grid of the new frames, as hf_batch_run_period does
    if (int rc = batch_update(b, device_frames, b->auto_deferred)) return rc;
    bool pending = false, all_have = true;
    for (int m = 0; m < n; m++) {
        pending = pending || b->members[m]->plane_pending[1];
        all_have = all_have && n_out[m] >= 1;
    }
    // the copy's arguments that do not depend on the chunk (outputs and their number: per chunk, interpolate_period); the ring is the update's
    hf::SceneCopyArgs ca{};
    ca.n = n;
    for (int m = 0; m < n; m++) {
        hf_ctx* c = b->members[m];
        const OutputLevels lv = output_levels(c);
        ca.m[m].src = copy_source(c);
        ca.m[m].black = lv.black; ca.m[m].white = lv.white;
    }
    // The period's order is hf_launch_plan.h's.  The steps behind the decision are chunk 0's -- all three launches, or only its copy and
    // conversion where its warps went ahead -- and then the later chunks whole: one interpolate_period call, first_parts says which of chunk 0.
    hf::AutoPeriodPlan plan = hf::plan_auto_period(b->defer_planes, b->auto_deferred, pending, mode, all_have, chunks);
    for (int k = 0; k < plan.n_steps; k++) {
        const hf::PeriodStep step = plan.step[k];
        if (step.kind == hf::kStepEarlyWarps) {
            // The warps of chunk 0 and nothing else of it: they read frames N-2 / N-1 and the flow buffer that is blurred[0] once the chain has
            // swapped (a warm-up member: the buffer its chain does not write; its outputs are overwritten by the copy), and build the pending
            // planes.  Nothing enqueued (the one-launch plan does not qualify): the period takes the usual order and the chain's stand-alone
            // plane launch fills in; a launch that was enqueued and failed is final.
            bool warped = false;
            const int rc = batch_interpolate(b, row, n_out, t, device_out, mode, true, &warped, nullptr, 0, hf::kPartWarps);
            if (warped) { if (rc) return rc; continue; }
            plan = hf::plan_auto_period(b->defer_planes, false, pending, mode, all_have, chunks);
            k = -1;
        } else if (step.kind == hf::kStepChain) {
            if (int rc = batch_calculate(b, true)) return rc;
        } else if (step.kind == hf::kStepDecide) {   // behind the chain's last launch
            hf::SceneDecideArgs da{};
            da.n = n;
            for (int m = 0; m < n; m++) {
                hf_ctx* c = b->members[m];
                hf_batch::SceneMember& sm = b->scene[(size_t)m];
                const uint32_t fc = c->p.frame_count;   // m_frameCount of this period (the update has counted the new frame)
                da.total_delta[m] = c->d_total_delta;
                da.frame_count[m] = fc;
                da.threshold[m] = sm.threshold;
                da.slot[m] = (uint32_t)(sm.written % hf_batch::kSceneRing);
                da.cap[m] = (int8_t)sm.cap;
                da.push[m] = fc >= 3 ? 1 : 0;           // HopperRender.cpp:955-972
                da.clear[m] = sm.clear ? 1 : 0;
                da.force[m] = (int8_t)(force_kind ? force_kind[m] : -1);
            }
            hf::launch_scene_decide(da, b->scene_states.get(), b->scene_kinds.get(), b->scene_records_dev, hf_batch::kSceneRing, b->stream.get());
            if (hipGetLastError() != hipSuccess) return batch_fail(b, HF_ERR_HIP, "scene_decide launch failed");
            for (hf_batch::SceneMember& sm : b->scene) { sm.written++; sm.clear = false; }
        } else {
            // the unchanged warps of the period (diagnostic modes: member by member on the same stream) and the repair of the cut periods, chunk by chunk
            int first_parts = 0;
            for (int j = k; j < plan.n_steps; j++)
                if (plan.step[j].chunk == 0) first_parts |= plan.step[j].kind == hf::kStepWarps ? hf::kPartWarps : plan.step[j].kind == hf::kStepCopy ? hf::kPartCopy : hf::kPartConvert;
            return batch_interpolate(b, row, n_out, t, device_out, mode, false, nullptr, &ca, 0, first_parts);
        }
    }
    return HF_OK;
}

}  // namespace hfi

extern "C" {

int hf_batch_run_period_auto(hf_batch* b, const void* const* device_frames, const int* n_out, const float* t, void* const* device_out,
                             int mode, const int32_t* force_kind) {
    return batch_run_period_auto(b, device_frames, HF_MAX_PERIOD_OUTPUTS, n_out, t, device_out, mode, force_kind);
}

int hf_batch_run_period_auto_wide(hf_batch* b, const void* const* device_frames, int row, const int* n_out, const float* t,
                                  void* const* device_out, int mode, const int32_t* force_kind) {
    return batch_run_period_auto(b, device_frames, row, n_out, t, device_out, mode, force_kind);
}

int hf_batch_scene_read(hf_batch* b, int member, hf_scene_record* out, int capacity, int* n_records) {
    if (!b) return batch_fail(nullptr, HF_ERR_INVALID_ARGUMENT, "null batch");
    if (!n_records || capacity < 0 || (capacity > 0 && !out)) return batch_fail(b, HF_ERR_INVALID_ARGUMENT, "hf_batch_scene_read: bad argument");
    if (member < 0 || member >= (int)b->members.size()) return batch_fail(b, HF_ERR_INVALID_ARGUMENT, "hf_batch_scene_read: member outside [0, batch size)");
    *n_records = 0;
    if (b->scene.empty()) return HF_OK;
    if (hipSetDevice(b->members[0]->device) != hipSuccess) return batch_fail(b, HF_ERR_HIP, "hipSetDevice failed");
    if (hipStreamSynchronize(b->stream.get()) != hipSuccess) return batch_fail(b, HF_ERR_HIP, "hipStreamSynchronize failed");   // (a no-op after hf_batch_sync)
    hf_batch::SceneMember& sm = b->scene[(size_t)member];
    const uint64_t have = sm.written - sm.read;
    *n_records = (int)have;   // how many there were; min(capacity, that) are handed out and leave the ring
    static_assert(sizeof(hf_scene_record) == sizeof(hf::SceneRecord), "hf_scene_record is hf::SceneRecord");
    const uint64_t k = have < (uint64_t)capacity ? have : (uint64_t)capacity;
    for (uint64_t i = 0; i < k; i++)
        std::memcpy(&out[i], &b->scene_records.get()[(size_t)member * hf_batch::kSceneRing + (size_t)((sm.read + i) % hf_batch::kSceneRing)], sizeof(hf_scene_record));
    sm.read += k;
    return HF_OK;
}

}  // extern "C"
