// hopperrender_amd/csrc/hf_calc.hip -- the five virtuals of ONE context on the gfx950 kernels (include/hopperflow.h): updateFrame
// (opticalFlowCalcSDR.cpp:19-29), calculateOpticalFlow (:44-139; the 16-step refinement chain + blur as a cached hipGraph), warpFrames
// (:141-168), copyFrame (:170-183), downloadFrame (:31-42), and the fused period calls built from them.  The three legs of a period each have
// ONE host path here, for n >= 1 contexts: update_frames, calculate_flow, interpolate_period; a batch (hf_batch.hip) and the asynchronous
// update (hf_async_io.hip) call the same functions.  Layout of the ABI: hf_ctx.h.

#include "hf_ctx.h"

using namespace hfi;

namespace hfi {

// Enqueue the refinement chains + blur (opticalFlowCalcSDR.cpp:44-116) of n contexts with identical geometry and
// parameters as ONE set of launches on stream s (hf_kernels.h FlowBatch; n == 1: the plain call).  Capturable: it only enqueues.
int enqueue_flow_chain(const hf_ctx* const* cs, int n, hipStream_t s) {
    const hf_ctx* c = cs[0];
    const hf::Geom& g = c->g;
    const int iters = effective_iterations(c);
    bool any_big = false;
    for (int k = 0; k < iters; k++) any_big |= c->levels[k].window > 32;
    // the window sums are zero on entry: zeroed at creation and re-zeroed by the blur kernel of every chain

    hf::FlowBatch a{};
    a.n = n;
    for (int i = 0; i < n; i++) {
        const hf_ctx* m = cs[i];
        hf::FlowStep& f = a.s[i];
        f.pp1 = m->pp[1].get();                                       // :79 frame N-1
        f.pp2 = m->pp[2].get();                                       // :80 frame N
        f.pl = m->pl;
        f.total_delta = m->d_total_delta;
        f.R = c->p.search_radius;
        f.delta_scalar = c->p.delta_scalar;
        f.neighbor_scalar = c->p.neighbor_scalar;
        f.delta_divisor = (uint32_t)(g.lh * g.lw * (g.hdr ? 6 : 10));  // :93 / HDR :93
        f.sadtab = m->sadtab.get(); f.sad_nbx = m->sad_nbx; f.sad_nby = m->sad_nby;
        f.tables_base = m->tables.get(); f.sums_base = m->sums.get();
        f.counters = c->counters.get();                               // (a batch counts in its leader's)
        f.still_count = m->still_count.get();
    }
    hf::FlowLevel none{};
    hf::PendingArgmin pending[hf::kMaxFlowBatch] = {};   // large-window step whose argmin the next launch takes (hf_kernels.h)
    int step_index = 0;
    auto flush_pending = [&]() {   // explicit argmin launch for a pending step nobody can resolve lazily
        if (!pending[0].active) return;
        hf::FlowBatch b = a;
        for (int i = 0; i < n; i++) {
            hf::FlowStep& f = b.s[i];
            const hf::PendingArgmin& p = pending[i];
            f.cur = p.lvl; f.prev = p.lvl_prev; f.axis = p.axis; f.capture_delta = p.capture_delta;
            f.sums = const_cast<uint32_t*>(p.sums); f.use_neighbors = p.use_neighbors; f.pend = hf::PendingArgmin{};
            pending[i] = hf::PendingArgmin{};
        }
        hf::launch_flow_big_argmin(g, b, s);
    };
    const bool lazy = !(c->cfg.flags & HF_FLAG_NO_LAZY_ARGMIN);
    bool tables_fresh = false;                                    // the previous level of THIS chain refreshed the SAD tables
    for (int k = 0; k < iters; k++) {                             // window halves every level (:110)
        const bool use_neighbors = k >= 4;                        // calcDeltaSumsKernelSDR.h:3,112
        if (use_neighbors) flush_pending();                       // a launch with a neighbour term reads other windows' entries
        const bool small = c->levels[k].window <= 32;
        for (int axis = 0; axis < (small ? 1 : 2); axis++) {
            for (int i = 0; i < n; i++) {
                const hf_ctx* m = cs[i];
                hf::FlowStep& f = a.s[i];
                f.cur = m->levels[k];
                f.prev = k ? m->levels[k - 1] : none;             // :68-69: the chain starts from zero offsets
                f.prev2 = k > 1 ? m->levels[k - 2] : none;
                f.level_index = k;
                // SAD tables: which levels write and read them is hf_launch_plan.h's
                const hf::SadUse sad = hf::plan_sad_tables(m->levels.data(), k, c->tab_mode && m->sadtab);
                f.sad_write = sad.write; f.sad_read = sad.read;
                f.use_neighbors = use_neighbors;
                f.axis = axis;
                f.capture_delta = (k == 0 && axis == 0);          // :91
                f.pend = pending[i];
                if (!small) f.sums = m->sums.get() + (size_t)step_index * m->sums_stride;
                pending[i] = hf::PendingArgmin{};
            }
            // sad_read follows from the previous level's window size; what makes it right is that that level wrote the tables (windows 32 .. 4
            // do, 2 does not: true while the window halves at every level and the chain ends at 2)
            if (a.s[0].sad_read && !tables_fresh)
                return fail(const_cast<hf_ctx*>(c), HF_ERR_STATE, "flow chain: level %d (window %d) would read SAD tables that level %d did not write", k, c->levels[k].window, k - 1);
            tables_fresh = a.s[0].sad_write != 0;
            if (small) {
                hf::launch_flow_level_small(g, a, s);
            } else {
                hf::launch_flow_big_partial(g, a, s);
                for (int i = 0; i < n; i++) {
                    const hf::FlowStep& f = a.s[i];
                    pending[i].active = 1; pending[i].axis = axis; pending[i].capture_delta = f.capture_delta;
                    pending[i].use_neighbors = f.use_neighbors;
                    pending[i].lvl = f.cur; pending[i].lvl_prev = f.prev; pending[i].sums = f.sums;
                }
                step_index++;
                if (!lazy || use_neighbors) flush_pending();
            }
        }
    }
    flush_pending();
    hf::BlurBatch bb{};
    bb.n = n;
    for (int i = 0; i < n; i++) {
        const hf_ctx* m = cs[i];
        bb.s[i].last = iters ? m->levels[iters - 1] : none;
        bb.s[i].blurred = m->blurred[0].get();
        bb.s[i].packed = m->blurred_xy[0].get();
        bb.s[i].zero = any_big ? m->sums.get() : nullptr;
        bb.s[i].still_count = m->still_count.get();
        bb.s[i].still_out = m->still_count ? m->d_total_delta + 1 : nullptr;
    }
    hf::launch_blur_flow(g, bb, c->cfg.blur_radius, (int)(c->sums_bytes / sizeof(uint32_t)), s);  // :115-116
    HF_HIP(const_cast<hf_ctx*>(c), hipGetLastError());
    return HF_OK;
}

// SAD tables or not for the NEXT chain of these contexts (one decision for a batch: its launches are shared).  The tables pay when most
// windows keep their offsets from level to level (tests/flow_reuse_model.py: 74-96 % on the bench scene) and cost 10-15 % of the pipeline
// when hardly any does (every 16 x 16 block its own motion, a hard cut).  Content is coherent in time, so the chain's last kernel reports how
// many windows of the 32-level chose d = 0 on both axes -- what the next level's reuse depends on -- and the host reads whatever report has
// arrived (mapped memory, no synchronisation: one or two periods old) when it issues the next chain.  Smoothed over chains (a cut every few
// periods does not flip it), with hysteresis.  Results are identical either way; only the kernels differ.  HF_FLAG_SAD_REUSE_ALWAYS pins it on.
bool choose_tab_mode(hf_ctx* const* cs, int n) {
    hf_ctx* l = cs[0];
    if (!l->sadtab) return false;
    if (l->cfg.flags & HF_FLAG_SAD_REUSE_ALWAYS) return true;
    // A lone stream (or two, three) leaves most of the device idle: a launch is as long as its slowest wave whatever the others skip, and the
    // table kernels' computing waves take two rounds of 8 candidates per axis.  Chain alone, tables on / off: 73.0 / 70.1 us (1 pair),
    // 84.6 / 82.0 (2), 107.7 / 112.4 (4), 215.8 / 238.1 (16).
    if (n < 4) return false;
    float sum = 0.f;
    int have = 0;
    for (int i = 0; i < n; i++) {
        hf_ctx* m = cs[i];
        const uint32_t raw = m->h_total_delta ? ((volatile uint32_t*)m->h_total_delta.get())[1] : 0xFFFFFFFFu;
        int n32 = 0;
        for (const hf::FlowLevel& L : m->levels) if (L.window == 32) n32 = L.nwx * L.nwy;
        if (raw != 0xFFFFFFFFu && n32 > 0) {
            const float share = (float)raw / (float)n32;
            m->still_share = m->still_share < 0.f ? share : 0.5f * m->still_share + 0.5f * share;
        }
        if (m->still_share >= 0.f) { sum += m->still_share; have++; }
    }
    if (!have) return l->tab_mode;
    const float share = sum / (float)have;
    return l->tab_mode ? share >= 0.30f : share >= 0.45f;
}

// Deferred phase planes (hf_batch_run_period): the chain reads the FULL plane of frame N-1.  Members whose pp[1] still holds only
// the grid samples -- no warp launch took the build up -- get it from the stand-alone plane kernel now, in one launch.
int ensure_older_planes(hf_ctx* const* cs, int n, hipStream_t s) {
    hf::PrepBatch pb{};
    for (int i = 0; i < n; i++) {
        hf_ctx* m = cs[i];
        if (!m->plane_pending[1]) continue;
        pb.frame[pb.n] = m->ring[1]; pb.pp[pb.n] = m->pp[1].get(); pb.n++;
    }
    if (pb.n) {
        hf::launch_prep_frames(cs[0]->g, cs[0]->pl, pb, s);
        if (hipGetLastError() != hipSuccess) return HF_ERR_HIP;
        for (int i = 0; i < n; i++) cs[i]->plane_pending[1] = false;
    }
    return HF_OK;
}

void finish_flow_timing(hf_ctx* c) {
    // opticalFlowCalcSDR.cpp:125-138
    if (!c->flow_timing_pending) return;
    c->flow_timing_pending = false;
    float ms = 0.f;
    if (c->upload_recorded && hipEventElapsedTime(&ms, c->ev_upload.get(), c->ev_flow_end.get()) == hipSuccess)
        c->ofc_calc_time = (double)ms / 1e3;
    if (c->ofc_count >= kCalcTimeInterval) {
        c->ofc_avg = c->ofc_sum / c->ofc_count;
        c->ofc_count = 0;
        c->ofc_sum = 0.0;
        c->ofc_peak = c->ofc_calc_time;
    }
    c->ofc_count++;
    c->ofc_sum += c->ofc_calc_time;
    if (c->ofc_calc_time > c->ofc_peak) c->ofc_peak = c->ofc_calc_time;
}

// Warp launches go to c->warp_stream (HF_FLAG_DUAL_STREAM: a second stream).  The two streams are tied together by
// events: the warp stream waits for what the warps read, and leave_warp_stream() makes c->stream wait for the warps
// again, so every other call keeps its plain in-order semantics.
int enter_warp_stream(hf_ctx* c) {
    if (c->warp_stream == c->stream || c->on_warp_stream) return HF_OK;
    if (c->dual() && c->ev_flow_valid[0]) {
        // warpFrames reads frames N-2/N-1 and the PREVIOUS flow (blurred[0]); the chain that may have just been
        // enqueued on c->stream writes the OTHER flow buffer, so the warps only wait for the chain that produced
        // blurred[0] (recorded behind the uploads of both frames) and run side by side with the current one
        HF_HIP(c, hipStreamWaitEvent(c->warp_stream, c->ev_flow[0].get(), 0));
    } else {
        // no tagged flow yet (the filter warps as soon as m_frameCount >= 3, before a second flow calculation):
        // order the warps behind everything enqueued so far, uploads included
        HF_HIP(c, hipEventRecord(c->ev_chain_done.get(), c->stream));
        HF_HIP(c, hipStreamWaitEvent(c->warp_stream, c->ev_chain_done.get(), 0));
    }
    c->on_warp_stream = true;
    return HF_OK;
}

int leave_warp_stream(hf_ctx* c) {
    if (!c->on_warp_stream) return HF_OK;
    // ev_warps_done was recorded right behind this context's last warp launch
    HF_HIP(c, hipStreamWaitEvent(c->stream, c->ev_warps_done.get(), 0));
    c->on_warp_stream = false;
    return HF_OK;
}

static void rotate_after_upload(hf_ctx* c) {
    // opticalFlowCalcSDR.cpp:22-28 : [0] <- [1] <- [2] <- new (the old [0]) ; frame_count++.  The owners move with their slots.
    auto rotate = [](auto& a) { std::rotate(std::begin(a), std::begin(a) + 1, std::end(a)); };
    rotate(c->ring); rotate(c->ring_store); rotate(c->pp); rotate(c->plane_pending);
    rotate(c->ev_slot_prep);
    rotate(c->in_stage);   // (HF_FLAG_PLANAR_IN) the stage a slot was converted from travels with it: ev_slot_prep guards both
    c->ring_phase = (c->ring_phase + 1) % 3;
    c->p.frame_count++;
}

// The frame update of n >= 1 contexts of one geometry, THE host path of an update: a lone context (b == nullptr, n == 1) or the members of
// batch b, each on its own c->stream (a batch's members share the batch's).  src[i] is context i's new frame, `how` the way all of them
// arrive (FrameSource, hf_ctx.h), planar whether they are planar 4:2:0 (a context's HF_FLAG_PLANAR_IN, a batch's planar_in).  defer
// (hf_batch_run_period): only the grid samples of the new frames now -- what the chain of this period reads of them; their full planes are
// built by the next period's warp launch or, failing that, by ensure_older_planes.  In this order, each step for all n contexts:
//   1. everything that can fail without enqueueing -- a null source (reported as `who`'s), leave_warp_stream, the stage of a planar host
//      frame -- before any context's ring or flags are touched: a failure leaves every context as it was;
//   2. ev_upload (m_ofcStartedEvent, opticalFlowCalcSDR.cpp:20) in front of everything the update enqueues;
//   3. the frame: copied into the context's own slot (a planar host frame: into the slot's stage), waited for (Staged), or referenced.
//      A planar frame always ends up in the own slot -- no reference is kept;
//   4. ONE re-layout launch for all planar sources;  5. ONE phase-plane (or grid-sample) launch over all n;
//   6. ev_slot_prep[0] for the side stream whose next H2D overwrites the slot or its stage;  7. the ring rotates;
//   8. a lone blocking context waits for it all -- but not behind a Staged frame: nothing of asynchronous host I/O blocks (hopperflow.h).
// An error is the failing context's (its err) and, of a batch, the batch's.
int update_frames(hf_batch* b, hf_ctx* const* cs, int n, const void* const* src, FrameSource how, bool planar, bool defer, const char* who) {
    hf_ctx* l = cs[0];
    auto of_member = [b](hf_ctx* m, int rc) { return b ? batch_fail(b, rc, m->err) : rc; };
    auto hip = [&](hf_ctx* m, hipError_t e, const char* what) -> int {
        if (e == hipSuccess) return HF_OK;
        return of_member(m, fail(m, e == hipErrorOutOfMemory ? HF_ERR_OUT_OF_MEMORY : HF_ERR_HIP, "HIP error %d (%s) in %s", (int)e, hipGetErrorString(e), what));
    };
    for (int i = 0; i < n; i++)
        if (!src[i]) return b ? batch_fail(b, HF_ERR_INVALID_ARGUMENT, std::string(who) + ": null frame") : fail(cs[i], HF_ERR_INVALID_ARGUMENT, "%s: null frame", who);
    for (int i = 0; i < n; i++) {
        if (int rc = leave_warp_stream(cs[i])) return of_member(cs[i], rc);
        if (planar && how == FrameSource::Host) if (int rc = ensure_in_stage(cs[i])) return of_member(cs[i], rc);
    }
    for (int i = 0; i < n; i++) {
        hf_ctx* c = cs[i];
        if (!c->timing()) continue;
        if (int rc = hip(c, hipEventRecord(c->ev_upload.get(), c->stream), "hipEventRecord")) return rc;
        c->upload_recorded = true;
    }
    hf::PrepBatch pb{};
    hf::PlanarPair pin[hf::kMaxFlowBatch];
    pb.n = n;
    for (int i = 0; i < n; i++) {
        hf_ctx* c = cs[i];
        const bool by_reference = how == FrameSource::DeviceRef && !planar;
        c->ring[0] = by_reference ? const_cast<void*>(src[i]) : c->ring_store[0].get();
        const void* from = src[i];   // where the re-layout reads a planar frame
        if (how == FrameSource::Staged) {   // the caller's H2D on io_in put it into the slot (planar: into the slot's stage, which is src[i])
            if (int rc = hip(c, hipStreamWaitEvent(c->stream, c->ev_h2d.get(), 0), "hipStreamWaitEvent")) return rc;
        } else if (how == FrameSource::Host && planar) {   // one H2D of the whole frame into the stage
            if (int rc = hip(c, hipMemcpyAsync(c->in_stage[0].get(), src[i], c->in_bytes, hipMemcpyHostToDevice, c->stream), "hipMemcpyAsync")) return rc;
            from = c->in_stage[0].get();
        } else if (!planar && !by_reference) {
            const hipMemcpyKind kind = how == FrameSource::Host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
            if (int rc = hip(c, hipMemcpyAsync(c->ring[0], src[i], c->in_bytes, kind, c->stream), "hipMemcpyAsync")) return rc;
        }
        pin[i] = hf::PlanarPair{from, c->ring[0]};
        pb.frame[i] = c->ring[0];
        pb.pp[i] = c->pp[0].get();
        c->plane_pending[0] = defer;
    }
    // (a lone context keeps the single-frame kernel: its argument block is a tenth of the pair table's, 0.3 us per launch at 2160p)
    if (planar && b) hf::launch_planar_in_batch(l->g.hdr, l->g.H, l->g.in_stride, n, pin, l->stream);
    else if (planar) hf::launch_planar_in(l->g.hdr, l->g.H, l->g.in_stride, pin[0].src, pin[0].dst, l->stream);
    if (defer) hf::launch_prep_grid(l->g, l->pl, pb, l->stream);
    else hf::launch_prep_frames(l->g, l->pl, pb, l->stream);   // (non-temporal plane stores for n > 1 only: a lone context and a batch of one keep the cached variant)
    if (int rc = hip(l, hipGetLastError(), "the phase-plane launch")) return rc;
    for (int i = 0; i < n; i++) {
        hf_ctx* c = cs[i];
        if (c->io_in) if (int rc = hip(c, hipEventRecord(c->ev_slot_prep[0].get(), c->stream), "hipEventRecord")) return rc;
        rotate_after_upload(c);
    }
    if (!b && !l->async() && how != FrameSource::Staged) return sync_ctx(l);
    return HF_OK;
}

int check_flow_params(hf_ctx* c) {
    const int R = c->p.search_radius;
    if (R < 2 || R > kMaxSearchRadius) return fail(c, HF_ERR_INVALID_ARGUMENT, "calculateOpticalFlow: search radius %d outside [2, 16]", R);
    if (c->p.delta_scalar < 0 || c->p.delta_scalar > 24 || c->p.neighbor_scalar < 0 || c->p.neighbor_scalar > 24)
        return fail(c, HF_ERR_INVALID_ARGUMENT, "calculateOpticalFlow: delta/neighbor scalar outside [0, 24]");
    return HF_OK;
}

// Bookkeeping behind an enqueued chain (eager, graph replay or batch), the one place a chain changes its context's host state: what the
// chain ran (hf_get_stats, hf_read_offsets), timing event, flow buffer swap.
int after_flow_enqueued(hf_ctx* c, hipStream_t s) {
    const int iters = effective_iterations(c);
    c->initial_window = initial_window(c->g.lw, c->g.lh);
    c->last_iterations = iters;
    c->last_level = iters ? c->levels[iters - 1] : hf::FlowLevel{};
    if (c->timing()) {
        HF_HIP(c, hipEventRecord(c->ev_flow_end.get(), s));
        c->flow_timing_pending = true;
    }
    c->delta_pending = c->last_iterations > 0;
    if (c->async() && !c->batch) {   // hf_wait_flow(): the host needs m_totalFrameDelta of THIS chain before it decides warp vs copy
        if (!c->ev_flow_done) HF_HIP(c, create_event(c->ev_flow_done, hipEventDisableTiming));
        HF_HIP(c, hipEventRecord(c->ev_flow_done.get(), s));
        c->flow_done_recorded = true;
    }
    if (c->dual()) {   // tag the flow buffer just written, the tag travels with the buffer through the swap below
        HF_HIP(c, hipEventRecord(c->ev_flow[0].get(), s));
        c->ev_flow_valid[0] = true;
        std::swap(c->ev_flow[0], c->ev_flow[1]);
        std::swap(c->ev_flow_valid[0], c->ev_flow_valid[1]);
    }
    // opticalFlowCalcSDR.cpp:121-123 : swap so that [1] = newest flow, [0] = previous flow
    std::swap(c->blurred[0], c->blurred[1]);
    std::swap(c->blurred_xy[0], c->blurred_xy[1]);
    c->blur_phase ^= 1;
    c->have_flow = true;
    return HF_OK;
}

// calculateOpticalFlow of n >= 1 contexts of one geometry and one set of flow parameters as ONE chain on stream s: a context (n = 1, its own
// stream) or the members of a batch (the batch's stream).  graphs: the cache the chain replays from, captured on a miss; nullptr: issued
// eagerly, launch by launch.  warmup_keeps_flow (hf_batch_run_period_auto): a context whose m_frameCount is below 3 rides the launches -- its
// ring always holds valid buffers -- but the filter would not have calculated a flow for it (HopperRender.cpp:955), so its chain writes the
// buffer the next real chain overwrites and nothing else of it moves: no flow-buffer swap, no timing, no delta, no statistics.
// An error is reported in cs[0]->err, whichever context it came from.
int calculate_flow(hf_ctx* const* cs, int n, hipStream_t s, ChainGraphs* graphs, bool warmup_keeps_flow) {
    hf_ctx* l = cs[0];
    auto of_member = [l](const hf_ctx* m, int rc) { if (m != l) l->err = m->err; return rc; };
    for (int i = 0; i < n; i++) if (int rc = leave_warp_stream(cs[i])) return of_member(cs[i], rc);
    if (ensure_older_planes(cs, n, s)) return fail(l, HF_ERR_HIP, "phase-plane launch failed");
    l->tab_mode = choose_tab_mode(cs, n);
    hipGraphExec_t exec = nullptr;
    if (graphs) {
        ChainGraphs::Key key;
        key.fill(-1);
        key[0] = l->p.search_radius; key[1] = l->p.delta_scalar; key[2] = l->p.neighbor_scalar; key[3] = (int)l->tab_mode;
        for (int i = 0; i < n; i++) key[4 + i] = cs[i]->ring_phase * 2 + cs[i]->blur_phase;
        exec = graphs->find(key);
        if (!exec) {
            hipGraph_t graph = nullptr;
            std::shared_lock<std::shared_mutex> capture_lock(g_capture_mutex);
            HF_HIP(l, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
            const int rc = enqueue_flow_chain(cs, n, s);
            const hipError_t e = hipStreamEndCapture(s, &graph);
            capture_lock.unlock();
            if (rc) { if (graph) hipGraphDestroy(graph); return rc; }
            HF_HIP(l, e);
            GraphExec fresh;
            const hipError_t ei = instantiate_graph(fresh, graph);
            hipGraphDestroy(graph);
            HF_HIP(l, ei);
            exec = graphs->insert(key, std::move(fresh));
        }
    }
    // the leader's profile carries the chain (one span = n chains); an observed launch carries the timeline's events, not a profile span's
    const int span = hf::t_launch_observer ? -1 : span_begin(l, 2);
    if (exec) HF_HIP(l, hipGraphLaunch(exec, s));
    else if (int rc = enqueue_flow_chain(cs, n, s)) return rc;
    if (span >= 0) { span_end(l, span); l->spans[span].frames = n; }
    for (int i = 0; i < n; i++)
        if (!(warmup_keeps_flow && cs[i]->p.frame_count < 3))
            if (int rc = after_flow_enqueued(cs[i], s)) return of_member(cs[i], rc);
    return HF_OK;
}

// warpFrames' checks of its arguments (opticalFlowCalcSDR.cpp:143-146, and the output mode) for the n_out outputs of one period, for every
// call that warps: the mode, n_out in [0, max_n_out] (max_n_out < 0: no upper bound), every blending scalar.  The error is c's.
int check_period_args(hf_ctx* c, const char* who, int n_out, int max_n_out, const float* t, int mode) {
    if (mode < 0 || mode > 6) return fail(c, HF_ERR_INVALID_ARGUMENT, "warpFrames: frame output mode %d outside [0, 6]", mode);
    if (n_out < 0 || (max_n_out >= 0 && n_out > max_n_out)) return fail(c, HF_ERR_INVALID_ARGUMENT, "%s: n_out outside [0, %d]", who, max_n_out);
    for (int i = 0; i < n_out; i++)
        if (t[i] > 1.0f) return fail(c, HF_ERR_INVALID_ARGUMENT, "Error in function warpFrames: blending scalar is greater than 1.0");
    return HF_OK;
}

// black and white level in the units of the frames' samples (opticalFlowCalcHDR.cpp:151-152,173-174)
OutputLevels output_levels(const hf_ctx* c) { const float k = c->g.hdr ? 256.0f : 1.0f; return {c->p.black_level * k, c->p.white_level * k}; }

// the frame copyFrame shows: N-2 once the ring is full, before that the oldest one there is (opticalFlowCalcSDR.cpp:173)
void* copy_source(const hf_ctx* c) { return c->ring[c->p.frame_count >= 3 ? 0 : c->p.frame_count >= 2 ? 1 : 2]; }

// m_warpCalcTime (opticalFlowCalcSDR.cpp:36-41) runs from the first warp or copy launch after a download, on the stream the caller names
static int mark_warp_start(hf_ctx* c, hipStream_t s) {
    if (!c->warp_started && c->timing()) { HF_HIP(c, hipEventRecord(c->ev_warp_start.get(), s)); c->warp_started = true; }
    return HF_OK;
}

// Fills the period descriptor of one context: frames N-2 / N-1, the PREVIOUS flow (:154-156), levels, outputs.
// flow_index 1: the period is issued BEFORE the chain of its source period -- the previous flow is still the newest one
static void fill_period(hf_ctx* c, int n, const float* t, void* const* outs, hf::WarpPeriod& p, int flow_index = 0) {
    p.frame12 = c->ring[0]; p.frame21 = c->ring[1];
    p.flow = c->blurred[flow_index].get(); p.flow_xy = c->blurred_xy[flow_index].get();
    p.black = output_levels(c).black; p.white = output_levels(c).white;
    p.n_out = n;
    p.counters = c->counters.get();
    for (int i = 0; i < n; i++) { p.ts[i] = t[i]; p.outs[i] = outs[i] ? outs[i] : c->out_frame.get(); }
}

// The semi-planar frames the warps of a period write where its output side is planar (HF_FLAG_PLANAR_OUT; a member of a
// HF_FLAG_BATCH_PLANAR_OUT batch) and the caller named a buffer: grown to the widest period seen, kMaxWarpOutputs at the most -- a wider
// period goes out in chunks, each converted before the next one's warps reuse the stages (stream order).  Allocates, so a call runs it
// before its first enqueue.  Released by hf_batch_destroy for a batch's members, with the context otherwise.
int ensure_period_stages(hf_ctx* c, int n) {
    while ((int)c->period_stage.size() < n && (int)c->period_stage.size() < hf::kMaxWarpOutputs) {
        DevBuf<void> p;
        HF_HIP(c, alloc_device(p, c->out_bytes));
        c->period_stage.push_back(std::move(p));
    }
    return HF_OK;
}

// The outputs of period p of ONE context on its warp stream: all of them in one launch when the fast warp kernel applies -- the flow is
// looked up once and the source rows of the later outputs come from L1/L2 instead of HBM (2F + nF bytes instead of n * 3F) -- else one
// launch per output.  Profiled launches carry start/stop events of the dispatch itself (hipExtLaunchKernel), i.e. the kernel's execution
// time as rocprof reports it, not the time the launch spent queued behind other streams.  The caller records ev_warps_done.
static int warp_member(hf_ctx* c, const hf::WarpPeriod& p, int mode) {
    if (int rc = mark_warp_start(c, c->stream)) return rc;
    if (int rc = enter_warp_stream(c)) return rc;
    const int n_out = p.n_out;
    for (int i = 0; i < n_out; i++) if (int rc = guard_output_slot(c, p.outs[i], c->warp_stream)) return rc;
    const bool fuse = n_out >= 2 && !(c->cfg.flags & HF_FLAG_NO_FUSED_WARP);
    bool fused = false;
    if (fuse) {
        const int span = span_open(c, 0);
        fused = hf::launch_warp_periods(c->g, 1, &p, mode, c->warp_stream, span >= 0 ? c->spans[span].b.get() : nullptr, span >= 0 ? c->spans[span].e.get() : nullptr);
        if (!fused) span_cancel(c, span);   // shape not eligible: drop the unused span
        else if (span >= 0) c->spans[span].frames = n_out;
    }
    for (int i = 0; i < n_out && !fused; i++) {
        const int span = span_open(c, 0);
        hf::launch_warp(c->g, p.frame12, p.frame21, p.flow, p.flow_xy, p.outs[i], p.ts[i], mode, p.black, p.white, c->warp_stream,
                        span >= 0 ? c->spans[span].b.get() : nullptr, span >= 0 ? c->spans[span].e.get() : nullptr);
    }
    HF_HIP(c, hipGetLastError());
    return note_launch(c, c->warp_stream);
}

// The warps of one source period of n >= 1 contexts of one geometry, THE host path of a period's warps: a lone context (b == nullptr,
// n == 1, any n_out) or the members of batch b.  t and device_out are [n][row] arrays.  Chunk by chunk (hf_launch_plan.h
// period_chunk_count; a period of up to kMaxWarpOutputs outputs per member is one chunk), per chunk in stream order:
//   1. targets: output i of a member goes to the caller's buffer, to the member's internal frame for a NULL entry, or -- planar output
//      side and a buffer named -- to the member's stage i (ensure_period_stages: the caller's, with its checks of n_out);
//   2. warps: ONE fused launch on the batch's stream over the members that have outputs in the chunk (single-stream members of a batch,
//      none of them HF_FLAG_NO_FUSED_WARP; they keep their batch index wherever the device looks one up: scene_kinds, SceneCopyArgs) or,
//      where that does not qualify (diagnostic modes, odd shapes, a misaligned output), those members one by one (warp_member);
//   3. the predicated copy of the chunk (copy != nullptr: hf_batch_run_period_auto; src and levels per member are the caller's, outputs
//      and counts are filled in here);
//   4. the conversion of the chunk's staged outputs into the caller's planar buffers, in ONE launch on the stream its warps ran on.
// Stream order lets every chunk reuse the same stages.  Chunks [first_chunk, ...) are issued; of chunk first_chunk only the launches named in
// first_parts (hf_launch_plan.h PeriodParts), of the later chunks all three.
// before_chain (hf_batch_run_period with deferred phase planes): chunk 0 -- every member has outputs in it -- goes out AHEAD of the
// period's chain: it reads frames N-2 / N-1 and the previous flow, which the chain does not touch, and builds the full plane of frame N-1
// that the chain then reads.  Only the one-launch path qualifies; *launched = false means nothing was enqueued and the caller keeps the
// usual order.  The later chunks of the period always follow the chain (first_chunk = 1): the member-by-member path reads flow buffer 0,
// which is the previous flow only once the chain has swapped the buffers.  hf_batch_run_period_auto on a deferring batch (hf_launch_plan.h
// plan_auto_period) sends only the WARPS of chunk 0 ahead (before_chain, first_parts = kPartWarps) and issues that chunk's copy and
// conversion behind the decision (first_chunk = 0, first_parts = kPartCopy | kPartConvert): the targets of a chunk depend on the call's
// arguments alone, so both calls name the same stages, which nothing between them touches.
// An error is the failing context's (its err) and, of a batch, the batch's.
int interpolate_period(hf_batch* b, hf_ctx* const* cs, int n, int row, const int* n_out, const float* t, void* const* device_out, int mode,
                       bool before_chain, bool* launched, hf::SceneCopyArgs* copy, int first_chunk, int first_parts) {
    hf_ctx* l = cs[0];
    const bool planar = b ? b->planar_out : l->planar_out();
    auto of_member = [b](hf_ctx* m, int rc) { return b ? batch_fail(b, rc, m->err) : rc; };
    auto of_launch = [b, l](const char* what) { return b ? batch_fail(b, HF_ERR_HIP, what) : fail(l, HF_ERR_HIP, "%s", what); };
    bool fused = b && !l->dual(), all_have = true;
    int chunks = 0;
    for (int m = 0; m < n; m++) {
        fused = fused && !(cs[m]->cfg.flags & HF_FLAG_NO_FUSED_WARP);
        all_have = all_have && n_out[m] >= 1;
        if (hf::period_chunks(n_out[m]) > chunks) chunks = hf::period_chunks(n_out[m]);
    }
    if (before_chain && !(fused && all_have)) return HF_OK;   // not eligible for one launch: the caller issues the period after the chain, as usual
    // (the auto call issues its predicated copy in a period without any output too: its launches do not depend on the schedule)
    const int end = before_chain ? 1 : chunks ? chunks : copy ? 1 : 0;
    for (int ch = first_chunk; ch < end; ch++) {
        hf::WarpPeriod periods[hf::kMaxFlowBatch];
        hf::PlanarPair pairs[hf::kMaxPlanarOutPairs];
        hf_ctx* who[hf::kMaxFlowBatch];
        const int parts = ch == first_chunk ? first_parts : hf::kPartsAll;
        int np = 0, frames = 0, npairs = 0;
        for (int m = 0; m < n; m++) {
            hf_ctx* c = cs[m];
            const int count = hf::period_chunk_count(n_out[m], ch);
            const size_t at = (size_t)m * row + (size_t)ch * hf::kMaxWarpOutputs;
            void* outs[hf::kMaxWarpOutputs];
            for (int i = 0; i < count; i++) {
                void* o = device_out[at + i];
                outs[i] = o && planar ? c->period_stage[(size_t)i].get() : o;
                if (o && planar) pairs[npairs++] = hf::PlanarPair{outs[i], o};
            }
            if (count) {
                fill_period(c, count, t + at, outs, periods[np], before_chain ? 1 : 0);
                who[np++] = c; frames += count;
            }
            if (copy) {   // the repair of the cut periods: this chunk's outputs of the members whose kind is copy
                copy->m[m].n_out = count;
                for (int i = 0; i < count; i++) copy->m[m].outs[i] = outs[i] ? outs[i] : c->out_frame.get();
            }
        }
        bool done = np == 0 || !(parts & hf::kPartWarps);
        if (fused && !done) {
            // the chunk of every member in ONE launch on the batch stream (single-stream members: program order does the rest).  They have
            // no asynchronous host I/O (hf_batch_create / hf_*_async enforce it): no output-ring slot to guard, no side stream to notify
            for (int k = 0; k < np; k++) {
                hf_ctx* c = who[k];
                if (before_chain && c->plane_pending[1]) periods[k].plane21 = c->pp[1].get();
                if (int rc = mark_warp_start(c, l->stream)) return of_member(c, rc);
            }
            const int span = hf::t_launch_observer == &b->tl ? -1 : span_open(l, 0);   // (an observed launch carries the timeline's events, not a profile span's)
            bool built[hf::kMaxFlowBatch];
            if (hf::launch_warp_periods(l->g, np, periods, mode, l->stream, span >= 0 ? l->spans[span].b.get() : nullptr, span >= 0 ? l->spans[span].e.get() : nullptr,
                                        before_chain ? &l->pl : nullptr, built)) {
                if (span >= 0) l->spans[span].frames = frames;
                if (launched) *launched = true;   // from here on the period's warps are enqueued: an error is final, never a reason to issue them again
                if (hipGetLastError() != hipSuccess) return of_launch("fused warp launch failed");
                for (int k = 0; k < np; k++) if (built[k]) who[k]->plane_pending[1] = false;
                done = true;
            } else {
                span_cancel(l, span);
            }
        }
        if (!done) {
            if (before_chain) return HF_OK;   // not eligible for one launch: the caller issues the period after the chain, as usual
            for (int k = 0; k < np; k++) if (int rc = warp_member(who[k], periods[k], mode)) return of_member(who[k], rc);
        }
        if (copy && (parts & hf::kPartCopy)) {
            hf::launch_scene_copy(l->g, *copy, b->scene_kinds.get(), l->stream);
            if (hipGetLastError() != hipSuccess) return of_launch("scene_copy launch failed");
        }
        if (npairs && (parts & hf::kPartConvert)) {
            hf::launch_planar_out_batch(l->g.hdr, l->g.H, l->g.out_stride, npairs, pairs, l->warp_stream);
            if (hipGetLastError() != hipSuccess) return of_launch("planar output launch failed");
        }
    }
    // one completion event for all the warps (and conversions) the period put on a member's warp stream, behind the last of them
    for (int m = 0; m < n; m++)
        if (n_out[m] > 0 && cs[m]->on_warp_stream)
            if (hipEventRecord(cs[m]->ev_warps_done.get(), cs[m]->warp_stream) != hipSuccess) return of_launch("hipEventRecord failed");
    return HF_OK;
}

int download_common(hf_ctx* c, void* dst, hipMemcpyKind kind) {
    if (int rc = set_device(c)) return rc;
    if (int rc = leave_warp_stream(c)) return rc;
    if (c->planar_out()) {
        if (kind == hipMemcpyDeviceToDevice) {
            hf::launch_planar_out(c->g.hdr, c->g.H, c->g.out_stride, c->out_target, dst, c->stream);
        } else {   // re-layout into the stage paired with the output slot, then one D2H
            if (int rc = ensure_out_stage(c)) return rc;
            void* st = c->out_stage[out_slot(c, c->out_target)].get();
            if (c->dl_issued)   // an asynchronous readback (hf_download_frame_async) may still read that stage
                HF_HIP(c, hipStreamWaitEvent(c->stream, c->ev_dl[(c->dl_issued - 1) % hf_ctx::kDlRing].get(), 0));
            hf::launch_planar_out(c->g.hdr, c->g.H, c->g.out_stride, c->out_target, st, c->stream);
            HF_HIP(c, hipMemcpyAsync(dst, st, c->out_bytes, kind, c->stream));
        }
        HF_HIP(c, hipGetLastError());
    } else if (c->out_target != dst) {
        HF_HIP(c, hipMemcpyAsync(dst, c->out_target, c->out_bytes, kind, c->stream));
    }
    if (c->timing()) HF_HIP(c, hipEventRecord(c->ev_warp_end.get(), c->stream));
    if (kind == hipMemcpyDeviceToHost || !c->async()) {
        if (int rc = sync_ctx(c)) return rc;
        float ms = 0.f;
        if (c->warp_started && hipEventElapsedTime(&ms, c->ev_warp_start.get(), c->ev_warp_end.get()) == hipSuccess)
            c->warp_calc_time = (double)ms / 1e3;  // opticalFlowCalcSDR.cpp:36-41
    }
    c->warp_started = false;
    return HF_OK;
}

}  // namespace hfi

static int update_one(hf_ctx* c, const void* frame, FrameSource how, const char* who) {
    HF_CHECK_CTX(c);
    if (int rc = set_device(c)) return rc;
    return update_frames(nullptr, &c, 1, &frame, how, c->planar_in(), false, who);
}

extern "C" {

int hf_update_frame(hf_ctx* c, const void* host_frame) { return update_one(c, host_frame, FrameSource::Host, "hf_update_frame"); }

int hf_update_frame_device(hf_ctx* c, const void* device_frame) { return update_one(c, device_frame, FrameSource::Device, "hf_update_frame_device"); }

int hf_update_frame_device_ref(hf_ctx* c, const void* device_frame) { return update_one(c, device_frame, FrameSource::DeviceRef, "hf_update_frame_device_ref"); }

int hf_calculate_optical_flow(hf_ctx* c) {
    HF_CHECK_CTX(c);
    if (int rc = set_device(c)) return rc;
    if (int rc = check_flow_params(c)) return rc;
    if (int rc = calculate_flow(&c, 1, c->stream, (c->cfg.flags & HF_FLAG_NO_GRAPH) ? nullptr : &c->graphs, false)) return rc;
    if (!c->async()) return sync_ctx(c);
    return HF_OK;
}

int hf_warp_frames(hf_ctx* c, float t, int mode) {
    HF_CHECK_CTX(c);
    if (int rc = check_period_args(c, "warpFrames", 1, -1, &t, mode)) return rc;
    if (int rc = set_device(c)) return rc;
    hf::WarpPeriod p;   // frames N-2 / N-1 and the PREVIOUS flow (:154-156) into the output target
    fill_period(c, 1, &t, &c->out_target, p);
    if (int rc = warp_member(c, p, mode)) return rc;
    if (c->on_warp_stream) HF_HIP(c, hipEventRecord(c->ev_warps_done.get(), c->warp_stream));
    return HF_OK;
}

// The argument checks of hf_warp_disagreement_map_enqueue, for it and for the call that runs its launch first (`who`).
static int check_disagreement_args(hf_ctx* c, const char* who, int n_t, const float* t, int tile, void* device_maps) {
    if (!t) return fail(c, HF_ERR_INVALID_ARGUMENT, "%s: null blending scalars", who);
    if (n_t < 1 || n_t > HF_MAX_DISAGREEMENT_OUTPUTS) return fail(c, HF_ERR_INVALID_ARGUMENT, "%s: %d outputs, one launch takes 1 .. %d", who, n_t, HF_MAX_DISAGREEMENT_OUTPUTS);
    if (int rc = check_period_args(c, who, n_t, HF_MAX_DISAGREEMENT_OUTPUTS, t, 0)) return rc;
    if (!HF_ERROR_MAP_TILES_OK(tile)) return fail(c, HF_ERR_INVALID_ARGUMENT, "%s: tile %d, not 16, 32 or 64", who, tile);
    if (!device_maps || ((uintptr_t)device_maps & 15u)) return fail(c, HF_ERR_INVALID_ARGUMENT, "%s: the map buffer %p is null or not 16-byte aligned", who, device_maps);
    return HF_OK;
}

// What hf_warp_frames would read at this moment -- frames N-2 / N-1 and the previous flow -- and where its modes 0 and 1 would disagree,
// per tile; ordered like hf_frame_error_enqueue.  Nothing of the context moves: no output, no warp bookkeeping, no span, no counters.
int hf_warp_disagreement_map_enqueue(hf_ctx* c, int n_t, const float* t, int tile, void* device_maps) {
    static_assert(HF_MAX_DISAGREEMENT_OUTPUTS == hf::kMaxDisagreementOutputs, "hopperflow.h");
    const char* who = "hf_warp_disagreement_map_enqueue";
    HF_CHECK_CTX(c);
    if (int rc = check_disagreement_args(c, who, n_t, t, tile, device_maps)) return rc;
    if (int rc = set_device(c)) return rc;
    if (int rc = leave_warp_stream(c)) return rc;
    hf::WarpPeriod p;
    fill_period(c, 0, nullptr, nullptr, p);
    if (!hf::launch_warp_disagreement(c->g, p.frame12, p.frame21, p.flow, p.flow_xy, n_t, t, tile, device_maps, c->stream))
        return fail(c, HF_ERR_INVALID_ARGUMENT, "%s: nothing launched", who);
    HF_HIP(c, hipGetLastError());
    return note_launch(c, c->stream);   // a reader of the ring like the warps: the next asynchronous upload into frame N-2's slot waits for it
}

// The disagreement launch as above, then behind it on the same stream the blend that acts on it: per output the mode-2 frame of
// hf_warp_frames mixed with the cross-fade of the two source frames by the weights of that output's map.  Same sources, order and state.
int hf_guarded_blend_enqueue(hf_ctx* c, int n_t, const float* t, int tile, int lo_q4, int hi_q4, void* device_maps, void* const* device_out) {
    const char* who = "hf_guarded_blend_enqueue";
    HF_CHECK_CTX(c);
    if (int rc = check_disagreement_args(c, who, n_t, t, tile, device_maps)) return rc;
    if (lo_q4 < 0 || lo_q4 >= hi_q4 || hi_q4 > 65535) return fail(c, HF_ERR_INVALID_ARGUMENT, "%s: thresholds %d, %d outside 0 <= lo_q4 < hi_q4 <= 65535", who, lo_q4, hi_q4);
    if (!device_out) return fail(c, HF_ERR_INVALID_ARGUMENT, "%s: null output frames", who);
    for (int k = 0; k < n_t; k++) if (!device_out[k]) return fail(c, HF_ERR_INVALID_ARGUMENT, "%s: output frame %d is null", who, k);
    if (int rc = set_device(c)) return rc;
    if (int rc = leave_warp_stream(c)) return rc;
    hf::WarpPeriod p;
    fill_period(c, 0, nullptr, nullptr, p);
    if (!hf::launch_warp_disagreement(c->g, p.frame12, p.frame21, p.flow, p.flow_xy, n_t, t, tile, device_maps, c->stream))
        return fail(c, HF_ERR_INVALID_ARGUMENT, "%s: nothing launched", who);
    HF_HIP(c, hipGetLastError());
    if (!hf::launch_guarded_blend(c->g, p.frame12, p.frame21, p.flow, p.flow_xy, n_t, t, tile, lo_q4, hi_q4, device_maps, device_out, p.black, p.white, c->stream))
        return fail(c, HF_ERR_INVALID_ARGUMENT, "%s: nothing launched", who);
    HF_HIP(c, hipGetLastError());
    return note_launch(c, c->stream);
}

int hf_copy_frame(hf_ctx* c) {
    HF_CHECK_CTX(c);
    if (int rc = set_device(c)) return rc;
    const OutputLevels lv = output_levels(c);
    if (int rc = leave_warp_stream(c)) return rc;
    if (int rc = mark_warp_start(c, c->stream)) return rc;
    if (int rc = guard_output_slot(c, c->out_target, c->stream)) return rc;
    const int span = span_begin(c, 1);
    hf::launch_copy(c->g, copy_source(c), c->out_target, lv.black, lv.white, c->stream);
    span_end(c, span);
    HF_HIP(c, hipGetLastError());
    return note_launch(c, c->stream);
}

int hf_interpolate_period(hf_ctx* c, const void* device_frame, int n_out, const float* t, void* const* device_out, int mode) {
    return hf_interpolate_period_ex(c, device_frame, n_out, t, device_out, mode, 1);
}

int hf_interpolate_period_ex(hf_ctx* c, const void* device_frame, int n_out, const float* t, void* const* device_out, int mode,
                             int update_and_flow) {
    HF_CHECK_CTX(c);
    if (n_out < 0 || (n_out > 0 && (!t || !device_out))) return fail(c, HF_ERR_INVALID_ARGUMENT, "hf_interpolate_period: bad argument");
    if (c->planar_out() && n_out > 0) {   // (the stages: allocated before anything of this call is enqueued)
        if (int rc = set_device(c)) return rc;
        if (int rc = ensure_period_stages(c, n_out)) return rc;
    }
    if (update_and_flow) {
        if (device_frame) if (int rc = hf_update_frame_device_ref(c, device_frame)) return rc;
        if (int rc = hf_calculate_optical_flow(c)) return rc;
    }
    if (int rc = set_device(c)) return rc;
    // (only now: the three separate calls would have updated and calculated before warpFrames refused its arguments; n_out has no upper bound here)
    if (int rc = check_period_args(c, "hf_interpolate_period", n_out, -1, t, mode)) return rc;
    return interpolate_period(nullptr, &c, 1, n_out, &n_out, t, device_out, mode);
}

int hf_download_frame(hf_ctx* c, void* host_out) {
    HF_CHECK_CTX(c);
    if (!host_out) return fail(c, HF_ERR_INVALID_ARGUMENT, "hf_download_frame: null buffer");
    return download_common(c, host_out, hipMemcpyDeviceToHost);
}

int hf_download_frame_device(hf_ctx* c, void* device_out) {
    HF_CHECK_CTX(c);
    if (!device_out) return fail(c, HF_ERR_INVALID_ARGUMENT, "hf_download_frame_device: null buffer");
    return download_common(c, device_out, hipMemcpyDeviceToDevice);
}

int hf_set_output_buffer(hf_ctx* c, void* device_out) {
    HF_CHECK_CTX(c);
    if (device_out && c->planar_out())
        return fail(c, HF_ERR_STATE, "hf_set_output_buffer: the kernels write NV12 / P010 frames; under HF_FLAG_PLANAR_OUT use hf_download_frame_device");
    c->out_target = device_out ? device_out : c->out_frame.get();
    return HF_OK;
}

}  // extern "C"
