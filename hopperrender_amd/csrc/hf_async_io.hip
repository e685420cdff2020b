// hopperrender_amd/csrc/hf_async_io.hip -- pinned asynchronous host I/O of a context on side streams (include/hopperflow.h
// hf_update_frame_async / hf_download_frame_async, hf_wait_flow / hf_wait_download): the reference's blocking CL_TRUE transfers
// (opticalFlowCalcSDR.cpp:19-42) as H2D / D2H copies that overlap the compute stream.  The upload is the H2D alone: the update behind it
// is update_frames (hf_calc.hip), the host path of every update.  Layout of the ABI: hf_ctx.h.

#include "hf_ctx.h"

using namespace hfi;

namespace hfi {

// All or nothing: the side streams, their events and output-ring slots 1 and 2 are built into locals and move into the context only
// when every step has succeeded; a failure leaves the context as it was (io_in empty: the next call tries again).
int io_init(hf_ctx* c) {
    if (c->io_in) return HF_OK;
    Stream in, out;
    Event h2d, last_launch, out_ready, slot_prep[3], d2h[hf_ctx::kOutRing], dl[hf_ctx::kDlRing];
    DevBuf<void> ring[hf_ctx::kOutRing];
    HF_HIP(c, create_stream(in));
    HF_HIP(c, create_stream(out));
    for (Event* e : {&h2d, &last_launch, &out_ready}) HF_HIP(c, create_event(*e, hipEventDisableTiming));
    for (auto& e : slot_prep) HF_HIP(c, create_event(e, hipEventDisableTiming));
    for (auto& e : d2h) HF_HIP(c, create_event(e, hipEventDisableTiming));
    for (auto& e : dl) HF_HIP(c, create_event(e, hipEventDisableTiming));
    for (int i = 1; i < hf_ctx::kOutRing; i++) HF_HIP(c, alloc_device(ring[i], c->out_bytes));
    c->io_in = std::move(in); c->io_out = std::move(out);
    c->ev_h2d = std::move(h2d); c->ev_last_launch = std::move(last_launch); c->ev_out_ready = std::move(out_ready);
    std::move(std::begin(slot_prep), std::end(slot_prep), c->ev_slot_prep);
    std::move(std::begin(d2h), std::end(d2h), c->ev_d2h);
    std::move(std::begin(dl), std::end(dl), c->ev_dl);
    std::move(std::begin(ring), std::end(ring), c->out_ring);
    return HF_OK;
}

// Before a warp/copy writes into an output-ring slot: wait for the asynchronous readback that still uses it.
// HF_FLAG_PLANAR_IN / _OUT stages (hf_ctx.h), allocated on first use
int ensure_in_stage(hf_ctx* c) {
    for (auto& p : c->in_stage) if (!p) HF_HIP(c, alloc_device(p, c->in_bytes));
    return HF_OK;
}

int ensure_out_stage(hf_ctx* c) {
    for (auto& p : c->out_stage) if (!p) HF_HIP(c, alloc_device(p, c->out_bytes));
    return HF_OK;
}

int out_slot(const hf_ctx* c, const void* target) {   // the output-ring slot `target` is, 0 if none
    for (int i = 0; i < hf_ctx::kOutRing; i++) if (c->out_at(i) && target == c->out_at(i)) return i;
    return 0;
}

int guard_output_slot(hf_ctx* c, const void* target, hipStream_t launch_stream) {
    if (!c->io_out) return HF_OK;
    for (int i = 0; i < hf_ctx::kOutRing; i++)
        if (target == c->out_at(i) && c->d2h_pending[i]) {
            HF_HIP(c, hipStreamWaitEvent(launch_stream, c->ev_d2h[i].get(), 0));
            c->d2h_pending[i] = false;
        }
    return HF_OK;
}

int note_launch(hf_ctx* c, hipStream_t launch_stream) {   // remembers "the frames/flow of the ring are being read up to here"
    if (!c->io_in) return HF_OK;
    HF_HIP(c, hipEventRecord(c->ev_last_launch.get(), launch_stream));
    c->have_last_launch = true;
    return HF_OK;
}

}  // namespace hfi

extern "C" {

int hf_update_frame_async(hf_ctx* c, const void* pinned_host_frame) {
    HF_CHECK_CTX(c);
    if (!pinned_host_frame) return fail(c, HF_ERR_INVALID_ARGUMENT, "hf_update_frame_async: null frame");
    if (c->batch) return fail(c, HF_ERR_STATE, "hf_update_frame_async: the context is a member of a batch (asynchronous host I/O uses side streams of its own)");
    if (int rc = set_device(c)) return rc;
    if (int rc = io_init(c)) return rc;
    // the slot about to be overwritten holds the oldest frame: its last readers are the warp/copy launches
    // issued so far and its own (three updates old) phase-plane build
    // (HF_FLAG_PLANAR_IN: the frame lands in the stage of that slot, whose last reader is the same re-layout launch in front of that build)
    if (c->planar_in()) if (int rc = ensure_in_stage(c)) return rc;
    if (c->have_last_launch) HF_HIP(c, hipStreamWaitEvent(c->io_in.get(), c->ev_last_launch.get(), 0));
    HF_HIP(c, hipStreamWaitEvent(c->io_in.get(), c->ev_slot_prep[0].get(), 0));
    void* const staged = c->planar_in() ? c->in_stage[0].get() : c->ring_store[0].get();
    HF_HIP(c, hipMemcpyAsync(staged, pinned_host_frame, c->in_bytes, hipMemcpyHostToDevice, c->io_in.get()));
    HF_HIP(c, hipEventRecord(c->ev_h2d.get(), c->io_in.get()));
    // the update itself (hf_calc.hip update_frames): c->stream waits for ev_h2d instead of copying
    return update_frames(nullptr, &c, 1, &staged, FrameSource::Staged, c->planar_in(), false, "hf_update_frame_async");
}

int hf_download_frame_async(hf_ctx* c, void* pinned_host_out) {
    HF_CHECK_CTX(c);
    if (!pinned_host_out) return fail(c, HF_ERR_INVALID_ARGUMENT, "hf_download_frame_async: null buffer");
    if (c->batch) return fail(c, HF_ERR_STATE, "hf_download_frame_async: the context is a member of a batch (asynchronous host I/O uses side streams of its own)");
    if (int rc = set_device(c)) return rc;
    if (int rc = io_init(c)) return rc;
    hipStream_t last = c->on_warp_stream ? c->warp_stream : c->stream;   // where the frame was just produced
    HF_HIP(c, hipEventRecord(c->ev_out_ready.get(), last));
    HF_HIP(c, hipStreamWaitEvent(c->io_out.get(), c->ev_out_ready.get(), 0));
    const void* from = c->out_target;
    if (c->planar_out()) {
        // re-layout on the readback stream into the stage paired with the output slot: the next conversion into that stage is issued
        // behind this readback on the same stream, and the next warp into the slot waits for ev_d2h[slot], recorded behind both
        if (int rc = ensure_out_stage(c)) return rc;
        void* st = c->out_stage[out_slot(c, c->out_target)].get();
        hf::launch_planar_out(c->g.hdr, c->g.H, c->g.out_stride, c->out_target, st, c->io_out.get());
        HF_HIP(c, hipGetLastError());
        from = st;
    }
    HF_HIP(c, hipMemcpyAsync(pinned_host_out, from, c->out_bytes, hipMemcpyDeviceToHost, c->io_out.get()));
    HF_HIP(c, hipEventRecord(c->ev_dl[c->dl_issued % hf_ctx::kDlRing].get(), c->io_out.get()));
    c->dl_issued++;
    for (int i = 0; i < hf_ctx::kOutRing; i++)
        if (c->out_target == c->out_at(i)) {   // internal output: the next frame goes to the next ring slot
            HF_HIP(c, hipEventRecord(c->ev_d2h[i].get(), c->io_out.get()));
            c->d2h_pending[i] = true;
            c->out_idx = (i + 1) % hf_ctx::kOutRing;
            c->out_target = c->out_at(c->out_idx);
            break;
        }
    c->warp_started = false;
    return HF_OK;
}

int hf_planar_convert_device(hf_ctx* c, int to_planar, const void* device_src, void* device_dst) {
    HF_CHECK_CTX(c);
    if (!device_src || !device_dst) return fail(c, HF_ERR_INVALID_ARGUMENT, "hf_planar_convert_device: null buffer");
    if (int rc = set_device(c)) return rc;
    if (to_planar) hf::launch_planar_out(c->g.hdr, c->g.H, c->g.out_stride, device_src, device_dst, c->stream);
    else hf::launch_planar_in(c->g.hdr, c->g.H, c->g.in_stride, device_src, device_dst, c->stream);
    HF_HIP(c, hipGetLastError());
    if (!c->async()) return sync_ctx(c);
    return HF_OK;
}

int hf_wait_flow(hf_ctx* c) {
    HF_CHECK_CTX(c);
    if (int rc = set_device(c)) return rc;
    if (!c->async()) return HF_OK;                       // blocking contexts have finished every call already
    if (c->batch) return fail(c, HF_ERR_STATE, "hf_wait_flow: the context is a member of a batch (use hf_sync)");
    if (!c->flow_done_recorded) return HF_OK;
    HF_HIP(c, hipEventSynchronize(c->ev_flow_done.get()));
    if (c->delta_pending) { c->total_frame_delta = *c->h_total_delta; c->delta_pending = false; }
    return HF_OK;
}

uint64_t hf_downloads_issued(const hf_ctx* c) { return c ? c->dl_issued : 0; }

int hf_wait_download(hf_ctx* c, uint64_t index) {
    HF_CHECK_CTX(c);
    if (index >= c->dl_issued) return fail(c, HF_ERR_INVALID_ARGUMENT, "hf_wait_download: download %llu has not been issued (%llu so far)",
                                           (unsigned long long)index, (unsigned long long)c->dl_issued);
    if (int rc = set_device(c)) return rc;
    // The ring keeps the events of the last kDlRing downloads.  A slot that has been reused belongs to a LATER download of the same
    // in-order stream, so waiting for it (or, for an index older than the whole ring, for the oldest event still kept) implies that
    // download `index` has landed.
    const uint64_t oldest = c->dl_issued > (uint64_t)hf_ctx::kDlRing ? c->dl_issued - (uint64_t)hf_ctx::kDlRing : 0;
    const uint64_t wait_for = index < oldest ? oldest : index;
    HF_HIP(c, hipEventSynchronize(c->ev_dl[wait_for % hf_ctx::kDlRing].get()));
    return HF_OK;
}

}  // extern "C"
