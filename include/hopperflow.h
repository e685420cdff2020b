/* include/hopperflow.h -- C ABI of the MI355X-native optical-flow frame interpolator.
 *
 * This is the drop-in boundary for ONE hot path of HopperLogger/HopperRender: the
 * OpticalFlowCalc{SDR,HDR} calculator (reference HopperRender/opticalFlowCalc.h:24-138 and
 * opticalFlowCalc{SDR,HDR}.cpp).  The reference's filter talks to that path through a C++
 * class; include/opticalFlowCalc.h re-creates that class source-compatibly ON TOP of this C
 * ABI, and any other host language binds these symbols directly.
 *
 * Conventions: plain C types only; every call returns 0 on success or a negative hf_status;
 * nothing throws; hf_last_error() returns a human-readable string for the last failure of
 * that context (or of hf_create when ctx == NULL).  Strides are in ELEMENTS (uint8 for NV12,
 * uint16 for P010), exactly like the reference (opticalFlowCalcHDR.cpp:20,279-282).
 * One context = one GPU + one HIP stream; a context is not thread-safe (reference: one object
 * per filter instance); contexts are independent of each other, also
 * on the same device, which is how independent frame pairs are batched and sharded.
 *
 * All file:line citations are relative to the reference's HopperRender/ directory.
 */
#ifndef HOPPERFLOW_H
#define HOPPERFLOW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HF_ABI_VERSION 6

typedef struct hf_ctx hf_ctx;

typedef enum hf_status {
    HF_OK = 0,
    HF_ERR_INVALID_ARGUMENT = -1, /* bad config / NULL pointer / blending scalar > 1 (opticalFlowCalcSDR.cpp:143-146) */
    HF_ERR_NO_DEVICE = -2,        /* no HIP device satisfies the request (reference: detectDevices throws, opticalFlowCalc.cpp:97-109) */
    HF_ERR_OUT_OF_MEMORY = -3,
    HF_ERR_HIP = -4,              /* a HIP runtime call failed (reference: CHECK_ERROR, opticalFlowCalc.h:15-22) */
    HF_ERR_STATE = -5             /* the object is in a state that excludes the call: a context that already belongs to a
                                     batch handed to hf_batch_create, asynchronous host I/O on a batch member */
} hf_status;

/* Frame output modes of warpFrames (reference HopperRender.h:10-18, warpFrameKernelSDR.h:133-183). */
typedef enum hf_output_mode {
    HF_MODE_WARPED_FRAME_12 = 0,
    HF_MODE_WARPED_FRAME_21 = 1,
    HF_MODE_BLENDED_FRAME = 2,
    HF_MODE_HSV_FLOW = 3,
    HF_MODE_GREY_FLOW = 4,
    HF_MODE_SIDE_BY_SIDE_1 = 5,
    HF_MODE_SIDE_BY_SIDE_2 = 6
} hf_output_mode;

#define HF_FLAG_ASYNC 0x1 /* calls only enqueue; results/timings valid after hf_sync(). Default: every
                             call blocks like the reference (CL_TRUE transfers, clWaitForEvents). */
#define HF_FLAG_NO_GRAPH 0x2 /* launch the flow chain eagerly instead of replaying a hipGraph (debug) */
#define HF_FLAG_PROFILE 0x4  /* bracket every warp/copy launch and every flow chain with HIP events on ctx's
                                stream; totals are read with hf_get_profile() (bench.py's live roofline figure) */
#define HF_FLAG_NO_LAZY_ARGMIN 0x8 /* large windows: take every argmin in a launch of its own (debug / A-B timing) */
#define HF_FLAG_DUAL_STREAM 0x40 /* async hosts: warp kernels on a second stream of the context.  warpFrames consumes the
                                    PREVIOUS flow and frames N-2/N-1 (opticalFlowCalcSDR.cpp:154-156) while
                                    calculateOpticalFlow produces the next flow from N-1/N into the other buffer, so the two
                                    overlap inside one context; events keep every other ordering intact */
#define HF_FLAG_NO_FUSED_WARP 0x80 /* hf_interpolate_period: one warp launch per output frame (debug / A-B timing) */
#define HF_FLAG_BATCH_NORMAL_PRIORITY 0x800 /* on the leader passed to hf_batch_create: give the batch a normal-priority stream
                                                (default: highest priority, see hf_batch_create) */
#define HF_FLAG_BATCH_EAGER_PLANES 0x1000 /* on the leader passed to hf_batch_create: hf_batch_run_period builds every phase plane in
                                              full when its frame arrives (default for large frames: grid samples only, the full
                                              plane comes out of the next period's warp launch -- see hf_batch_run_period) */
#define HF_FLAG_NO_SAD_REUSE 0x2000 /* flow chain: recompute every candidate SAD at every step, as the reference does, instead of summing the per-block SAD
                                     * tables of the last step that sampled the same positions (same results; debug / A-B timing) */
#define HF_FLAG_SAD_REUSE_ALWAYS 0x4000 /* flow chain: keep the SAD tables whatever the content (default: the chain reports how many windows kept their
                                         * offsets and the next chains drop the tables while hardly any does -- same results, other kernels) */
#define HF_FLAG_NO_TIMING 0x200 /* do not record the events behind m_ofcCalcTime / m_warpCalcTime (hf_stats times stay 0).
                                   Every timing event is a barrier packet on the stream: measured 5-6 us each between
                                   back-to-back kernels, ~15 us per source period in a throughput pipeline */
/* Planar 4:2:0 frames (yuv420p / yuv420p10le, e.g. the frames of a .y4m file or of an ffmpeg rawvideo pipe) instead of NV12 / P010 at
 * the boundary.  The two flags are independent.  A planar frame of H rows, stride S (input_stride for inputs, output_stride for outputs,
 * in elements; must be even) and width W holds 1.5 H S elements -- the same bytes as the NV12 / P010 frame, so input_frame_bytes,
 * output_frame_bytes and every buffer size stay as they are:
 *     Y(y, x)  at  y S + x                              0 <= y < H,   0 <= x < W
 *     U(m, k)  at  H S + m (S/2) + k                     0 <= m < H/2, 0 <= k < W/2
 *     V(m, k)  at  H S + (H/2)(S/2) + m (S/2) + k
 * In:  NV12.Y(y, x) = Y(y, x), UV(m, 2k) = U(m, k), UV(m, 2k+1) = V(m, k); HDR values are LSB-aligned 10-bit (yuv420p10le) and become
 *      (v << 6) & 0xFFFF (values above 1023 lose their top bits).  Padding columns [W, S) of a planar input are never read.
 * Out: the inverse; HDR values become v >> 6 (the low 6 bits of the P010 value are dropped).  Padding columns of a planar output are
 *      unspecified.
 * The conversion is a kernel of its own at the boundary (csrc/hf_planar.hip); flow, m_totalFrameDelta, phase planes, diagnostics and timings
 * are those of the NV12 / P010 path.  Entry points that honour them:
 *   PLANAR_IN   hf_update_frame, hf_update_frame_device, hf_update_frame_device_ref (converts: no zero-copy reference, see there),
 *               hf_update_frame_async, the device_frame of hf_interpolate_period(_ex), hf_filter_deliver's host_in, hf_hostio's fill buffers
 *   PLANAR_OUT  hf_download_frame, hf_download_frame_async, hf_download_frame_device, the device_out of hf_interpolate_period(_ex),
 *               hf_filter_deliver's host_out, hf_hostio's sink frames; hf_set_output_buffer(ctx, non-NULL) returns HF_ERR_STATE
 * Contexts with either flag cannot join a batch (hf_batch_create returns HF_ERR_INVALID_ARGUMENT).  Staging buffers are allocated on
 * first use: up to three frames per side for host I/O, one semi-planar frame per output of hf_interpolate_period. */
#define HF_FLAG_PLANAR_IN 0x8000
#define HF_FLAG_PLANAR_OUT 0x10000
/* The same layout at the boundary of a BATCH.  Read only from the leader passed to hf_batch_create, like HF_FLAG_BATCH_EAGER_PLANES; a
 * context's own calls ignore them and the members stay ordinary NV12 / P010 contexts (see hf_batch_create). */
#define HF_FLAG_BATCH_PLANAR_IN 0x20000  /* the batch's input frames are planar */
#define HF_FLAG_BATCH_PLANAR_OUT 0x40000 /* the batch's caller-owned outputs are planar */
#define HF_FLAG_BATCH_AUTO_DEFERRED 0x80000 /* on the leader passed to hf_batch_create: hf_batch_run_period_auto(_wide) accepts a batch that defers its
                                             * phase planes (hf_batch_defers_planes) and keeps the deferred order -- grid samples at update time, the
                                             * warps of the period's first six outputs per member ahead of its chain, where they build the planes; only
                                             * the predicated copy and the planar conversion of those outputs wait for the decision.  Same outputs,
                                             * records and state as the HF_FLAG_BATCH_EAGER_PLANES twin.  No effect on a batch that does not defer, on
                                             * hf_batch_run_period and the three separate calls, on the HF_FLAG_DUAL_STREAM refusal.  Without it the
                                             * auto call refuses a deferring batch, as ABI 6 documents; the flag becomes the default at the next ABI
                                             * bump.  Additive to ABI version 6. */
/* (0x10, 0x20, 0x100, 0x400 were round-1 stream-topology experiments -- shared warp stream, priority streams, warp
 *  turnstile, deferred phase planes -- all measured slower or equal; removed, findings in DESIGN.md section 4) */

/* The nine constructor arguments of OpticalFlowCalcSDR/HDR (opticalFlowCalcSDR.cpp:206-208)
 * plus build-side extensions (0 selects the reference behaviour for each). */
typedef struct hf_config {
    uint32_t struct_size;   /* = sizeof(hf_config), for ABI evolution */
    int32_t is_hdr;         /* 0: NV12 8-bit (OpticalFlowCalcSDR), 1: P010 16-bit (OpticalFlowCalcHDR) */
    int32_t frame_height;   /* ctor arg 1 */
    int32_t frame_width;    /* ctor arg 2 */
    int32_t input_stride;   /* ctor arg 3, elements; <= 0 -> frame_width (:212) */
    int32_t output_stride;  /* ctor arg 4, elements; <= 0 -> frame_width (:213) */
    int32_t delta_scalar;   /* ctor arg 5, config.h:23 default 8 */
    int32_t neighbor_scalar;/* ctor arg 6, config.h:24 default 6 */
    float black_level;      /* ctor arg 7, 0..255 */
    float white_level;      /* ctor arg 8, 0..255 */
    int32_t max_calc_res;   /* ctor arg 9, config.h:4 default 270 */
    /* --- extensions --- */
    int32_t device_index;   /* HIP device ordinal, or -1 = the first suitable device like the reference's detectDevices
                               (opticalFlowCalc.cpp:67-93); hf_get_device() tells which one it became */
    int32_t iterations;     /* NUM_ITERATIONS (config.h:6) made runtime; 0 = auto */
    int32_t blur_radius;    /* KERNEL_RADIUS (blurFlowKernelSDR.h:4) made runtime; 0 -> 4 */
    int32_t search_radius;  /* initial m_opticalFlowSearchRadius; 0 -> MIN_SEARCH_RADIUS 5 (:216) */
    uint32_t flags;         /* HF_FLAG_* */
} hf_config;

/* The public fields the filter reads/writes on the calculator (opticalFlowCalc.h:27-48). */
typedef struct hf_params {
    int32_t delta_scalar;    /* m_deltaScalar           (r/w by the settings thread, HopperRender.cpp:1385-1390) */
    int32_t neighbor_scalar; /* m_neighborBiasScalar */
    float black_level;       /* m_outputBlackLevel */
    float white_level;       /* m_outputWhiteLevel */
    int32_t search_radius;   /* m_opticalFlowSearchRadius, 5..16 (governor, HopperRender.cpp:1438-1463) */
    uint32_t frame_count;    /* m_frameCount (NewSegment zeroes it, HopperRender.cpp:840) */
} hf_params;

typedef struct hf_stats {
    uint32_t total_frame_delta; /* m_totalFrameDelta (bug-compatible, opticalFlowCalcSDR.cpp:91-94) */
    uint32_t frame_count;       /* m_frameCount */
    double ofc_calc_time;       /* m_ofcCalcTime: upload start -> blur end, seconds (:125-127) */
    double ofc_avg_calc_time;   /* m_ofcAvgCalcTime (:128-133) */
    double ofc_peak_calc_time;  /* m_ofcPeakCalcTime (:131,136-138) */
    double warp_calc_time;      /* m_warpCalcTime: first warp/copy launch -> readback end (:36-41) */
    int32_t res_scalar;         /* m_opticalFlowResScalar */
    int32_t low_width;          /* m_opticalFlowFrameWidth */
    int32_t low_height;         /* m_opticalFlowFrameHeight */
    int32_t frame_width, frame_height, input_stride, output_stride;
    int32_t iterations;         /* effective refinement iterations of the last flow calc */
    int32_t initial_window;     /* first window size (opticalFlowCalcSDR.cpp:49-59) */
    uint64_t input_frame_bytes; /* bytes updateFrame reads  = bpp*(H*S_in + (H/2)*S_in)  (:20) */
    uint64_t output_frame_bytes;/* bytes downloadFrame writes = bpp*(H*S_out + (H/2)*S_out) (:33) */
    uint64_t phase_plane_bytes; /* bytes of one phase plane (this build's re-laid copy of a frame) */
    int32_t sad_tables;         /* 1: the last flow calc kept SAD tables (exact cross-step reuse, csrc/hf_flow.hip), 0: it recomputed every step */
    float still_share;          /* smoothed share of 32-windows that chose d = 0 on both axes in the last chains (what switches the tables off on
                                 * content where hardly any window keeps its offsets; < 0: no report yet) */
} hf_stats;

/* ---- lifecycle: constructor / destructor (opticalFlowCalcSDR.cpp:206-325, :185-204) ---- */
int hf_create(const hf_config* cfg, hf_ctx** out_ctx);
void hf_destroy(hf_ctx* ctx);
const char* hf_last_error(const hf_ctx* ctx);
int hf_abi_version(void);

/* detectDevices (opticalFlowCalc.cpp:45-109) as a pure function over a capability table, so that the rule can be tested
 * without hardware: index of the FIRST entry with vram_bytes >= required_vram_bytes, >= 2048 bytes of LDS per workgroup,
 * workgroups of 256 threads (16 x 16) and 64-wide wavefronts, or -1.  why_not (optional) receives the reference's messages
 * for the last entry inspected (:98-108).  hf_create(device_index = -1) applies it to the HIP devices (vram = total device
 * memory, as the reference compares CL_DEVICE_GLOBAL_MEM_SIZE) and then insists on that much FREE memory, moving on if not. */
typedef struct hf_device_caps {
    uint64_t vram_bytes;
    uint64_t lds_bytes_per_workgroup;
    int32_t max_threads_per_workgroup;
    int32_t wavefront_size;
} hf_device_caps;
int hf_select_device(const hf_device_caps* caps, int n, uint64_t required_vram_bytes, char* why_not, size_t why_not_size);
int hf_get_device(const hf_ctx* ctx);   /* the HIP ordinal the context lives on */

/* ---- the five virtuals of OpticalFlowCalc (opticalFlowCalc.h:100-132) ---- */
/* updateFrame (opticalFlowCalcSDR.cpp:19-29): upload one NV12/P010 frame, rotate the 3-frame ring, frame_count++ */
int hf_update_frame(hf_ctx* ctx, const void* host_frame);
/* calculateOpticalFlow (opticalFlowCalcSDR.cpp:44-139): flow between ring[1] (N-1) and ring[2] (N) */
int hf_calculate_optical_flow(hf_ctx* ctx);
/* warpFrames (opticalFlowCalcSDR.cpp:141-168): blending_scalar in [.., 1], mode = hf_output_mode */
int hf_warp_frames(hf_ctx* ctx, float blending_scalar, int frame_output_mode);
/* copyFrame (opticalFlowCalcSDR.cpp:170-183) */
int hf_copy_frame(hf_ctx* ctx);
/* downloadFrame (opticalFlowCalcSDR.cpp:31-42): blocking readback of the output frame */
int hf_download_frame(hf_ctx* ctx, void* host_out);

/* ---- public-field access ---- */
int hf_get_params(const hf_ctx* ctx, hf_params* out);
int hf_set_params(hf_ctx* ctx, const hf_params* in);
int hf_get_stats(hf_ctx* ctx, hf_stats* out);

/* ---- device-resident variants (batch driver / benchmarks: inputs and outputs stay in HBM) ---- */
/* Same as hf_update_frame but the source is a device pointer on ctx's device (device-to-device). */
int hf_update_frame_device(hf_ctx* ctx, const void* device_frame);
/* Asynchronous host I/O on side streams of the context (page-locked buffers, e.g. hf_host_malloc_pinned): the
 * upload of frame N+1 and the readback of finished output frames overlap the flow chain and the warps; nothing
 * blocks, hf_sync() waits for everything.  The host buffers must stay valid (and, for the readback, unread) until
 * hf_sync().  Output frames rotate through an internal ring of three device buffers so that the next warp does
 * not wait for the previous readback. */
int hf_update_frame_async(hf_ctx* ctx, const void* pinned_host_frame);
int hf_download_frame_async(hf_ctx* ctx, void* pinned_host_out);
/* Streaming hosts (the multi-GPU driver, hopperrender_amd/hostio.py): what the host must know WITHOUT draining the side streams.
 *   hf_wait_flow      blocks until the last hf_calculate_optical_flow of an asynchronous context has finished and makes its
 *                     m_totalFrameDelta visible in hf_get_stats -- the filter decides warp vs copy from it (HopperRender.cpp:
 *                     959-972,1126-1176) while uploads and readbacks keep running;
 *   hf_wait_download  blocks until the index-th hf_download_frame_async of this context (0, 1, 2 ... in issue order;
 *                     hf_downloads_issued() = how many there are) has landed in its host buffer. */
int hf_wait_flow(hf_ctx* ctx);
uint64_t hf_downloads_issued(const hf_ctx* ctx);
int hf_wait_download(hf_ctx* ctx, uint64_t index);
/* Zero-copy variant: the ring keeps a REFERENCE to device_frame (e.g. a decoder surface).  The caller must
 * leave the frame untouched until three further frames have been submitted (it stays in the 3-frame ring
 * as frame N, N-1 and N-2, opticalFlowCalcSDR.cpp:22-28).  Under HF_FLAG_PLANAR_IN the frame is converted into the
 * context's own ring slot instead: the caller's buffer is free once ctx's stream has passed the call. */
int hf_update_frame_device_ref(hf_ctx* ctx, const void* device_frame);
/* One source-frame period in a single call (batch driver): hf_update_frame_device_ref(device_frame) if it is
 * non-NULL, hf_calculate_optical_flow(), then for i < n_out: hf_warp_frames(t[i], mode) written to
 * device_out[i].  Same results as the individual calls; only the host overhead differs. */
int hf_interpolate_period(hf_ctx* ctx, const void* device_frame, int n_out, const float* t, void* const* device_out, int mode);
/* update_and_flow = 0: only the warps of the period (no updateFrame, no calculateOpticalFlow). */
int hf_interpolate_period_ex(hf_ctx* ctx, const void* device_frame, int n_out, const float* t, void* const* device_out, int mode,
                             int update_and_flow);
/* ---- Batched flow calculation (throughput drivers) -------------------------------------------------------------
 * The reference computes one pair at a time (opticalFlowCalcSDR.cpp:44-139: 66 enqueues per call).  Its flow grid is
 * at most 480x270, so one refinement chain is a sequence of small latency-bound launches that cannot fill 256 CUs.
 * A driver that converts INDEPENDENT frame pairs groups up to 32 contexts of identical
 * geometry/parameters into a batch: hf_batch_calculate_optical_flow() runs the calculateOpticalFlow() of every
 * member as ONE set of launches (each kernel handles all pairs).  Results per member are bit-identical to
 * hf_calculate_optical_flow(member).
 *   - members: HF_FLAG_ASYNC contexts without async host I/O, all single-stream or all HF_FLAG_DUAL_STREAM, same device, frame geometry, iterations, blur radius; at call time the same search
 *     radius / delta / neighbor scalar.  DUAL_STREAM members issue their warps on up to 3 streams the batch shares
 *     out round robin (they overlap the batched chain; measured slower than single-stream batches).
 *   - the batch issues on a stream of its own of the HIGHEST priority.  Not for the priority: the HIP runtime keeps one pool of
 *     hardware queues per priority and nobody else creates such streams, so the batch streams of a process land on different
 *     hardware queues whatever was created before them (DESIGN.md "Streams and hardware queues").  SIDE EFFECT: the priority is
 *     real -- batch launches are scheduled ahead of every normal-priority stream of the process (other contexts' work and
 *     asynchronous I/O, RCCL).  A host that mixes batches with latency-sensitive single contexts passes
 *     HF_FLAG_BATCH_NORMAL_PRIORITY on the leader; if the priority range cannot be queried the batch falls back to a normal stream.
 *   - while the batch exists all members issue on ONE stream (the batch's own): their hf_update_frame_device*,
 *     hf_interpolate_period_ex(..., update_and_flow = 0), hf_sync ... calls keep working and stay in program order
 *     with the batched chain.  Destroy the batch before its members. */
typedef struct hf_batch hf_batch;
int hf_batch_create(hf_ctx* const* members, int n, hf_batch** out_batch);
void hf_batch_destroy(hf_batch* batch);
int hf_batch_calculate_optical_flow(hf_batch* batch);
/* hf_update_frame_device_ref(member i, device_frames[i]) for every member, the phase planes of all new frames built by
 * ONE launch. */
int hf_batch_update_frames_device_ref(hf_batch* batch, const void* const* device_frames);
/* hf_interpolate_period_ex(member i, NULL, n_out[i], t + 6 i, device_out + 6 i, mode, 0) for every member: the warps of
 * one source period of EVERY member that has an output in ONE launch (single-stream members, modes 0-2; otherwise
 * member by member).  t and device_out are [batch size][HF_MAX_PERIOD_OUTPUTS] arrays; a NULL device_out entry
 * selects the member's internal output frame. */
#define HF_MAX_PERIOD_OUTPUTS 6
int hf_batch_interpolate_period(hf_batch* batch, const int* n_out, const float* t, void* const* device_out, int mode);
/* One source period of the whole batch in ONE call (what a throughput driver issues per period -- three calls' worth of
 * argument marshalling matter when a period is ~70 us of GPU time): hf_batch_update_frames_device_ref(device_frames) unless
 * device_frames == NULL, hf_batch_calculate_optical_flow() if calculate_flow, hf_batch_interpolate_period(n_out, t,
 * device_out, mode) unless n_out == NULL.  Same results and same error behaviour as the three calls.
 * Where the batched period warp is the workgroup-staged kernel (batches of frames > 1080p, one flow cell per 16-byte thread) the
 * call defers the phase planes: at update time only the grid samples of the new frame are taken, and the full plane of frame
 * N-1, which the chain of the NEXT period reads, is built by that period's warp launch -- it reads the frame anyway -- which
 * is then enqueued ahead of the period's chain (it uses the previous flow and frames N-2 / N-1, so the order is free).  Saves
 * the stand-alone plane kernel's re-read of every frame.  Any period that cannot do that (no outputs, diagnostic modes, a
 * separate hf_batch_calculate_optical_flow / hf_calculate_optical_flow call) builds the missing plane with the stand-alone
 * kernel first.  Side effect: m_ofcCalcTime of the members then includes the warp launch.  HF_FLAG_BATCH_EAGER_PLANES on the
 * leader turns it off. */
int hf_batch_run_period(hf_batch* batch, const void* const* device_frames, int calculate_flow, const int* n_out, const float* t,
                        void* const* device_out, int mode);
/* 1: hf_batch_run_period defers the phase planes of this batch (see above); 0: it builds them eagerly. */
int hf_batch_defers_planes(const hf_batch* batch);
/* ---- Planar 4:2:0 clips through a batch (layout, strides and HDR shifts: the comment at HF_FLAG_PLANAR_IN above) ----
 * HF_FLAG_BATCH_PLANAR_IN on the leader: the device_frames of hf_batch_update_frames_device_ref, hf_batch_run_period and
 *   hf_batch_run_period_auto are planar.  ONE launch on the batch stream, ahead of the phase-plane launch, converts the new frame of every
 *   member into the member's own ring slot; the ring references that slot, so a caller's frame is free once the batch stream has passed the
 *   call (no three-period hold -- the rule of hf_update_frame_device_ref under HF_FLAG_PLANAR_IN).
 * HF_FLAG_BATCH_PLANAR_OUT on the leader: the non-NULL device_out entries of hf_batch_interpolate_period, hf_batch_run_period and
 *   hf_batch_run_period_auto receive planar frames.  The period's warps (every output mode; in the auto call the predicated copy too)
 *   write semi-planar frames into stages the library owns -- per member as many output frames as the largest n_out seen, allocated on
 *   first use, freed with the batch -- and ONE launch behind them converts every output of every member into the caller's buffers.  A
 *   NULL entry still selects the member's internal output frame, which stays NV12 / P010 (hf_download_frame_device of the member).
 * Flow, m_totalFrameDelta, phase planes (deferred or eager), scene records and timings are those of a plain batch fed the NV12 / P010
 * twins of the frames.  hf_batch_create returns HF_ERR_INVALID_ARGUMENT for an odd stride on a planar side and for either flag with
 * HF_FLAG_DUAL_STREAM members; contexts with HF_FLAG_PLANAR_IN / _OUT of their own are refused as before.  Additive to ABI version 6.
 * hf_batch_planar: bit 0 = planar in, bit 1 = planar out; 0 for NULL. */
int hf_batch_planar(const hf_batch* batch);
/* ---- Whole clips through a batch: scene-cut copy periods decided on the device ----
 * The reference's filter shows a source period as warpFrames or as copyFrame, decided from the m_totalFrameDelta history
 * (HopperRender.cpp:959-972, 1126-1183; hf_filter_push_frame_delta / hf_filter_detect_scene_change).  The decision needs the delta of the
 * period's own chain, so a host that takes it waits once per period (hf_wait_flow) -- which a batch cannot afford.  Here it follows the
 * chain onto the batch stream: a tiny kernel behind the chain's last launch pushes every member's delta into the member's history (the
 * function of csrc/hf_scene.h, the same integer arithmetic as hf_filter.cpp:130-161) and leaves its kind on the device; the period's warps
 * are the unchanged fused launch; a predicated copy launch behind them overwrites the outputs of the members whose period turned out to be
 * a scene change with exactly what hf_copy_frame writes (members without one leave it at once).  Nothing waits on the host.
 *   hf_batch_scene_set        arms / re-arms one member: its history starts over (NewSegment).  source_frame_time (100-ns units, <= 0 ->
 *                             417083) sets the 3-second window; threshold < 0 = DEFAULT_SCENE_CHANGE_THRESHOLD.  A host starts a new clip
 *                             in a slot with hf_set_params(frame_count = 0) + hf_batch_scene_set.
 *   hf_batch_run_period_auto  one source period of every member; only enqueues: hf_batch_update_frames_device_ref,
 *                             hf_batch_calculate_optical_flow, the decision, hf_batch_interpolate_period, the predicated copy.  A member
 *                             whose m_frameCount is below 3 rides the same launches (its ring always holds valid buffers) and its outputs
 *                             are copies of the frame hf_copy_frame shows; its delta is not pushed and its flow buffers do not move, as if
 *                             calculateOpticalFlow had not been called for it.  force_kind: NULL, or per member -1 decide, 0 copy, 1 warp.
 *                             n_out[m] == 0 writes nothing for member m; its history still advances.  Any output mode (diagnostic modes
 *                             warp member by member on the same stream).  Every period of an armed member must go through this call: the
 *                             history assumes consecutive m_frameCount values (re-arm after anything else).
 *                             HF_ERR_STATE, nothing enqueued: a batch that defers its phase planes (hf_batch_defers_planes) whose leader
 *                             carries neither HF_FLAG_BATCH_AUTO_DEFERRED nor HF_FLAG_BATCH_EAGER_PLANES, HF_FLAG_DUAL_STREAM members, a
 *                             member that was never armed, a record ring that would overflow.
 *                             On a deferring batch with HF_FLAG_BATCH_AUTO_DEFERRED the period keeps hf_batch_run_period's order: the update
 *                             samples only the grid, and where that call would send chunk 0 ahead (some member's older plane pending, mode
 *                             0 .. 2, every member has an output, the one-launch warp qualifies) its WARPS go out ahead of the chain and
 *                             build the planes; chain and decision follow; then chunk 0's predicated copy and planar conversion, then the
 *                             later chunks whole.  Every other period takes the order above and the chain's stand-alone plane launch fills
 *                             in.  Everything a host can observe equals the HF_FLAG_BATCH_EAGER_PLANES twin (a member whose m_frameCount is
 *                             below 3 is warped early with the flow buffer its chain does not write, and then overwritten by the copy; only
 *                             force_kind 1 on such a member, whose flow means nothing either way, could show it).  Error behaviour is
 *                             hf_batch_run_period's on such a batch: every argument, the chain's included, is checked before the first
 *                             enqueue; once the early launch is enqueued an error is final.  m_ofcCalcTime then includes the early warps.
 *   hf_batch_scene_read       after hf_batch_sync: the records of one member since the last read, in period order.  *n_records = how many
 *                             there were; min(capacity, *n_records) are copied and leave the ring.  The ring holds 128 periods per member.
 * Additive to ABI version 6: no existing struct or call changed. */
typedef struct hf_scene_record {
    uint32_t frame_count;        /* m_frameCount of the period */
    uint32_t total_delta;        /* m_totalFrameDelta pushed for it (0: m_frameCount < 3, nothing pushed) */
    int32_t kind;                /* 1 warp, 0 copy: what the period's outputs are */
    int32_t average, d1, d2;     /* hf_filter_state: average_frame_delta, scene_change_delta1 / 2 -- of the last decision that had 3 deltas */
} hf_scene_record;
int hf_batch_scene_set(hf_batch* batch, int member, int64_t source_frame_time, int32_t threshold);
int hf_batch_run_period_auto(hf_batch* batch, const void* const* device_frames, const int* n_out, const float* t, void* const* device_out,
                             int mode, const int32_t* force_kind);
int hf_batch_scene_read(hf_batch* batch, int member, hf_scene_record* out, int capacity, int* n_records);
/* ---- Periods of more than HF_MAX_PERIOD_OUTPUTS outputs (24 fps -> 144 Hz and above) ----
 * The three period calls above with t and device_out as [batch size][row] arrays, 1 <= row <= HF_MAX_PERIOD_OUTPUTS_WIDE, and n_out[m] in
 * [0, row]; the calls above are these with row = HF_MAX_PERIOD_OUTPUTS and keep refusing a seventh output.  Everything else -- NULL
 * device_out entries, force_kind, n_out[m] == 0, the planar flags of the leader, the three-calls equivalence of hf_batch_run_period, what
 * hf_batch_run_period_auto refuses and with which code -- is the narrow call's.  No new device code: a period goes out in chunks of up to
 * HF_MAX_PERIOD_OUTPUTS outputs per member (chunk c = outputs [6 c, 6 c + 6), the split of hf_interpolate_period_ex), each chunk the fused
 * launch over the members that have outputs in it, in the auto call followed by its predicated copy, under HF_FLAG_BATCH_PLANAR_OUT by its
 * conversion launch; the decision and the scene record stay one per member and period, and a member never owns more than
 * HF_MAX_PERIOD_OUTPUTS planar stages.  On a batch that defers its phase planes chunk 0 goes out ahead of the chain and builds the
 * planes, the other chunks follow the chain.  Additive to ABI version 6. */
#define HF_MAX_PERIOD_OUTPUTS_WIDE 24   /* 23.976 -> 480 Hz: 21 */
int hf_batch_interpolate_period_wide(hf_batch* batch, int row, const int* n_out, const float* t, void* const* device_out, int mode);
int hf_batch_run_period_wide(hf_batch* batch, const void* const* device_frames, int calculate_flow, int row, const int* n_out,
                             const float* t, void* const* device_out, int mode);
int hf_batch_run_period_auto_wide(hf_batch* batch, const void* const* device_frames, int row, const int* n_out, const float* t,
                                  void* const* device_out, int mode, const int32_t* force_kind);
int hf_batch_sync(hf_batch* batch);   /* hf_sync() of every member */
int hf_batch_size(const hf_batch* batch);
const char* hf_batch_last_error(const hf_batch* batch);   /* batch == NULL: error of the last failed hf_batch_create (per thread) */

/* ---- Frame error sums on the device: how far two frames are apart, without reading them back ----
 * What a leave-one-out quality evaluation needs (withhold every second frame, interpolate it, compare: hopperrender_amd/quality.py), and
 * a cheap "how many elements differ, and by how much" for tests.  One launch compares up to HF_MAX_ERROR_PAIRS pairs (a[i], b[i]) of
 * frames of ctx's geometry (frame_width, frame_height, 8 or 16 bit); each side has its own stride in elements (>= frame_width), and
 * both frames of a pair are NV12 / P010 (planar = 0) or both planar as defined at HF_FLAG_PLANAR_IN (planar = 1: even strides).  Per
 * plane -- index 0 Y, 1 U, 2 V, interleaved UV split -- over the elements of columns [0, frame_width) (chroma: [0, frame_width / 2)):
 *     sse = sum (a - b)^2    sad = sum |a - b|    max_abs = max |a - b|    n_differ = #(a != b)    count = elements compared
 * Values are compared as stored (raw 16-bit P010 words; LSB-aligned words in planar HDR frames).  Padding columns [frame_width, stride)
 * are never read, so an output's unspecified padding cannot reach a sum.  Integer sums: the results are exact and reproducible.
 *   hf_frame_error_enqueue  only enqueues: zeroes result slots [first_slot, first_slot + n) of ctx and compares pair i into slot
 *                           first_slot + i.  Ordered like hf_download_frame_device: behind every warp, copy and update ctx has enqueued
 *                           (the warp stream of an HF_FLAG_DUAL_STREAM context included); a batch member enqueues onto its batch's stream.
 *                           So a driver calls it straight after hf_interpolate_period / hf_batch_run_period* with no sync, and reads
 *                           the slots at the end of the clip.  The frames must stay as they are until the comparison has run.
 *   hf_frame_error_read     waits for ctx's work (hf_sync) and copies n slots out.
 *   hf_frame_error          one pair, blocking; uses a slot of its own outside [0, HF_ERROR_SLOTS).
 * HF_ERR_INVALID_ARGUMENT with nothing enqueued: NULL tables or entries, n outside [1, HF_MAX_ERROR_PAIRS], a slot range outside
 * [0, HF_ERROR_SLOTS), a stride below frame_width, an odd stride with planar = 1.  The slots (28 KB) are allocated on first use and
 * freed with the context.  Additive to ABI version 6. */
#define HF_MAX_ERROR_PAIRS 192
#define HF_ERROR_SLOTS 256
struct hf_frame_error {   /* index 0 Y, 1 U, 2 V.  A struct tag only, no typedef: the one-pair call below carries the same name, and in C a
                           * typedef name and a function share one name space (write `struct hf_frame_error`, in C++ too) */
    uint64_t sse[3], sad[3], n_differ[3], count[3];
    uint32_t max_abs[3];
    uint32_t reserved;
};
int hf_frame_error_enqueue(hf_ctx* ctx, int n, const void* const* device_a, const void* const* device_b, int stride_a, int stride_b,
                           int planar, int first_slot);
int hf_frame_error_read(hf_ctx* ctx, int first_slot, int n, struct hf_frame_error* out);
int hf_frame_error(hf_ctx* ctx, const void* device_a, const void* device_b, int stride_a, int stride_b, int planar,
                   struct hf_frame_error* out);

/* ---- Per-tile frame error maps on the device: WHERE two frames are apart ----
 * The error sums above reduce a frame to a few numbers per plane; a map keeps them per tile, so that a quality sweep or a parity test
 * learns where the error sits (a moving edge, the frame border, one flow window) without reading either frame back.  The pairs,
 * strides, layouts, planes and compared columns are those of hf_frame_error_enqueue (padding columns are never read); step by step:
 *   1. Tiles.  `tile` is the tile edge in luma pixels, 16, 32 or 64 (HF_ERROR_MAP_TILES_OK);  tw = (frame_width + tile - 1) / tile,
 *      th = (frame_height + tile - 1) / tile.
 *   2. Y, tile (i, j) covers rows [j tile, min((j + 1) tile, frame_height)) and columns [i tile, min((i + 1) tile, frame_width)).
 *      U and V, tile (i, j) covers chroma rows [j tile / 2, min((j + 1) tile / 2, frame_height / 2)) and chroma columns
 *      [i tile / 2, min((i + 1) tile / 2, frame_width / 2)) of that channel: the same picture area as the Y tile.
 *   3. Per tile, over its elements, in integers:  sse = sum (a - b)^2,  sad = sum |a - b|,  max_abs = max |a - b|  (a 64 x 64 tile of
 *      16-bit elements stays below 2^44 in sse and 2^28 in sad).
 *   4. One map is `struct hf_error_tile [3][th][tw]`, plane 0 Y, 1 U, 2 V: bytes_per_map = 48 tw th.  device_maps is ONE caller-owned
 *      device buffer of n bytes_per_map bytes, 16-byte aligned; the map of pair i starts at byte i bytes_per_map.  (One buffer, not a
 *      table of pointers: the tables of a and b take 3 KB of the 4 KB of kernel arguments at HF_MAX_ERROR_PAIRS already.)
 *   5. EVERY entry of every map is written by the launch, zeros included: the caller does not clear the buffer.  Per pair and plane
 *      the sum of sse over the tiles is hf_frame_error's sse, the sum of sad its sad, the largest max_abs its max_abs.
 *   hf_frame_error_map_shape    tw, th and bytes_per_map of ctx's geometry for a tile (any of the three results may be NULL).
 *   hf_frame_error_map_enqueue  only enqueues, ordered exactly like hf_frame_error_enqueue (behind every warp, copy and update of ctx,
 *                               the warp stream of an HF_FLAG_DUAL_STREAM context included; a batch member on its batch's stream).
 *                               Read the maps with hf_memcpy_d2h after hf_sync.  The frames must stay as they are until it has run.
 * HF_ERR_INVALID_ARGUMENT with nothing enqueued: everything hf_frame_error_enqueue refuses but the slot range (there are no slots), a
 * tile outside {16, 32, 64}, a NULL or misaligned device_maps.  Additive to ABI version 6. */
#define HF_ERROR_MAP_TILES_OK(t) ((t) == 16 || (t) == 32 || (t) == 64)
struct hf_error_tile { uint64_t sse; uint32_t sad; uint32_t max_abs; };   /* 16 bytes */
int hf_frame_error_map_shape(const hf_ctx* ctx, int tile, int* tiles_x, int* tiles_y, size_t* bytes_per_map);
int hf_frame_error_map_enqueue(hf_ctx* ctx, int n, const void* const* device_a, const void* const* device_b, int stride_a, int stride_b,
                               int planar, int tile, void* device_maps);

/* ---- Windowed SSIM on the device, beside the frame error sums ----
 * PSNR rewards smoothing (a ghost of two averaged frames scores above a sharp, slightly misplaced edge) and cannot tell a frame that is
 * a little wrong everywhere from one torn in a single place; structural similarity over small windows is the usual second judge, as a
 * mean and as a worst window.  This is the block form of x264 and of FFmpeg's `ssim` filter, with every step pinned so that the result
 * is a set of integers anyone can reproduce.  The pairs, strides, layouts and planes are those of hf_frame_error_enqueue; per plane of
 * w x h compared elements (padding columns are never read):
 *   1. Blocks.  bw = w >> 2, bh = h >> 2; block (i, j) covers rows 4 j .. 4 j + 3 and columns 4 i .. 4 i + 3 (the trailing w & 3 columns
 *      and h & 3 rows are not used).  Per block, in integers:  s1 = sum a,  s2 = sum b,  ss = sum (a^2 + b^2),  s12 = sum a b.
 *   2. Windows.  Window (i, j), 0 <= i < bw - 1, 0 <= j < bh - 1, is the 2 x 2 blocks (i, j) .. (i + 1, j + 1) -- 8 x 8 elements at
 *      stride 4; S1, S2, SS, S12 are the sums over its four blocks.  count = (bw - 1) (bh - 1), or 0 if bw < 2 or bh < 2.
 *   3. Constants, integers, with integer division:  c1 = (64 peak^2 + 5000) / 10000,  c2 = (9 * 64 * 63 peak^2 + 5000) / 10000
 *      (peak 255: 416 and 235963, FFmpeg's 8-bit constants; 65535: 27486952 and 15585101693; 1023: 6698 and 3797644).
 *   4. Window terms, in 64-bit integers (each stays below 2^53 in magnitude, so its conversion to double is exact):
 *          vars = 64 SS - S1^2 - S2^2      covar = 64 S12 - S1 S2
 *          A = 2 S1 S2 + c1      B = 2 covar + c2      C = S1^2 + S2^2 + c1      D = vars + c2
 *   5. Window score:  ssim = (double(A) * double(B)) / (double(C) * double(D)) -- two IEEE multiplications and one IEEE division, no
 *      contraction;  q = llrint(ssim * 2^32), round to nearest even (the multiplication is exact);  loss = 2^32 - q, an unsigned integer
 *      in [0, 2^33], 0 where the two windows are equal (then A == C and B == D).
 *   6. Per plane:  sum_loss_q32 = sum of loss,  max_loss_q32 = largest loss,  count.  Mean SSIM = 1 - sum_loss_q32 / 2^32 / count, worst
 *      window = 1 - max_loss_q32 / 2^32.  Integer sums: exact, independent of the order of addition; equal frames give zero losses.
 * peak: 0 selects 255 on an 8-bit context, 65535 on a 16-bit one with planar = 0 and 1023 with planar = 1 (LSB-aligned yuv420p10le);
 * otherwise 1 .. 255 on 8 bit and 1 .. 65535 on 16 bit.  (A peak below 9 makes c1 zero: a window that is zero on both sides then has
 * no score, 0 / 0, and what it adds is unspecified.)
 *   hf_frame_ssim_enqueue  only enqueues, ordered exactly like hf_frame_error_enqueue (behind every warp, copy and update of ctx, the
 *                          warp stream of an HF_FLAG_DUAL_STREAM context included; a batch member on its batch's stream): zeroes SSIM
 *                          slots [first_slot, first_slot + n) and scores pair i into slot first_slot + i.  The SSIM slots are their own:
 *                          the error slots of the same numbers are untouched.
 *   hf_frame_ssim_read     waits for ctx's work and copies n slots out; HF_ERR_STATE before any enqueue.
 *   hf_frame_ssim          one pair, blocking; uses a slot of its own outside [0, HF_SSIM_SLOTS).
 * HF_ERR_INVALID_ARGUMENT with nothing enqueued: everything hf_frame_error_enqueue refuses (with HF_SSIM_SLOTS as the slot bound), and
 * a peak outside its range.  The slots (18 KB) are allocated on first use and freed with the context.  Additive to ABI version 6. */
#define HF_SSIM_SLOTS 256
struct hf_frame_ssim {   /* index 0 Y, 1 U, 2 V; a struct tag only, like hf_frame_error */
    uint64_t sum_loss_q32[3], max_loss_q32[3], count[3];
};
int hf_frame_ssim_enqueue(hf_ctx* ctx, int n, const void* const* device_a, const void* const* device_b, int stride_a, int stride_b,
                          int planar, int peak, int first_slot);
int hf_frame_ssim_read(hf_ctx* ctx, int first_slot, int n, struct hf_frame_ssim* out);
int hf_frame_ssim(hf_ctx* ctx, const void* device_a, const void* device_b, int stride_a, int stride_b, int planar, int peak,
                  struct hf_frame_ssim* out);

/* ---- Per-tile SSIM maps on the device: WHERE a frame is torn ----
 * hf_frame_ssim's max_loss_q32 is the score of a plane's worst window, not its position, and the error maps above hold only squared
 * and absolute error, which a ghost passes and a sharp, slightly misplaced edge fails.  This keeps the windowed SSIM per tile of the
 * error maps' grid, so that the two maps join entry by entry.  Pairs, strides, layouts, planes, compared columns, the peak rule, the
 * constants, the window terms and the window loss are those of hf_frame_ssim_enqueue, steps 1 to 5, unchanged; step by step:
 *   1. Tiles.  `tile`, tw and th are those of hf_frame_error_map_shape: 16, 32 or 64 luma pixels (HF_ERROR_MAP_TILES_OK),
 *      tw = (frame_width + tile - 1) / tile, th = (frame_height + tile - 1) / tile.  The tile edge in a plane's own elements is
 *      te = tile for Y and tile / 2 for U and V (always a multiple of 4): tile (i, j) is the picture area of the error map's tile (i, j).
 *   2. Which tile owns a window.  Window (i, j) of a plane covers elements 4 i .. 4 i + 7 by 4 j .. 4 j + 7 and belongs to the ONE tile
 *      that holds its first element: tile (4 i / te, 4 j / te).  A window whose first block is the last block column or row of a tile
 *      reaches 4 elements into the neighbouring tile and still belongs to the first.
 *   3. Per tile and plane:  sum_loss_q32 = sum of the losses of its windows,  max_loss_q32 = the largest,  count = their number
 *      (a 64 x 64 tile holds 256 windows of at most 2^33 each: sums stay below 2^42).  Mean SSIM of a tile = 1 - sum_loss_q32 / 2^32 /
 *      count.
 *   4. A tile may own no window: in the last column or row where fewer than 8 elements remain past the tile's first element, where the
 *      unused w & 3 / h & 3 remainder cuts the last window, or in a plane without any window.  It is written as zeros, count = 0.
 *   5. One map is `struct hf_ssim_tile [3][th][tw]`, plane 0 Y, 1 U, 2 V: bytes_per_map = 72 tw th.  device_maps is ONE caller-owned
 *      device buffer of n bytes_per_map bytes, 16-byte aligned; the map of pair i starts at byte i bytes_per_map.
 *   6. EVERY entry of every map is written by the launch, zeros included: the caller does not clear the buffer.  Per pair and plane the
 *      sum of sum_loss_q32 over the tiles is hf_frame_ssim's sum_loss_q32, the largest max_loss_q32 its max_loss_q32, the sum of count
 *      its count.  Equal frames give zero losses.
 *   hf_frame_ssim_map_shape    tw, th and bytes_per_map of ctx's geometry for a tile (any of the three results may be NULL).
 *   hf_frame_ssim_map_enqueue  only enqueues, ordered exactly like hf_frame_error_enqueue (behind every warp, copy and update of ctx,
 *                              the warp stream of an HF_FLAG_DUAL_STREAM context included; a batch member on its batch's stream).
 *                              Read the maps with hf_memcpy_d2h after hf_sync.  The frames must stay as they are until it has run.
 *                              The SSIM slots and the error slots are untouched.
 * HF_ERR_INVALID_ARGUMENT with nothing enqueued: everything hf_frame_ssim_enqueue refuses but the slot range (there are no slots), a
 * tile outside {16, 32, 64}, a NULL or misaligned device_maps.  Additive to ABI version 6. */
struct hf_ssim_tile { uint64_t sum_loss_q32; uint64_t max_loss_q32; uint32_t count; uint32_t reserved; };   /* 24 bytes, reserved = 0 */
int hf_frame_ssim_map_shape(const hf_ctx* ctx, int tile, int* tiles_x, int* tiles_y, size_t* bytes_per_map);
int hf_frame_ssim_map_enqueue(hf_ctx* ctx, int n, const void* const* device_a, const void* const* device_b, int stride_a, int stride_b,
                              int planar, int peak, int tile, void* device_maps);

/* ---- Warp disagreement maps on the device: confidence WITHOUT a truth frame ----
 * Every judge above needs a second frame to compare with, so a clip can only be judged leave-one-out.  A blended output, though, is made
 * of two warped halves -- frame N-2 pushed forward by t and frame N-1 pulled back by 1 - t -- and where the flow is right the two show
 * the same picture; where it is wrong (occlusion, a motion boundary, motion beyond the search reach) they differ.  This call measures
 * that difference per tile of the error maps' grid, for up to HF_MAX_DISAGREEMENT_OUTPUTS blending scalars of one source period, in one
 * launch and without writing a frame.  Step by step:
 *   1. Sources.  What hf_warp_frames would read if it were called at the same moment: frames N-2 and N-1 of ctx's ring (always NV12 /
 *      P010, whatever HF_FLAG_PLANAR_IN / HF_FLAG_PLANAR_OUT say) and the previous blurred flow.  No state is checked that
 *      hf_warp_frames does not check.
 *   2. Per t[k] and per element (plane, row, column) of the picture:  a = the value hf_warp_frames(ctx, t[k], HF_MODE_WARPED_FRAME_12)
 *      writes there,  b = the value hf_warp_frames(ctx, t[k], HF_MODE_WARPED_FRAME_21) writes there -- the raw gathered samples of the
 *      two frames, no levels, no blend;  d = |a - b|.
 *   3. Tiles, planes and sums are those of hf_frame_error_map_enqueue, steps 1 to 3: `tile` is 16, 32 or 64, tw and th come from
 *      hf_frame_error_map_shape, the interleaved UV plane is split into U and V, and per tile  sse = sum d^2,  sad = sum d,
 *      max_abs = max d.
 *   4. device_maps is ONE caller-owned device buffer of n_t bytes_per_map bytes, 16-byte aligned, holding
 *      `struct hf_error_tile [n_t][3][th][tw]`; the map of t[k] starts at byte k bytes_per_map.  EVERY entry is written by the launch,
 *      zeros included.
 *   5. The identity that defines it: map k is byte for byte what hf_frame_error_map_enqueue stores for the pair (mode-0 output at t[k],
 *      mode-1 output at t[k]) of this context, with any output stride and planar = 0.
 * The call only enqueues, ordered exactly like hf_frame_error_enqueue (behind every update, chain, warp and copy of ctx, the warp stream
 * of an HF_FLAG_DUAL_STREAM context included; a batch member on its batch's stream).  Straight behind hf_interpolate_period or
 * hf_batch_run_period* it describes the frames and the flow that period's warps used.  The frames of an hf_update_frame_device_ref
 * update must stay as they are until the launch has run.  Nothing observable of ctx changes: not the output frame or its target, not
 * m_warpCalcTime, no profile span, no diagnostic counter, no error or SSIM slot.  Read the maps with hf_memcpy_d2h after hf_sync.
 * HF_ERR_INVALID_ARGUMENT with nothing enqueued: a NULL t, n_t outside [1, HF_MAX_DISAGREEMENT_OUTPUTS], any t[k] > 1 (hf_warp_frames'
 * own rule), a tile outside {16, 32, 64}, a NULL or misaligned device_maps.  Additive to ABI version 6. */
#define HF_MAX_DISAGREEMENT_OUTPUTS 24   /* = HF_MAX_PERIOD_OUTPUTS_WIDE */
int hf_warp_disagreement_map_enqueue(hf_ctx* ctx, int n_t, const float* t, int tile, void* device_maps);

/* ---- Guarded blend: a cross-fade where the warped halves disagree (artifact masking) ----
 * HF_MODE_BLENDED_FRAME mixes the two warped halves everywhere, however far apart they are; where the flow is wrong that is a torn
 * picture.  This call acts on the disagreement maps above: per output it writes the motion-compensated blend where the halves agree and
 * fades into the plain cross-fade of the two source frames -- a soft ghost instead of a tear -- where they do not.  The reference has no
 * counterpart; the definition is this one, in integers.  Step by step:
 *   1. Sources.  Exactly what hf_warp_disagreement_map_enqueue reads at the same moment: frames N-2 and N-1 of ctx's ring and the
 *      previous blurred flow.
 *   2. Maps.  device_maps is caller-owned, n_t bytes_per_map bytes, 16-byte aligned; after the call it holds byte for byte what
 *      hf_warp_disagreement_map_enqueue(ctx, n_t, t, tile, device_maps) stores (that launch runs first), so the confidence comes free.
 *   3. Tile weight, per tile (ty, tx) of the LUMA plane of map k, in 64-bit integers:  cnt = the luma pixels of the tile inside the
 *      frame (edge tiles are partial);  m = (16 sad) / (cnt << (hdr ? 8 : 0)), floor -- the mean absolute difference in sixteenths of an
 *      8-bit code, so one 10-bit code of a P010 frame is 4 units;  wt = 0 if m <= lo_q4,  256 if m >= hi_q4,  else
 *      ((m - lo_q4) 256) / (hi_q4 - lo_q4), floor.  The chroma planes of the map are not consulted.
 *   4. Element weight: the tile weights interpolated bilinearly between the nominal tile centres.  With tile = 1 << lg, for a luma
 *      element (x, y):  u = x - tile / 2,  tx0 = u >> lg (arithmetic shift),  fx = u & (tile - 1),  tx1 = tx0 + 1, both indices clamped
 *      to [0, tw - 1];  v, ty0, fy, ty1 the same way from y;
 *          w = ((tile - fx)(tile - fy) wt00 + fx (tile - fy) wt10 + (tile - fx) fy wt01 + fx fy wt11 + tile tile / 2) >> (2 lg)
 *      (wtXY: column txX, row tyY).  An element (cx, cy) of the interleaved UV plane takes the weight of luma position
 *      (cx & ~1, 2 cy); U and V share it.  0 <= w <= 256.
 *   5. Output.  G = (M (256 - w) + Z w + 128) >> 8, with M the value hf_warp_frames(ctx, t[k], HF_MODE_BLENDED_FRAME) writes at that
 *      element, output levels included, and Z the value the same call writes there when the blurred flow is all zeros: the cross-fade,
 *      with the warp's edge rule as it is.  w = 0 gives M exactly, w = 256 gives Z exactly.
 *   6. device_out[k] is a caller-owned frame of output_frame_bytes, NV12 / P010 at the output stride whatever HF_FLAG_PLANAR_* say.
 *      Every element of columns [0, W) of every row is written; the padding columns are unspecified.
 *   7. The identity that defines it: frame k is the mix of step 5 of the two frames that hf_warp_frames(t[k], 2) writes with the flow as
 *      it is and after hf_write_blurred_flow(ctx, 0, zeros), by the weights of steps 3 and 4 from the map of step 2.
 * Ordering and state are those of hf_warp_disagreement_map_enqueue: the call only enqueues, behind every update, chain, warp and copy of
 * ctx (a batch member on its batch's stream), the next asynchronous upload into frame N-2's slot waits for it, and nothing observable
 * of ctx changes.  (lo_q4, hi_q4) = (4080, 4081) is GUARD OFF: m never exceeds 4080 in SDR, and reaches 4081 in HDR only where the mean
 * difference of a tile is at least 65296 of 65535 codes (black against white).  No thresholds are recommended: measure them on your material (quality.py --guard).
 * HF_ERR_INVALID_ARGUMENT with nothing enqueued and no byte of device_maps or of any device_out[k] written: everything
 * hf_warp_disagreement_map_enqueue refuses, a NULL device_out or device_out[k], thresholds outside 0 <= lo_q4 < hi_q4 <= 65535.
 * Additive to ABI version 6. */
int hf_guarded_blend_enqueue(hf_ctx* ctx, int n_t, const float* t, int tile, int lo_q4, int hi_q4,
                             void* device_maps, void* const* device_out);

/* Device-to-device copy of the output frame into caller-owned device memory. */
int hf_download_frame_device(hf_ctx* ctx, void* device_out);
/* Redirect warp/copy output into caller-owned device memory (NULL restores the internal buffer).  HF_FLAG_PLANAR_OUT: the kernels
 * write semi-planar frames, so a non-NULL buffer returns HF_ERR_STATE (use hf_download_frame_device). */
int hf_set_output_buffer(hf_ctx* ctx, void* device_out);
/* Block until everything enqueued on ctx's stream has finished; finalises timings/total_frame_delta. */
int hf_sync(hf_ctx* ctx);

/* ---- parity / debugging taps on the reference's device buffers ---- */
/* m_offsetArray: int16 [2][low_h][low_w] (raw flow of the last calc) */
int hf_read_offsets(hf_ctx* ctx, int16_t* host_out);
/* m_blurredOffsetArray[idx]: idx 0 = flow consumed by warpFrames, 1 = newest (opticalFlowCalcSDR.cpp:121-123) */
int hf_read_blurred_flow(hf_ctx* ctx, int idx, int16_t* host_out);
int hf_write_blurred_flow(hf_ctx* ctx, int idx, const int16_t* host_in);
/* This build's phase plane of ring frame ring_slot (0 = N-2, 1 = N-1, 2 = N; hf_stats.phase_plane_bytes bytes; the re-laid top-8-bit
 * copy of a frame that replaces the strided sampling of calcDeltaSumsKernelSDR.h:78-100).  *complete = 0: the
 * plane holds only its grid samples so far (deferred build, hf_batch_run_period). */
int hf_read_phase_plane(hf_ctx* ctx, int ring_slot, void* host_out, int* complete);

/* Per-kernel device time accumulated since the last hf_reset_profile() (needs HF_FLAG_PROFILE). */
typedef struct hf_profile {
    uint64_t warp_launches;   /* warp_kernel launches (one per warpFrames: both planes) */
    double warp_ms;           /* summed device time of those launches */
    uint64_t copy_launches;
    double copy_ms;
    uint64_t flow_chains;     /* calculateOpticalFlow chains (16 steps + blur) */
    double flow_ms;           /* summed device time first kernel start -> blur end */
    uint64_t warp_frames;     /* output frames produced by the counted warp launches (hf_interpolate_period fuses a period) */
} hf_profile;
int hf_get_profile(hf_ctx* ctx, hf_profile* out); /* synchronises ctx */
/* Bracket only every n-th warp/copy launch and every m-th flow chain (default 1/1): event records perturb
 * back-to-back launches, so throughput runs sample instead of bracketing everything. */
int hf_set_profile_interval(hf_ctx* ctx, int warp_every, int flow_every);
int hf_reset_profile(hf_ctx* ctx);

/* ---- caller protocol: what the reference's filter does AROUND the calculator (HopperRender.cpp:938-1197,1438-1463) ----
 * Host logic only (no GPU work of its own): how many output frames a source period gets and at which blending scalars,
 * the scene-change decision on the m_totalFrameDelta stream (warp vs copy -- it decides output pixels), the search-radius
 * governor.  A C++ host that keeps the reference's own filter code does not need these; tests/cpp/replay_filter.cpp,
 * the Python mirror (hopperrender_amd/protocol.py) and any cgo / JNI host do.  Times are 100-ns units (REFERENCE_TIME). */
typedef struct hf_filter hf_filter;
typedef struct hf_filter_config {
    uint32_t struct_size;
    int32_t scene_change_threshold;  /* m_iSceneChangeThreshold; < 0 -> DEFAULT_SCENE_CHANGE_THRESHOLD 200 (config.h:27) */
    int64_t source_frame_time;       /* m_rtSourceFrameTime, <= 0 -> 417083 = 23.976 fps (HopperRender.cpp:162) */
    int64_t target_frame_time;       /* m_rtTargetFrameTime, <= 0 -> 166667 = 60 fps (:163) */
    int32_t frame_output_mode;       /* m_iFrameOutput (hf_output_mode), BlendedFrame = 2 */
    int32_t auto_adjust;             /* run the governor in hf_filter_deliver (AUTO_SEARCH_RADIUS_ADJUST, config.h:12) */
    int32_t active;                  /* interpolation requested (m_iIntActiveState != Deactivated) */
    int32_t reserved;
} hf_filter_config;
typedef struct hf_filter_state {
    int32_t num_int_frames;          /* m_iNumIntFrames of the current source period */
    int32_t active;                  /* m_iIntActiveState == Active */
    double blending_scalar;          /* m_dBlendingScalar */
    double total_warp_duration;      /* m_dTotalWarpDuration, seconds */
    int64_t playback_frame_time;     /* m_rtCurrPlaybackFrameTime */
    uint32_t peak_scene_change_delta, peak_scene_change_delta2;  /* m_iPeakSceneChangeDelta{,2} (1-second window) */
    uint32_t frame_delta_history, scene_change_history;          /* entries in the two sliding windows */
    int32_t average_frame_delta, scene_change_delta1, scene_change_delta2;  /* of the last decision (:1139-1144) */
} hf_filter_state;
int hf_filter_create(const hf_filter_config* cfg, hf_filter** out_filter);
void hf_filter_destroy(hf_filter* filter);
int hf_filter_new_segment(hf_filter* filter, double rate);                       /* NewSegment (:834-845); the caller zeroes m_frameCount (:840) */
int hf_filter_set_playback_frame_time(hf_filter* filter, int64_t playback_frame_time);
int hf_filter_is_active(const hf_filter* filter);
int hf_filter_begin_source_frame(hf_filter* filter);                            /* :944-948, returns m_iNumIntFrames */
double hf_filter_blending_scalar(const hf_filter* filter);                      /* m_dBlendingScalar */
void hf_filter_advance_blending_scalar(hf_filter* filter);                      /* :1192-1197 */
void hf_filter_add_warp_duration(hf_filter* filter, double warp_calc_time);     /* :1189 */
int hf_filter_auto_adjust(hf_filter* filter, double ofc_calc_time, int32_t* search_radius); /* :1438-1463; returns -1/0/+1 */
int hf_filter_push_frame_delta(hf_filter* filter, uint32_t frame_count, uint32_t total_frame_delta);   /* :959-972 */
int hf_filter_detect_scene_change(hf_filter* filter, uint32_t frame_count);     /* :1126-1176; 1 = copyFrame instead of warpFrames */
int hf_filter_get_state(const hf_filter* filter, hf_filter_state* out);
/* One DeliverToRenderer (:938-1197) on a blocking context: host_out[i] receives output frame i (n = return of
 * hf_filter_begin_source_frame <= max_out), kinds[i] (optional) = 1 warp / 0 copy.  The number of outputs is unbounded in
 * principle (a slowed-down segment): call hf_filter_begin_source_frame() first to size host_out -- it only recomputes
 * m_iNumIntFrames from the state -- or retry after HF_ERR_INVALID_ARGUMENT with the *n_out buffers it then reports (nothing else
 * has been touched at that point). */
int hf_filter_deliver(hf_filter* filter, hf_ctx* ctx, const void* host_in, void* const* host_out, int max_out, int* n_out, int32_t* kinds);

/* ---- Streaming host-I/O driver of one rank + timeline planner (multi-GPU hosts; csrc/hf_hostio.cpp, plain host C++) --------
 * The reference's filter feeds the calculator from host memory with blocking transfers (opticalFlowCalcSDR.cpp:19-42) on one
 * GPU.  A throughput host converts one clip on several GPUs: rank r (= process = GPU) owns a contiguous chunk of the source
 * timeline (hf_shard_timeline: no exchange between ranks -- the warm-up frames in front of a chunk rebuild ring, previous flow
 * and scene-change history), and hf_hostio_run() streams it: pinned input ring -> hf_update_frame_async -> chain / warps ->
 * hf_download_frame_async -> pinned output ring -> sink(), output frames strictly in index order, the filter's warp-vs-copy
 * decision (hf_filter) made per period from that period's m_totalFrameDelta (one hf_wait_flow per period).  `fill` and `sink`
 * run on the calling thread; the buffers they are handed are page-locked and only valid during the call. */
typedef struct hf_timeline_chunk {
    int64_t first_period, n_periods;   /* source periods (= source frames) this rank interpolates */
    int64_t first_frame, n_frames;     /* source frames it has to be fed: the warm-up frames + its own */
    int64_t first_output, n_outputs;   /* global index of its first output frame, number of its output frames */
    double blend_at_start;             /* m_dBlendingScalar when its first period begins */
} hf_timeline_chunk;
/* n_out (optional): [n_periods] outputs per owned period; t (optional): their blending scalars, t_capacity entries at least
 * n_outputs (call once with n_out = t = NULL to learn the sizes).  overlap = 3 and delta_history = 12 reproduce the sequential
 * filter (delta_history 0: scene-change detection off). */
int hf_shard_timeline(int64_t n_source_frames, int world, int rank, int64_t source_frame_time, int64_t target_frame_time, int overlap,
                      int delta_history, hf_timeline_chunk* out, int32_t* n_out, float* t, int64_t t_capacity);
typedef struct hf_hostio hf_hostio;
typedef struct hf_hostio_config {
    uint32_t struct_size;
    int32_t in_ring, out_ring;          /* page-locked input / output frame buffers; <= 0 -> 3 / 12 (>= 3 / >= 2) */
    int32_t frame_output_mode;          /* m_iFrameOutput, BlendedFrame = 2 */
    int32_t scene_change_threshold;     /* < 0 -> DEFAULT_SCENE_CHANGE_THRESHOLD */
    int32_t reserved;
    int64_t source_frame_time, target_frame_time;   /* 100-ns units; <= 0 -> 417083 / 166667 */
} hf_hostio_config;
typedef int (*hf_hostio_fill_fn)(void* user, int64_t source_frame_index, void* pinned_frame);              /* 0 = ok */
typedef int (*hf_hostio_sink_fn)(void* user, int64_t output_index_in_chunk, const void* frame, int32_t kind);   /* kind: 1 warp, 0 copy */
/* ctx: an HF_FLAG_ASYNC (| HF_FLAG_DUAL_STREAM) context that the driver uses exclusively while it exists.
 * cfg == NULL: the filter's defaults -- rings 3 / 12, BlendedFrame output, DEFAULT_SCENE_CHANGE_THRESHOLD, 23.976 -> 60 fps.  (In a
 * caller-supplied struct a scene_change_threshold of 0 means what it says: every non-zero frame delta is a scene change.) */
int hf_hostio_create(hf_ctx* ctx, const hf_hostio_config* cfg, hf_hostio** out);
void hf_hostio_destroy(hf_hostio* io);
/* kinds (optional): [chunk->n_outputs] 1 warp / 0 copy per output frame. */
int hf_hostio_run(hf_hostio* io, const hf_timeline_chunk* chunk, const int32_t* n_out, const float* t, hf_hostio_fill_fn fill,
                  hf_hostio_sink_fn sink, void* user, int32_t* kinds);
int hf_hostio_get_traffic(const hf_hostio* io, uint64_t* bytes_in, uint64_t* bytes_out);   /* host -> device / device -> host so far */
const char* hf_hostio_last_error(const hf_hostio* io);   /* io == NULL: last failed hf_hostio_create / hf_shard_timeline of this thread */

/* ---- plain device-memory helpers so non-HIP hosts (ctypes, cgo, JNI) can stage frames ---- */
int hf_device_count(void);
int hf_device_malloc(int device_index, size_t bytes, void** out_dev_ptr);
int hf_device_free(int device_index, void* dev_ptr);
int hf_memcpy_h2d(int device_index, void* dev_dst, const void* host_src, size_t bytes);
int hf_memcpy_d2h(int device_index, void* host_dst, const void* dev_src, size_t bytes);
/* Page-locked host memory for frame buffers handed to hf_update_frame / hf_download_frame (full PCIe rate). */
int hf_host_malloc_pinned(size_t bytes, void** out_host_ptr);
int hf_host_free_pinned(void* host_ptr);

#ifdef __cplusplus
}
#endif
#endif /* HOPPERFLOW_H */
