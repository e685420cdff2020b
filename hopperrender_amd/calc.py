"""Python mirror of the reference's OpticalFlowCalc interface (reference HopperRender/
opticalFlowCalc.h:24-138, opticalFlowCalcSDR.h:10-56, opticalFlowCalcHDR.h:10-56) on the C ABI.

Same constructor arguments, same method names (updateFrame / downloadFrame / calculateOpticalFlow /
warpFrames / copyFrame) and the same public field names (m_*), so tests read like calls made by the
reference's filter (HopperRender.cpp:907-1189).  `init` and `blendFrames` are the aliases
BASELINE.json's north_star uses for the constructor body and warpFrames(t, 2).
Errors surface as HopperFlowError (reference: std::runtime_error).
"""
import ctypes as C

import numpy as np

from . import capi

BlendedFrame = 2  # HopperRender.h:10-18
WarpedFrame12, WarpedFrame21, HSVFlow, GreyFlow, SideBySide1, SideBySide2 = 0, 1, 3, 4, 5, 6


def _ptr(a):
    if isinstance(a, np.ndarray):
        if not a.flags["C_CONTIGUOUS"]:
            raise ValueError("frame buffers must be C-contiguous")
        return a.ctypes.data_as(C.c_void_p)
    return C.c_void_p(a)


class OpticalFlowCalc:
    """Abstract base in the reference; here the shared implementation (is_hdr set by subclasses)."""

    is_hdr = False

    def __init__(self, frameHeight, frameWidth, inputStride=0, outputStride=0, deltaScalar=8, neighborScalar=6,
                 blackLevel=0.0, whiteLevel=255.0, maxCalcRes=270, *, device_index=0, iterations=0, blur_radius=0,
                 search_radius=0, flags=0):
        self._lib = capi.load()
        self._ctx = C.c_void_p()
        self.init(frameHeight, frameWidth, inputStride, outputStride, deltaScalar, neighborScalar, blackLevel,
                  whiteLevel, maxCalcRes, device_index=device_index, iterations=iterations, blur_radius=blur_radius,
                  search_radius=search_radius, flags=flags)

    def init(self, frameHeight, frameWidth, inputStride, outputStride, deltaScalar, neighborScalar, blackLevel,
             whiteLevel, maxCalcRes, *, device_index=0, iterations=0, blur_radius=0, search_radius=0, flags=0):
        """Constructor body (opticalFlowCalcSDR.cpp:206-325)."""
        if self._ctx:
            self._lib.hf_destroy(self._ctx)
            self._ctx = C.c_void_p()
        cfg = capi.HfConfig(C.sizeof(capi.HfConfig), int(self.is_hdr), frameHeight, frameWidth, inputStride, outputStride,
                            deltaScalar, neighborScalar, blackLevel, whiteLevel, maxCalcRes, device_index, iterations,
                            blur_radius, search_radius, flags)
        capi.check(self._lib.hf_create(C.byref(cfg), C.byref(self._ctx)))
        self.device_index = self._lib.hf_get_device(self._ctx)   # device_index = -1: the first suitable device
        capi._devices_used.add(self.device_index)
        st = self._stats()
        self.m_frameWidth, self.m_frameHeight = st.frame_width, st.frame_height
        self.m_inputStride, self.m_outputStride = st.input_stride, st.output_stride
        self.m_opticalFlowResScalar = st.res_scalar
        self.m_opticalFlowFrameWidth, self.m_opticalFlowFrameHeight = st.low_width, st.low_height
        self.input_frame_bytes, self.output_frame_bytes = st.input_frame_bytes, st.output_frame_bytes
        self.phase_plane_bytes = st.phase_plane_bytes
        self.dtype = np.uint16 if self.is_hdr else np.uint8

    # ---- public fields of the reference object, backed by the context ----
    def _params(self):
        p = capi.HfParams()
        capi.check(self._lib.hf_get_params(self._ctx, C.byref(p)), self._ctx)
        return p

    def _set(self, **kw):
        p = self._params()
        for k, v in kw.items():
            setattr(p, k, v)
        capi.check(self._lib.hf_set_params(self._ctx, C.byref(p)), self._ctx)

    def _stats(self):
        s = capi.HfStats()
        capi.check(self._lib.hf_get_stats(self._ctx, C.byref(s)), self._ctx)
        return s

    m_deltaScalar = property(lambda s: s._params().delta_scalar, lambda s, v: s._set(delta_scalar=int(v)))
    m_neighborBiasScalar = property(lambda s: s._params().neighbor_scalar, lambda s, v: s._set(neighbor_scalar=int(v)))
    m_outputBlackLevel = property(lambda s: s._params().black_level, lambda s, v: s._set(black_level=float(v)))
    m_outputWhiteLevel = property(lambda s: s._params().white_level, lambda s, v: s._set(white_level=float(v)))
    m_opticalFlowSearchRadius = property(lambda s: s._params().search_radius, lambda s, v: s._set(search_radius=int(v)))
    m_frameCount = property(lambda s: s._params().frame_count, lambda s, v: s._set(frame_count=int(v)))
    m_totalFrameDelta = property(lambda s: s._stats().total_frame_delta)
    m_ofcCalcTime = property(lambda s: s._stats().ofc_calc_time)
    m_ofcAvgCalcTime = property(lambda s: s._stats().ofc_avg_calc_time)
    m_ofcPeakCalcTime = property(lambda s: s._stats().ofc_peak_calc_time)
    m_warpCalcTime = property(lambda s: s._stats().warp_calc_time)

    # ---- the five virtuals ----
    def updateFrame(self, inputPlanes):
        """opticalFlowCalcSDR.cpp:19-29.  inputPlanes: host ndarray (NV12 uint8 / P010 uint16)."""
        a = np.ascontiguousarray(inputPlanes)
        if a.nbytes < self.input_frame_bytes:
            raise ValueError(f"input frame has {a.nbytes} bytes, need {self.input_frame_bytes}")
        capi.check(self._lib.hf_update_frame(self._ctx, _ptr(a)), self._ctx)

    def downloadFrame(self, outputPlanes=None):
        """opticalFlowCalcSDR.cpp:31-42.  Returns the flat output frame (allocated if not given)."""
        if outputPlanes is None:
            outputPlanes = np.empty(self.output_frame_bytes // np.dtype(self.dtype).itemsize, dtype=self.dtype)
        if outputPlanes.nbytes < self.output_frame_bytes:
            raise ValueError("output buffer too small")
        capi.check(self._lib.hf_download_frame(self._ctx, _ptr(outputPlanes)), self._ctx)
        return outputPlanes

    def calculateOpticalFlow(self):
        """opticalFlowCalcSDR.cpp:44-139."""
        capi.check(self._lib.hf_calculate_optical_flow(self._ctx), self._ctx)

    def warpFrames(self, blendingScalar, frameOutputMode):
        """opticalFlowCalcSDR.cpp:141-168."""
        capi.check(self._lib.hf_warp_frames(self._ctx, float(blendingScalar), int(frameOutputMode)), self._ctx)

    def blendFrames(self, blendingScalar):
        self.warpFrames(blendingScalar, BlendedFrame)

    def copyFrame(self):
        """opticalFlowCalcSDR.cpp:170-183."""
        capi.check(self._lib.hf_copy_frame(self._ctx), self._ctx)

    # ---- device-resident / async extensions ----
    def updateFrameDevice(self, dev_ptr):
        capi.check(self._lib.hf_update_frame_device(self._ctx, C.c_void_p(dev_ptr)), self._ctx)

    def updateFrameDeviceRef(self, dev_ptr):
        """Zero-copy: the ring references the caller's device frame (valid until 3 more updates)."""
        capi.check(self._lib.hf_update_frame_device_ref(self._ctx, C.c_void_p(dev_ptr)), self._ctx)

    def interpolatePeriod(self, dev_frame_ptr, scalars, out_ptrs, mode=BlendedFrame):
        """updateFrame(ref) + calculateOpticalFlow + one warpFrames per scalar, in ONE native call."""
        n = len(scalars)
        ts = (C.c_float * n)(*[float(x) for x in scalars])
        outs = (C.c_void_p * n)(*[int(p) for p in out_ptrs[:n]])
        capi.check(self._lib.hf_interpolate_period(self._ctx, C.c_void_p(dev_frame_ptr or 0), n, ts, outs, int(mode)), self._ctx)

    def interpolateOnly(self, scalars, out_ptrs, mode=BlendedFrame):
        """The warps of one period (one fused launch when eligible), without updateFrame / calculateOpticalFlow."""
        n = len(scalars)
        ts = (C.c_float * n)(*[float(x) for x in scalars])
        outs = (C.c_void_p * n)(*[int(p) for p in out_ptrs[:n]])
        capi.check(self._lib.hf_interpolate_period_ex(self._ctx, None, n, ts, outs, int(mode), 0), self._ctx)

    def updateFrameAsync(self, pinned):
        """H2D on a side stream; `pinned` = PinnedArray (or its .array) that stays valid until sync()."""
        a = pinned.array if hasattr(pinned, "array") else pinned
        capi.check(self._lib.hf_update_frame_async(self._ctx, _ptr(a)), self._ctx)

    def downloadFrameAsync(self, pinned):
        """D2H of the frame just produced on a side stream; read `pinned` only after sync()."""
        a = pinned.array if hasattr(pinned, "array") else pinned
        capi.check(self._lib.hf_download_frame_async(self._ctx, _ptr(a)), self._ctx)

    def waitFlow(self):
        """Asynchronous contexts: block until the last calculateOpticalFlow has finished (m_totalFrameDelta valid); side streams keep running."""
        capi.check(self._lib.hf_wait_flow(self._ctx), self._ctx)

    def downloadsIssued(self):
        return int(self._lib.hf_downloads_issued(self._ctx))

    def waitDownload(self, index):
        """Block until the index-th downloadFrameAsync (issue order, from 0) has landed in its host buffer."""
        capi.check(self._lib.hf_wait_download(self._ctx, int(index)), self._ctx)

    def downloadFrameDevice(self, dev_ptr):
        capi.check(self._lib.hf_download_frame_device(self._ctx, C.c_void_p(dev_ptr)), self._ctx)

    # ---- frame error sums on the device (hf_frame_error*) ----
    def _pair_args(self, who, a_ptrs, b_ptrs, stride_a, stride_b, planar):
        """(n, a table, b table, stride_a, stride_b, planar) as ctypes arguments of the four enqueue calls below; strides 0 = the frame width"""
        n = len(a_ptrs)
        if len(b_ptrs) != n:
            raise ValueError(who + ": as many b frames as a frames")
        a = (C.c_void_p * max(n, 1))(*[int(p) if p else None for p in a_ptrs])
        b = (C.c_void_p * max(n, 1))(*[int(p) if p else None for p in b_ptrs])
        return n, a, b, int(stride_a) or self.m_frameWidth, int(stride_b) or self.m_frameWidth, 1 if planar else 0

    @staticmethod
    def _frame_error_dict(e):
        """struct hf_frame_error as {'Y': {...}, 'U': {...}, 'V': {...}} of plain ints: sse, sad, max_abs, n_differ, count"""
        return {p: {k: int(getattr(e, k)[i]) for k in ("sse", "sad", "max_abs", "n_differ", "count")} for i, p in enumerate("YUV")}

    def frameErrorEnqueue(self, a_ptrs, b_ptrs, first_slot=0, stride_a=0, stride_b=0, planar=False):
        """hf_frame_error_enqueue: compare device frames a_ptrs[i] and b_ptrs[i] into result slot first_slot + i, behind everything this
        context has enqueued; only enqueues.  Strides in elements, 0 = the frame width."""
        args = self._pair_args("frameErrorEnqueue", a_ptrs, b_ptrs, stride_a, stride_b, planar)
        capi.check(self._lib.hf_frame_error_enqueue(self._ctx, *args, int(first_slot)), self._ctx)

    def frameErrorRead(self, first_slot, n):
        """hf_frame_error_read: wait for this context's work and return result slots [first_slot, first_slot + n) as dicts."""
        out = (capi.HfFrameError * max(int(n), 1))()
        capi.check(self._lib.hf_frame_error_read(self._ctx, int(first_slot), int(n), out), self._ctx)
        return [self._frame_error_dict(e) for e in out[:n]]

    def frameError(self, a_ptr, b_ptr, stride_a=0, stride_b=0, planar=False):
        """hf_frame_error: one pair, blocking."""
        e = capi.HfFrameError()
        capi.check(self._lib.hf_frame_error(self._ctx, C.c_void_p(a_ptr or 0), C.c_void_p(b_ptr or 0), int(stride_a) or self.m_frameWidth,
                                            int(stride_b) or self.m_frameWidth, 1 if planar else 0, C.byref(e)), self._ctx)
        return self._frame_error_dict(e)

    # ---- per-tile error maps on the device (hf_frame_error_map*) ----
    def frameErrorMapShape(self, tile):
        """hf_frame_error_map_shape: (tiles_x, tiles_y, bytes of one map) of this context's geometry for tiles of `tile` luma pixels."""
        tw, th, nbytes = C.c_int(), C.c_int(), C.c_size_t()
        capi.check(self._lib.hf_frame_error_map_shape(self._ctx, int(tile), C.byref(tw), C.byref(th), C.byref(nbytes)), self._ctx)
        return tw.value, th.value, nbytes.value

    def frameErrorMapEnqueue(self, a_ptrs, b_ptrs, tile, maps_ptr, stride_a=0, stride_b=0, planar=False):
        """hf_frame_error_map_enqueue: the per-tile error sums of device frames a_ptrs[i] against b_ptrs[i] into map i of the device buffer
        at maps_ptr (len(a_ptrs) maps of frameErrorMapShape(tile)[2] bytes, 16-byte aligned), behind everything this context has
        enqueued; only enqueues.  Download the buffer after sync() and view it with frame_error_maps()."""
        args = self._pair_args("frameErrorMapEnqueue", a_ptrs, b_ptrs, stride_a, stride_b, planar)
        capi.check(self._lib.hf_frame_error_map_enqueue(self._ctx, *args, int(tile), C.c_void_p(maps_ptr or 0)), self._ctx)

    # ---- warp disagreement maps on the device (hf_warp_disagreement_map_enqueue) ----
    def warpDisagreementMapEnqueue(self, ts, tile, maps_ptr):
        """hf_warp_disagreement_map_enqueue: for every blending scalar of ts, per tile, how far the two warped halves of an output are
        apart (what warpFrames(t, 0) and warpFrames(t, 1) would write, compared like frameErrorMapEnqueue) into map k of the device buffer
        at maps_ptr (len(ts) maps of frameErrorMapShape(tile)[2] bytes, 16-byte aligned), behind everything this context has enqueued; one
        launch, no frame written, only enqueues.  Download the buffer after sync() and view it with frame_error_maps()."""
        n = len(ts)
        t = (C.c_float * max(n, 1))(*[float(x) for x in ts])
        capi.check(self._lib.hf_warp_disagreement_map_enqueue(self._ctx, n, t, int(tile), C.c_void_p(maps_ptr or 0)), self._ctx)

    # ---- guarded blend on the device (hf_guarded_blend_enqueue) ----
    def guardedBlendEnqueue(self, ts, tile, lo_q4, hi_q4, maps_ptr, out_ptrs):
        """hf_guarded_blend_enqueue: for every blending scalar of ts the blended frame of warpFrames(t, 2), faded into the plain cross-fade
        of the two source frames where the warped halves disagree, into the device frame out_ptrs[k] (output_frame_bytes each, NV12 / P010
        at the output stride); map k of the buffer at maps_ptr receives what warpDisagreementMapEnqueue(ts, tile, maps_ptr) stores.  A
        tile's mean luma difference in sixteenths of an 8-bit code up to lo_q4 keeps the blend, from hi_q4 on it is all cross-fade;
        (4080, 4081) is guard off.  Behind everything this context has enqueued; only enqueues.  guard_weights() shows the mask."""
        n = len(ts)
        if len(out_ptrs) != n:
            raise ValueError(f"guardedBlendEnqueue: {n} blending scalars, {len(out_ptrs)} output frames")
        t = (C.c_float * max(n, 1))(*[float(x) for x in ts])
        outs = (C.c_void_p * max(n, 1))(*[C.c_void_p(p or 0) for p in out_ptrs])
        capi.check(self._lib.hf_guarded_blend_enqueue(self._ctx, n, t, int(tile), int(lo_q4), int(hi_q4), C.c_void_p(maps_ptr or 0), outs), self._ctx)

    # ---- windowed SSIM on the device (hf_frame_ssim*) ----
    @staticmethod
    def _frame_ssim_dict(e):
        """struct hf_frame_ssim as {'Y': {...}, 'U': {...}, 'V': {...}}: the plain ints sum_loss_q32, max_loss_q32, count and the floats
        ssim = 1 - sum_loss_q32 / 2^32 / count (mean) and min_ssim = 1 - max_loss_q32 / 2^32 (worst window); None where count == 0"""
        out = {}
        for i, p in enumerate("YUV"):
            s, m, n = int(e.sum_loss_q32[i]), int(e.max_loss_q32[i]), int(e.count[i])
            out[p] = {"sum_loss_q32": s, "max_loss_q32": m, "count": n, "ssim": 1.0 - s / 4294967296.0 / n if n else None,
                      "min_ssim": 1.0 - m / 4294967296.0 if n else None}
        return out

    def frameSsimEnqueue(self, a_ptrs, b_ptrs, first_slot=0, stride_a=0, stride_b=0, planar=False, peak=0):
        """hf_frame_ssim_enqueue: score device frames a_ptrs[i] against b_ptrs[i] into SSIM slot first_slot + i, behind everything this
        context has enqueued; only enqueues.  Strides in elements, 0 = the frame width; peak 0 = the format's own."""
        args = self._pair_args("frameSsimEnqueue", a_ptrs, b_ptrs, stride_a, stride_b, planar)
        capi.check(self._lib.hf_frame_ssim_enqueue(self._ctx, *args, int(peak), int(first_slot)), self._ctx)

    def frameSsimRead(self, first_slot, n):
        """hf_frame_ssim_read: wait for this context's work and return SSIM slots [first_slot, first_slot + n) as dicts."""
        out = (capi.HfFrameSsim * max(int(n), 1))()
        capi.check(self._lib.hf_frame_ssim_read(self._ctx, int(first_slot), int(n), out), self._ctx)
        return [self._frame_ssim_dict(e) for e in out[:n]]

    def frameSsim(self, a_ptr, b_ptr, stride_a=0, stride_b=0, planar=False, peak=0):
        """hf_frame_ssim: one pair, blocking."""
        e = capi.HfFrameSsim()
        capi.check(self._lib.hf_frame_ssim(self._ctx, C.c_void_p(a_ptr or 0), C.c_void_p(b_ptr or 0), int(stride_a) or self.m_frameWidth,
                                           int(stride_b) or self.m_frameWidth, 1 if planar else 0, int(peak), C.byref(e)), self._ctx)
        return self._frame_ssim_dict(e)

    # ---- per-tile SSIM maps on the device (hf_frame_ssim_map*) ----
    def frameSsimMapShape(self, tile):
        """hf_frame_ssim_map_shape: (tiles_x, tiles_y, bytes of one map) of this context's geometry for tiles of `tile` luma pixels: the
        tile grid of frameErrorMapShape, 72 bytes a tile."""
        tw, th, nbytes = C.c_int(), C.c_int(), C.c_size_t()
        capi.check(self._lib.hf_frame_ssim_map_shape(self._ctx, int(tile), C.byref(tw), C.byref(th), C.byref(nbytes)), self._ctx)
        return tw.value, th.value, nbytes.value

    def frameSsimMapEnqueue(self, a_ptrs, b_ptrs, tile, maps_ptr, stride_a=0, stride_b=0, planar=False, peak=0):
        """hf_frame_ssim_map_enqueue: the windowed SSIM of device frames a_ptrs[i] against b_ptrs[i] per tile into map i of the device
        buffer at maps_ptr (len(a_ptrs) maps of frameSsimMapShape(tile)[2] bytes, 16-byte aligned), behind everything this context has
        enqueued; only enqueues.  Download the buffer after sync() and view it with frame_ssim_maps()."""
        args = self._pair_args("frameSsimMapEnqueue", a_ptrs, b_ptrs, stride_a, stride_b, planar)
        capi.check(self._lib.hf_frame_ssim_map_enqueue(self._ctx, *args, int(peak), int(tile), C.c_void_p(maps_ptr or 0)), self._ctx)

    def setOutputBuffer(self, dev_ptr):
        capi.check(self._lib.hf_set_output_buffer(self._ctx, C.c_void_p(dev_ptr or 0)), self._ctx)

    def sync(self):
        capi.check(self._lib.hf_sync(self._ctx), self._ctx)

    def timerBegin(self):
        capi.check(self._lib.hf_timer_begin(self._ctx), self._ctx)

    def timerEnd(self):
        ms = C.c_float()
        capi.check(self._lib.hf_timer_end(self._ctx, C.byref(ms)), self._ctx)
        return ms.value

    def profile(self):
        """Device-time totals since resetProfile() (needs flags=HF_FLAG_PROFILE)."""
        pr = capi.HfProfile()
        capi.check(self._lib.hf_get_profile(self._ctx, C.byref(pr)), self._ctx)
        return {k: getattr(pr, k) for k, _ in pr._fields_}

    def setProfileInterval(self, warp_every, flow_every):
        capi.check(self._lib.hf_set_profile_interval(self._ctx, int(warp_every), int(flow_every)), self._ctx)

    def resetProfile(self):
        capi.check(self._lib.hf_reset_profile(self._ctx), self._ctx)

    # ---- parity taps ----
    def readOffsets(self):
        a = np.empty((2, self.m_opticalFlowFrameHeight, self.m_opticalFlowFrameWidth), dtype=np.int16)
        capi.check(self._lib.hf_read_offsets(self._ctx, _ptr(a)), self._ctx)
        return a

    def readBlurredFlow(self, idx):
        a = np.empty((2, self.m_opticalFlowFrameHeight, self.m_opticalFlowFrameWidth), dtype=np.int16)
        capi.check(self._lib.hf_read_blurred_flow(self._ctx, idx, _ptr(a)), self._ctx)
        return a

    def readPhasePlane(self, ring_slot):
        """(plane as uint32 words, complete?) -- hf_read_phase_plane"""
        import ctypes
        n = int(self.phase_plane_bytes)
        a = np.empty(n // 4, dtype=np.uint32)
        done = ctypes.c_int(0)
        capi.check(self._lib.hf_read_phase_plane(self._ctx, ring_slot, _ptr(a), ctypes.byref(done)), self._ctx)
        return a, bool(done.value)

    def writeBlurredFlow(self, idx, flow):
        a = np.ascontiguousarray(flow, dtype=np.int16)
        assert a.shape == (2, self.m_opticalFlowFrameHeight, self.m_opticalFlowFrameWidth)
        capi.check(self._lib.hf_write_blurred_flow(self._ctx, idx, _ptr(a)), self._ctx)

    def deviceRcp(self, values):
        x = np.ascontiguousarray(values, dtype=np.float32)
        y = np.empty_like(x)
        capi.check(self._lib.hf_device_rcp(self._ctx, _ptr(x), _ptr(y), len(x)), self._ctx)
        return y

    def countersEnable(self, on=True):
        """hopperflow_diag.h hf_debug_counters_enable: device-side counters of the kernels' per-window / per-workgroup decisions."""
        capi.check(self._lib.hf_debug_counters_enable(self._ctx, 1 if on else 0), self._ctx)

    def counters(self, reset=False):
        """{'warp_workgroups': {staged, interior_global, generic}, 'levels': {window: {'X': (windows, reused), 'Y': ...}}}"""
        cc = capi.HfDebugCounters()
        capi.check(self._lib.hf_debug_counters_read(self._ctx, C.byref(cc), 1 if reset else 0), self._ctx)
        lv = {}
        for k in range(16):
            if cc.level_window_size[k] and (cc.level_windows[k][0] or cc.level_windows[k][1]):
                lv[int(cc.level_window_size[k])] = {"X": (int(cc.level_windows[k][0]), int(cc.level_reused[k][0])),
                                                     "Y": (int(cc.level_windows[k][1]), int(cc.level_reused[k][1]))}
        return {"warp_workgroups": dict(zip(("staged", "interior_global", "generic"), [int(x) for x in cc.warp_workgroups])), "levels": lv}

    def stats(self):
        s = self._stats()
        return {k: getattr(s, k) for k, _ in s._fields_}

    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.hf_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class OpticalFlowCalcSDR(OpticalFlowCalc):
    """NV12, 8-bit (opticalFlowCalcSDR.h:10-56)."""
    is_hdr = False


class OpticalFlowCalcHDR(OpticalFlowCalc):
    """P010, 16-bit (opticalFlowCalcHDR.h:10-56)."""
    is_hdr = True


ERROR_TILE_DTYPE = np.dtype([("sse", "<u8"), ("sad", "<u4"), ("max_abs", "<u4")])   # struct hf_error_tile


def frame_error_maps(raw, n, tiles_x, tiles_y):
    """A downloaded map buffer of hf_frame_error_map_enqueue (bytes, or any array of n * 48 * tiles_y * tiles_x bytes) as a structured
    array [n][3][tiles_y][tiles_x] with fields sse, sad, max_abs; plane 0 Y, 1 U, 2 V.  A view, no copy."""
    a = np.ascontiguousarray(np.frombuffer(raw, dtype=np.uint8) if isinstance(raw, (bytes, bytearray, memoryview)) else raw).reshape(-1).view(np.uint8)
    need = n * 3 * tiles_y * tiles_x * ERROR_TILE_DTYPE.itemsize
    if a.size < need:
        raise ValueError(f"frame_error_maps: {a.size} bytes, {n} maps of 3 x {tiles_y} x {tiles_x} tiles need {need}")
    return a[:need].view(ERROR_TILE_DTYPE).reshape(n, 3, tiles_y, tiles_x)


def guard_weights(maps, tile, lo_q4, hi_q4, H, W, hdr):
    """The mask of hf_guarded_blend_enqueue from downloaded disagreement maps (frame_error_maps(): [n][3][th][tw]), steps 3 and 4 of its
    definition in include/hopperflow.h: (tile_weights [n][th][tw], luma_weights [n][H][W]), int64, 0 .. 256 -- 0 keeps the
    motion-compensated blend, 256 is the cross-fade.  A chroma element (cx, cy) takes luma_weights[k][2 * cy][cx & ~1]."""
    if tile not in (16, 32, 64) or not 0 <= lo_q4 < hi_q4 <= 65535:
        raise ValueError(f"guard_weights: tile {tile} not 16, 32 or 64, or thresholds {lo_q4}, {hi_q4} outside 0 <= lo_q4 < hi_q4 <= 65535")
    lg = tile.bit_length() - 1
    th, tw = (H + tile - 1) // tile, (W + tile - 1) // tile
    sad = np.asarray(maps["sad"])[:, 0].astype(np.int64)
    if sad.shape[1:] != (th, tw):
        raise ValueError(f"guard_weights: maps of {sad.shape[1:]} tiles, {H} x {W} at tile {tile} has {(th, tw)}")
    cnt = np.minimum(tile, H - tile * np.arange(th, dtype=np.int64))[:, None] * np.minimum(tile, W - tile * np.arange(tw, dtype=np.int64))[None, :]
    m = (16 * sad) // (cnt << (8 if hdr else 0))
    wt = np.where(m <= lo_q4, 0, np.where(m >= hi_q4, 256, ((m - lo_q4) * 256) // (hi_q4 - lo_q4))).astype(np.int64)
    u, v = np.arange(W, dtype=np.int64) - tile // 2, np.arange(H, dtype=np.int64) - tile // 2
    tx0, fx, ty0, fy = np.clip(u >> lg, 0, tw - 1), (u & (tile - 1))[None, None, :], np.clip(v >> lg, 0, th - 1), (v & (tile - 1))[None, :, None]
    tx1, ty1 = np.clip((u >> lg) + 1, 0, tw - 1), np.clip((v >> lg) + 1, 0, th - 1)
    pick = lambda ty, tx: wt[:, ty][:, :, tx]
    w = ((tile - fx) * (tile - fy) * pick(ty0, tx0) + fx * (tile - fy) * pick(ty0, tx1) + (tile - fx) * fy * pick(ty1, tx0) + fx * fy * pick(ty1, tx1)
         + tile * tile // 2) >> (2 * lg)
    return wt, w


SSIM_TILE_DTYPE = np.dtype([("sum_loss_q32", "<u8"), ("max_loss_q32", "<u8"), ("count", "<u4"), ("reserved", "<u4")])   # struct hf_ssim_tile


def frame_ssim_maps(raw, n, tiles_x, tiles_y):
    """A downloaded map buffer of hf_frame_ssim_map_enqueue (bytes, or any array of n * 72 * tiles_y * tiles_x bytes) as a structured
    array [n][3][tiles_y][tiles_x] with fields sum_loss_q32, max_loss_q32, count, reserved; plane 0 Y, 1 U, 2 V.  A view, no copy."""
    a = np.ascontiguousarray(np.frombuffer(raw, dtype=np.uint8) if isinstance(raw, (bytes, bytearray, memoryview)) else raw).reshape(-1).view(np.uint8)
    need = n * 3 * tiles_y * tiles_x * SSIM_TILE_DTYPE.itemsize
    if a.size < need:
        raise ValueError(f"frame_ssim_maps: {a.size} bytes, {n} maps of 3 x {tiles_y} x {tiles_x} tiles need {need}")
    return a[:need].view(SSIM_TILE_DTYPE).reshape(n, 3, tiles_y, tiles_x)


class DeviceBuffer:
    """A plain hipMalloc'ed buffer through the C ABI helpers (bench / batch staging)."""

    def __init__(self, nbytes, device_index=0):
        self._lib = capi.load()
        self.device_index, self.nbytes = device_index, nbytes
        p = C.c_void_p()
        capi.check(self._lib.hf_device_malloc(device_index, nbytes, C.byref(p)))
        self.ptr = p.value

    def upload(self, a):
        a = np.ascontiguousarray(a)
        assert a.nbytes <= self.nbytes
        capi.check(self._lib.hf_memcpy_h2d(self.device_index, C.c_void_p(self.ptr), _ptr(a), a.nbytes))

    def download(self, dtype, count=None):
        dt = np.dtype(dtype)
        n = count if count is not None else self.nbytes // dt.itemsize
        a = np.empty(n, dtype=dt)
        capi.check(self._lib.hf_memcpy_d2h(self.device_index, _ptr(a), C.c_void_p(self.ptr), a.nbytes))
        return a

    def free(self):
        if self.ptr:
            self._lib.hf_device_free(self.device_index, C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PinnedArray:
    """A numpy view of page-locked host memory (hf_host_malloc_pinned) for frame I/O at full PCIe rate."""

    def __init__(self, count, dtype):
        self._lib = capi.load()
        dt = np.dtype(dtype)
        p = C.c_void_p()
        capi.check(self._lib.hf_host_malloc_pinned(count * dt.itemsize, C.byref(p)))
        self.ptr = p.value
        self.array = np.ctypeslib.as_array((C.c_ubyte * (count * dt.itemsize)).from_address(self.ptr)).view(dt)

    def free(self):
        if self.ptr:
            self.array = None
            self._lib.hf_host_free_pinned(C.c_void_p(self.ptr))
            self.ptr = None


class FlowBatch:
    """hf_batch: calculateOpticalFlow() of up to 32 contexts (independent frame pairs, same geometry and parameters)
    as one set of launches.  While the batch exists its members issue on one stream; close() it before them."""

    def __init__(self, members):
        self._lib = capi.load()
        self.members = list(members)
        arr = (C.c_void_p * len(self.members))(*[m._ctx for m in self.members])
        out = C.c_void_p()
        rc = self._lib.hf_batch_create(arr, len(self.members), C.byref(out))
        if rc != 0:
            raise capi.HopperFlowError(rc, (self._lib.hf_batch_last_error(None) or b"").decode())
        self._b = out

    def defersPlanes(self):
        """hf_batch_defers_planes: runPeriod samples only the grid of a new frame, the next period's warp launch builds its plane"""
        return bool(self._lib.hf_batch_defers_planes(self._b))

    def planar(self):
        """hf_batch_planar: (inputs planar, caller-owned outputs planar) -- the leader's HF_FLAG_BATCH_PLANAR_IN / HF_FLAG_BATCH_PLANAR_OUT"""
        bits = self._lib.hf_batch_planar(self._b)
        return bool(bits & 1), bool(bits & 2)

    def calculateOpticalFlow(self):
        self._check(self._lib.hf_batch_calculate_optical_flow(self._b))

    def _check(self, rc):
        if rc != 0:
            raise capi.HopperFlowError(rc, (self._lib.hf_batch_last_error(self._b) or b"").decode())

    def updateFramesDeviceRef(self, dev_ptrs):
        """updateFrameDeviceRef of every member; the phase planes of all new frames are built by one launch."""
        arr = (C.c_void_p * len(self.members))(*[int(p) for p in dev_ptrs])
        self._check(self._lib.hf_batch_update_frames_device_ref(self._b, arr))

    @staticmethod
    def _row(scalars):
        """Entries per member of the t / device_out arrays: HF_MAX_PERIOD_OUTPUTS (the narrow calls) unless some member's list is longer --
        then the longest list, which the *_wide calls take (more than HF_MAX_PERIOD_OUTPUTS_WIDE: they raise the library's error)."""
        return max([capi.HF_MAX_PERIOD_OUTPUTS] + [len(ts) for ts in scalars])

    def _marshal(self, scalars, out_ptrs):
        n, K = len(self.members), self._row(scalars)
        counts = (C.c_int * n)(*[len(ts) for ts in scalars])
        t = (C.c_float * (n * K))()
        outs = (C.c_void_p * (n * K))()
        for i, ts in enumerate(scalars):
            for k, x in enumerate(ts):
                t[i * K + k] = float(x)
                outs[i * K + k] = int(out_ptrs[i][k])
        return K, counts, t, outs

    def interpolatePeriod(self, scalars, out_ptrs, mode=BlendedFrame):
        """The warps of one source period of every member in ONE launch per chunk of 6 outputs.  scalars[i] / out_ptrs[i]: member i's lists
        (more than 6 entries in some list: hf_batch_interpolate_period_wide)."""
        K, counts, t, outs = self._marshal(scalars, out_ptrs)
        if K > capi.HF_MAX_PERIOD_OUTPUTS:
            self._check(self._lib.hf_batch_interpolate_period_wide(self._b, K, counts, t, outs, int(mode)))
        else:
            self._check(self._lib.hf_batch_interpolate_period(self._b, counts, t, outs, int(mode)))

    def preparePeriod(self, dev_ptrs, scalars, out_ptrs, mode=BlendedFrame, calculate_flow=True):
        """The arguments of one hf_batch_run_period call, marshalled once (a driver's schedule is known ahead of time);
        dev_ptrs / scalars may be None to skip the update / the warps.  A list of more than 6 scalars makes it the argument tuple of
        hf_batch_run_period_wide (one element more: the row, after calculate_flow); runPeriod tells the two apart by their length."""
        n = len(self.members)
        frames = (C.c_void_p * n)(*[int(p) for p in dev_ptrs]) if dev_ptrs is not None else None
        K, counts, t, outs = capi.HF_MAX_PERIOD_OUTPUTS, None, None, None
        if scalars is not None:
            K, counts, t, outs = self._marshal(scalars, out_ptrs)
        if K > capi.HF_MAX_PERIOD_OUTPUTS:
            return (frames, 1 if calculate_flow else 0, K, counts, t, outs, int(mode))
        return (frames, 1 if calculate_flow else 0, counts, t, outs, int(mode))

    def runPeriod(self, prepared):
        """updateFramesDeviceRef + calculateOpticalFlow + interpolatePeriod of one source period in ONE native call."""
        rc = (self._lib.hf_batch_run_period if len(prepared) == 6 else self._lib.hf_batch_run_period_wide)(self._b, *prepared)
        if rc != 0:
            self._check(rc)

    def sceneSet(self, member, source_frame_time, threshold=-1):
        """hf_batch_scene_set: arms / re-arms member's scene-change history (NewSegment); threshold < 0 = DEFAULT_SCENE_CHANGE_THRESHOLD."""
        self._check(self._lib.hf_batch_scene_set(self._b, int(member), int(source_frame_time), int(threshold)))

    def runPeriodAuto(self, dev_ptrs, scalars, out_ptrs, mode=BlendedFrame, force_kind=None):
        """hf_batch_run_period_auto: one source period of every member, warp or copy decided on the device; only enqueues.
        scalars[i] / out_ptrs[i]: member i's lists (an empty list: no output; more than 6 entries in some list:
        hf_batch_run_period_auto_wide); force_kind: None or per member -1 decide / 0 copy / 1 warp.  A batch that defers its phase planes
        takes it with HF_FLAG_BATCH_AUTO_DEFERRED on its leader (the warps of chunk 0 stay ahead of the chain)."""
        prepared = self.preparePeriod(dev_ptrs, scalars, out_ptrs, mode)
        force = (C.c_int32 * len(self.members))(*[int(k) for k in force_kind]) if force_kind is not None else None
        if len(prepared) == 6:
            frames, _, counts, t, outs, mode = prepared
            rc = self._lib.hf_batch_run_period_auto(self._b, frames, counts, t, outs, mode, force)
        else:
            frames, _, row, counts, t, outs, mode = prepared
            rc = self._lib.hf_batch_run_period_auto_wide(self._b, frames, row, counts, t, outs, mode, force)
        if rc != 0:
            self._check(rc)

    def sceneRead(self, member):
        """hf_batch_scene_read (after sync()): member's records since the last read, in period order, as dicts of
        frame_count, total_delta, kind (1 warp / 0 copy), average, d1, d2."""
        n = C.c_int(0)
        self._check(self._lib.hf_batch_scene_read(self._b, int(member), None, 0, C.byref(n)))
        if n.value == 0:
            return []
        recs = (capi.HfSceneRecord * n.value)()
        self._check(self._lib.hf_batch_scene_read(self._b, int(member), recs, n.value, C.byref(n)))
        return [{k: getattr(r, k) for k, _ in r._fields_} for r in recs[:n.value]]

    def sync(self):
        self._check(self._lib.hf_batch_sync(self._b))

    def timelineEnable(self, max_launches, skip_periods=0):
        """hf_batch_timeline_enable: after skip_periods further runPeriod calls every dispatch carries its own start / stop events (0: off)."""
        self._check(self._lib.hf_batch_timeline_enable(self._b, int(max_launches), int(skip_periods)))

    def timelineRead(self):
        """hf_batch_timeline_read: [(kernel, period, start_ms, end_ms)] on the device's clock, relative to the process's reference event."""
        n = C.c_int(0)
        self._check(self._lib.hf_batch_timeline_read(self._b, None, 0, C.byref(n)))
        if n.value == 0:
            return []
        recs = (capi.HfTimelineRecord * n.value)()
        self._check(self._lib.hf_batch_timeline_read(self._b, recs, n.value, C.byref(n)))
        return [(r.kernel.decode(), r.period, r.start_ms, r.start_ms + r.duration_ms) for r in recs[:n.value] if not (r.flags & 1)]

    def __len__(self):
        return self._lib.hf_batch_size(self._b)

    def close(self):
        if self._b:
            self._lib.hf_batch_destroy(self._b)
            self._b = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

