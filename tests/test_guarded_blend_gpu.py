"""GPU: the device's guarded blend (hf_guarded_blend_enqueue, csrc/hf_kernels.hip) -- per blending scalar the blended frame, faded into
the cross-fade of the two source frames where the warped halves disagree.  Every case is held twice: to the model of
tests/guarded_blend_model.py (the oracle's mode-2 frames with the flow and with a zero flow, the disagreement model, the integer weights),
every element of columns [0, W) EQUAL, and to the composition on the device -- warpFrames(t, 2) into two buffers, one with the flow and
one after writeBlurredFlow(0, zeros), warpDisagreementMapEnqueue, the mix in numpy -- frames and maps byte for byte.  The flow is
injected with writeBlurredFlow; map and frame buffers are prefilled with 0xFF bytes.  The padding columns of a frame are unspecified by
the definition and not asserted; the bytes behind a frame's last row are."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded_blend_model as gbm  # noqa: E402
import test_warp_disagreement_gpu as WD  # noqa: E402  (its Rig, geometries and flows: the launch this call runs first)
from warp_disagreement_model import warp_disagreement_maps  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

INVALID = -1   # HF_ERR_INVALID_ARGUMENT
T5, T24 = WD.T5, WD.T24
TAIL = 64


class Rig(WD.Rig):
    """WD.Rig with frame buffers for the call's outputs, each with TAIL sentinel bytes behind the frame."""

    def __init__(self, hdr, H, W, res=270, in_stride=0, out_stride=0, by_ref=False, flags=None, seed=1, frames=None, levels=(0.0, 255.0)):
        g = WD._geom(hdr, H, W, in_stride, out_stride, res)
        if frames is None:
            frames = gbm.guard_frames(np.random.default_rng(seed), hdr, g)
        super().__init__(hdr, H, W, res, in_stride, out_stride, by_ref, flags, seed + 1000, frames)
        self.levels = levels
        self.c.m_outputBlackLevel, self.c.m_outputWhiteLevel = levels
        self.dt = np.uint16 if hdr else np.uint8
        self.fbytes = self.c.output_frame_bytes
        self.rows, self.so = H + H // 2, self.g.out_stride
        assert self.fbytes == self.rows * self.so * np.dtype(self.dt).itemsize
        self.gout = []

    def outs(self, n):
        from hopperrender_amd.calc import DeviceBuffer
        while len(self.gout) < n:
            self.gout.append(DeviceBuffer(self.fbytes + TAIL))
        for b in self.gout[:n]:
            b.upload(np.full(self.fbytes + TAIL, 0xFF, np.uint8))
        return self.gout[:n]

    def frames_of(self, bufs):
        out = np.empty((len(bufs), self.rows, self.so), self.dt)
        for k, b in enumerate(bufs):
            raw = b.download(np.uint8)
            assert (raw[self.fbytes:] == 0xFF).all(), f"bytes behind the last row of frame {k} were written"
            out[k] = raw[:self.fbytes].view(self.dt).reshape(self.rows, self.so)
        return out

    def device(self, ts, tile, lo, hi):
        """the new call, enqueued behind whatever the context has in flight: (frames [n][rows][out stride], raw bytes of the maps)"""
        nbytes = self.shape(tile)[2] * len(ts)
        buf, outs = self._buf(nbytes), self.outs(len(ts))
        self.c.guardedBlendEnqueue(ts, tile, lo, hi, buf.ptr, [o.ptr for o in outs])
        self.c.sync()
        raw = buf.download(np.uint8)
        assert (raw[nbytes:] == 0xFF).all(), "bytes behind the last map were written"
        return self.frames_of(outs), raw[:nbytes].copy()

    def warped(self, t, flow=None):
        """warpFrames(t, 2) into a buffer; flow: injected for this warp only"""
        if flow is not None:
            self.c.sync()
            keep = self.c.readBlurredFlow(0)
            self.c.writeBlurredFlow(0, flow)
        self.c.setOutputBuffer(self.out[0].ptr)
        self.c.warpFrames(t, 2)
        self.c.setOutputBuffer(None)
        self.c.sync()
        if flow is not None:
            self.c.writeBlurredFlow(0, keep)
        return self.out[0].download(self.dt, self.rows * self.so).reshape(self.rows, self.so)

    def composed(self, ts, tile, lo, hi):
        """step 7 of the definition on the device: M and Z by two warps per t, the maps by the disagreement call, the mix in numpy"""
        from hopperrender_amd.calc import guard_weights
        nbytes = self.shape(tile)[2] * len(ts)
        buf = self._buf(nbytes)
        self.c.warpDisagreementMapEnqueue(ts, tile, buf.ptr)
        self.c.sync()
        raw = buf.download(np.uint8)[:nbytes].copy()
        _, w = guard_weights(self.view(raw, len(ts), tile), tile, lo, hi, self.H, self.W, self.hdr)
        w = gbm.element_weights(w, self.H, self.W, self.so)
        zeros = np.zeros((2, self.g.lh, self.g.lw), np.int16)
        out, done = np.empty((len(ts), self.rows, self.so), self.dt), {}
        for k, t in enumerate(ts):
            if float(t) not in done:
                done[float(t)] = (self.warped(t).copy(), self.warped(t, zeros).copy())
            out[k] = gbm.mix(*done[float(t)], w[k])
        return out, raw, w

    def check(self, flow, ts, tile, lo, hi, what, model=True):
        """the flow injected, then the new call against the model and against the composition; returns (frames, element weights)"""
        self.c.sync()
        self.c.writeBlurredFlow(0, flow)
        W = self.W
        got, maps = self.device(ts, tile, lo, hi)
        if model:
            want, wmaps, _ = gbm.guarded_blend(self.f[0], self.f[1], flow, self.g, [np.float32(t) for t in ts], tile, lo, hi, *self.levels)
            assert np.array_equal(self.view(maps, len(ts), tile), wmaps), f"{what}: the maps differ from the model"
            if not np.array_equal(got[:, :, :W], want[:, :, :W]):
                bad = np.argwhere(got[:, :, :W] != want[:, :, :W])
                i = tuple(bad[0])
                raise AssertionError(f"{what}: {len(bad)} of {want[:, :, :W].size} elements differ from the model; first at [t, row, column] = {i}: device {got[i]}, model {want[i]}")
        comp, cmaps, w = self.composed(ts, tile, lo, hi)
        assert np.array_equal(maps, cmaps), f"{what}: {np.count_nonzero(maps != cmaps)} map bytes differ from the disagreement call's"
        assert np.array_equal(got[:, :, :W], comp[:, :, :W]), f"{what}: {np.count_nonzero(got[:, :, :W] != comp[:, :, :W])} elements differ from the composition on the device"
        return got, w[:, :, :W]

    def close(self):
        super().close()
        for b in self.gout:
            b.free()


def run_geometry(name, hdr, kinds=("zero", "far+", "far-", "odd", "random"), rss=(0, 1, 2, 3), ts=T5, tiles=None):
    H, W, res, si, so, by_ref, all_tiles = WD.GEOMETRIES[name]
    for rs in rss:
        r = Rig(hdr, H, W, res[rs], si, so, by_ref, seed=17 + rs + 4 * hdr)
        try:
            assert r.c.m_opticalFlowResScalar == rs
            fl = WD.flows(r.g, r.rng)
            for tile in tiles or all_tiles:
                lo, hi = gbm.thresholds_around(warp_disagreement_maps(r.f[0], r.f[1], fl["random"], r.g, [np.float32(t) for t in T5], tile), tile, H, W, hdr)
                seen = set()
                for kind in kinds:
                    _, w = r.check(fl[kind], ts, tile, lo, hi, (name, hdr, rs, kind, tile, lo, hi))
                    seen |= set(np.unique(w).tolist())
                if "zero" in kinds and "random" in kinds:
                    assert 0 in seen and 256 in seen and any(0 < v < 256 for v in seen), (name, hdr, rs, tile, sorted(seen))
        finally:
            r.close()


@pytest.mark.parametrize("hdr", [False, True], ids=["sdr", "hdr"])
@pytest.mark.parametrize("name", list(WD.GEOMETRIES))
def test_geometries_flows_tiles_and_resolution_scalars(native_lib, name, hdr):
    """Every geometry at rs 0 .. 3, every flow, every tile, t = 0, .3996, .5, .998 and 1 in one call; thresholds around the mean of the
    random part, so that store groups with and without a weight, and weights 0, 256 and between, occur in every geometry (asserted)."""
    run_geometry(name, hdr)


@pytest.mark.parametrize("hdr", [False, True], ids=["sdr", "hdr"])
def test_output_levels(native_lib, hdr):
    """black 16 / white 235: M and Z carry the levels, the mix is behind them"""
    r = Rig(hdr, 50, 86, 25, 0, 96, levels=(16.0, 235.0), seed=3 + hdr)
    try:
        fl = WD.flows(r.g, r.rng)
        lo, hi = gbm.thresholds_around(warp_disagreement_maps(r.f[0], r.f[1], fl["random"], r.g, [np.float32(t) for t in T5], 16), 16, 50, 86, hdr)
        got, w = r.check(fl["random"], T5, 16, lo, hi, ("levels", hdr))
        plain = Rig(hdr, 50, 86, 25, 0, 96, seed=3 + hdr)
        try:
            other, _ = plain.check(fl["random"], T5, 16, lo, hi, ("no levels", hdr), model=False)
            assert not np.array_equal(got, other)
        finally:
            plain.close()
    finally:
        r.close()


@pytest.mark.parametrize("hdr", [False, True], ids=["sdr", "hdr"])
@pytest.mark.parametrize("n", [1, 24])
def test_outputs_per_call(native_lib, hdr, n):
    """n_t = 1, and n_t = 24: four blend launches of six outputs each, every frame in its own buffer and its own map's weights"""
    r = Rig(hdr, 50, 86, 25, 0, 96, seed=5 + hdr)
    try:
        fl = WD.flows(r.g, r.rng)
        ts = T24[:n] if n > 1 else [0.3996]
        lo, hi = gbm.thresholds_around(warp_disagreement_maps(r.f[0], r.f[1], fl["random"], r.g, [np.float32(t) for t in T24], 16), 16, 50, 86, hdr)
        got, w = r.check(fl["random"], ts, 16, lo, hi, ("n_t", n))
        assert got.shape[0] == n
        if n > 1:
            assert len({got[k].tobytes() for k in range(n)}) == n and len({w[k].tobytes() for k in range(n)}) > n // 2
    finally:
        r.close()


@pytest.mark.parametrize("hdr", [False, True], ids=["sdr", "hdr"])
def test_guard_extremes(native_lib, hdr):
    """Guard off: bytewise the warpFrames(t, 2) frame, no store group loads the cross-fade.  lo = 0, hi = 1 on random frames: bytewise the
    zero-flow frame, every group loads it."""
    H, W = 50, 86
    g = WD._geom(hdr, H, W, 0, 96, 25)
    rng = np.random.default_rng(23 + hdr)
    r = Rig(hdr, H, W, 25, 0, 96, frames=[WD._random_frame(rng, hdr, g) for _ in range(3)])
    try:
        flow = WD.flows(r.g, rng)["random"]
        zeros = np.zeros_like(flow)
        off, w0 = r.check(flow, T5, 16, *gbm.GUARD_OFF, "guard off")
        on, w1 = r.check(flow, T5, 16, 0, 1, "guard all on")
        assert not w0.any() and (w1 == 256).all()
        for k, t in enumerate(T5):
            M, Z = r.warped(t), r.warped(t, zeros)
            assert np.array_equal(off[k][:, :W], M[:, :W]) and np.array_equal(on[k][:, :W], Z[:, :W])
            assert np.array_equal(M, Z) == (t in (0.0, 1.0))
    finally:
        r.close()


def test_a_saturated_hdr_tile(native_lib):
    """64 x 64 HDR, frame N-2 all 0 against frame N-1 all 65535: m = 4095 at every tile size, the largest there is"""
    H = W = 64
    g = WD._geom(True, H, W)
    n = H * W * 3 // 2
    r = Rig(True, H, W, frames=[np.zeros(n, np.uint16), np.full(n, 65535, np.uint16), np.zeros(n, np.uint16)])
    try:
        for tile in WD.TILES:
            _, w = r.check(np.zeros((2, g.lh, g.lw), np.int16), [0.5], tile, 0, 65535, ("saturated", tile))
            assert (w == 15).all()
            _, w = r.check(np.zeros((2, g.lh, g.lw), np.int16), [0.5], tile, 4094, 4095, ("saturated, all on", tile))
            assert (w == 256).all()
    finally:
        r.close()


def test_a_real_chain_on_a_moving_scene(native_lib):
    """A flow the chain itself calculated on synth.Scene frames (read back only for the model)."""
    from hopperrender_amd import synth
    H, W = 180, 320
    sc = synth.Scene(H, W, False, 21)
    f = [sc.frame(k) for k in range(4)]
    r = Rig(False, H, W, frames=f[:3])
    try:
        r.c.m_opticalFlowSearchRadius = 8
        r.c.calculateOpticalFlow()
        r.c.updateFrame(f[3])          # the ring: frames 1, 2 | 3, the previous flow: that of (1, 2)
        r.c.calculateOpticalFlow()
        r.c.sync()
        r.f = f[1:]
        flow = r.c.readBlurredFlow(0)
        assert np.count_nonzero(flow)
        lo, hi = gbm.thresholds_around(warp_disagreement_maps(r.f[0], r.f[1], flow, r.g, [np.float32(t) for t in T5], 16), 16, H, W, False)
        _, w = r.check(flow, T5, 16, lo, hi, "chain")
        assert w.min() == 0 and w.max() == 256
    finally:
        r.close()


def test_refusals_enqueue_nothing(native_lib):
    """Every refusal is HF_ERR_INVALID_ARGUMENT, names the call and leaves the sentinel-filled maps and frames as they were."""
    from hopperrender_amd import capi
    r = Rig(False, 50, 86, 25, 0, 96)
    L = capi.load()
    try:
        nbytes = r.shape(16)[2]
        buf = r._buf(24 * nbytes)
        outs = r.outs(24)
        fl = lambda *v: (C.c_float * len(v))(*v)
        ptrs = lambda ps: (C.c_void_p * len(ps))(*[C.c_void_p(p) for p in ps])
        all_out = ptrs([o.ptr for o in outs])
        enq = lambda n, t, tile, lo, hi, maps, out=all_out: L.hf_guarded_blend_enqueue(r.c._ctx, n, t, tile, lo, hi, C.c_void_p(maps), out)
        ok5 = fl(*T5)
        bad = {f"tile {t}": enq(5, ok5, t, 32, 96, buf.ptr) for t in (0, -16, 8, 17, 48, 128)}
        bad.update({
            "null t": enq(5, None, 16, 32, 96, buf.ptr), "n = 0": enq(0, ok5, 16, 32, 96, buf.ptr), "n < 0": enq(-1, ok5, 16, 32, 96, buf.ptr),
            "n = 25": enq(25, fl(*([0.5] * 25)), 16, 32, 96, buf.ptr, ptrs([o.ptr for o in outs] + [outs[0].ptr])),
            "t above 1": enq(3, fl(0.5, 1.0001, 0.2), 16, 32, 96, buf.ptr), "last t above 1": enq(24, fl(*([0.5] * 23 + [2.0])), 16, 32, 96, buf.ptr),
            "null maps": enq(5, ok5, 16, 32, 96, None), "maps 8 bytes in": enq(5, ok5, 16, 32, 96, buf.ptr + 8), "maps 4 bytes in": enq(5, ok5, 16, 32, 96, buf.ptr + 4),
            "null outputs": enq(5, ok5, 16, 32, 96, buf.ptr, None),
            "first output null": enq(5, ok5, 16, 32, 96, buf.ptr, ptrs([None] + [o.ptr for o in outs[:4]])),
            "last output null": enq(5, ok5, 16, 32, 96, buf.ptr, ptrs([o.ptr for o in outs[:4]] + [None])),
            "lo below 0": enq(5, ok5, 16, -1, 96, buf.ptr), "lo = hi": enq(5, ok5, 16, 96, 96, buf.ptr), "lo above hi": enq(5, ok5, 16, 97, 96, buf.ptr),
            "hi above 65535": enq(5, ok5, 16, 32, 65536, buf.ptr), "lo = hi = 0": enq(5, ok5, 16, 0, 0, buf.ptr),
            "null context": L.hf_guarded_blend_enqueue(None, 5, ok5, 16, 32, 96, C.c_void_p(buf.ptr), all_out),
        })
        assert {k: v for k, v in bad.items() if v != INVALID} == {}
        assert b"hf_guarded_blend_enqueue" in L.hf_last_error(r.c._ctx)
        r.c.sync()
        assert (buf.download(np.uint8) == 0xFF).all()
        for o in outs:
            assert (o.download(np.uint8) == 0xFF).all()
        with pytest.raises(capi.HopperFlowError) as e:
            r.c.guardedBlendEnqueue([0.5], 16, 96, 32, buf.ptr, [outs[0].ptr])
        assert e.value.code == INVALID
        with pytest.raises(ValueError):
            r.c.guardedBlendEnqueue([0.5, 0.6], 16, 32, 96, buf.ptr, [outs[0].ptr])
        assert enq(24, fl(*T24), 16, 0, 65535, buf.ptr) == 0 and enq(1, fl(-0.25), 64, 4080, 4081, buf.ptr) == 0   # (a t below 0 is hf_warp_frames' to take, too)
        r.c.sync()
    finally:
        r.close()


@pytest.mark.parametrize("dual", [False, True], ids=["async", "dual-stream"])
def test_straight_behind_a_period_without_a_sync(native_lib, dual):
    """interpolatePeriod, then the call at once: equal to the composition made after a sync and to the model, on the frames and the flow
    that period's warps used; the output frame, m_warpCalcTime and the debug counters are as the period left them."""
    from hopperrender_amd import capi, synth
    from hopperrender_amd.calc import DeviceBuffer
    H, W, tile, ts = 360, 640, 32, [0.25, 0.5]
    sc = synth.Scene(H, W, True, 78)
    f = [sc.frame(k) for k in range(4)]
    r = Rig(True, H, W, by_ref=True, frames=f[:2], flags=capi.HF_FLAG_ASYNC | (capi.HF_FLAG_DUAL_STREAM if dual else 0))
    more = [DeviceBuffer(x.nbytes) for x in f[2:]]
    period_out = DeviceBuffer(r.c.output_frame_bytes)
    try:
        r.c.m_opticalFlowSearchRadius = 8
        r.c.countersEnable()
        for b, x in zip(more, f[2:]):
            b.upload(x)
        lo, hi = 300, 600   # (the scene's tiles disagree by 10 .. 1500 sixteenths at t = 0.5, half of them by 300 .. 550)
        r.c.interpolatePeriod(more[0].ptr, [0.5], [period_out.ptr])
        r.c.interpolatePeriod(more[1].ptr, ts, [period_out.ptr, r.out[1].ptr])   # shows the pair (1, 2) with the flow of the period before
        got, maps = r.device(ts, tile, lo, hi)                                   # enqueued at once; the sync is behind it
        before = (r.c.downloadFrame().copy(), r.c.m_warpCalcTime, r.c.counters(), period_out.download(np.uint16))
        again, maps2 = r.device(ts, tile, lo, hi)
        after = (r.c.downloadFrame().copy(), r.c.m_warpCalcTime, r.c.counters(), period_out.download(np.uint16))
        assert np.array_equal(before[0], after[0]) and before[1] == after[1] and before[2] == after[2] and np.array_equal(before[3], after[3])
        comp, cmaps, w = r.composed(ts, tile, lo, hi)
        assert np.array_equal(maps, cmaps) and np.array_equal(maps2, cmaps)
        assert np.array_equal(got[:, :, :W], comp[:, :, :W]) and np.array_equal(again[:, :, :W], comp[:, :, :W])
        flow = r.c.readBlurredFlow(0)
        want, wmaps, _ = gbm.guarded_blend(f[1], f[2], flow, r.g, [np.float32(t) for t in ts], tile, lo, hi)
        assert np.array_equal(got[:, :, :W], want[:, :, :W]) and np.array_equal(r.view(maps, 2, tile), wmaps)
        assert 0 < w.mean() < 256 and len(np.unique(w)) > 2
    finally:
        r.close()
        for b in more + [period_out]:
            b.free()


def test_members_of_a_batch(native_lib):
    """Two members behind hf_batch_run_period, no sync between: each member's frames are the model's on the frames and the flow that
    period's warps used; with the guard off they are bytewise what hf_batch_interpolate_period writes in mode 2."""
    from hopperrender_amd import capi, synth
    from hopperrender_amd.calc import DeviceBuffer, FlowBatch, frame_error_maps
    H, W, tile, ts, lo, hi = 180, 320, 16, [0.3996, 0.7992], 300, 700
    scs = [synth.Scene(H, W, False, 31 + i) for i in range(2)]
    fr = [[sc.frame(k) for k in range(4)] for sc in scs]
    ms = [WD._cls(False)(H, W, search_radius=8, flags=capi.HF_FLAG_ASYNC) for _ in range(2)]
    g = WD._geom(False, H, W)
    dev = [[DeviceBuffer(x.nbytes) for x in f] for f in fr]
    for bs, f in zip(dev, fr):
        for b, x in zip(bs, f):
            b.upload(x)
    fbytes = ms[0].output_frame_bytes
    outs = [[DeviceBuffer(fbytes) for _ in range(6)] for _ in range(2)]
    tw, th, nbytes = ms[0].frameErrorMapShape(tile)
    maps = [DeviceBuffer(2 * nbytes) for _ in range(4)]
    batch = FlowBatch(ms)
    try:
        for k in range(4):
            batch.runPeriod(batch.preparePeriod([dev[i][k].ptr for i in range(2)], [ts] * 2, [[o.ptr for o in outs[i][:2]] for i in range(2)], 2))
        for i, m in enumerate(ms):   # straight behind the period, no sync
            m.guardedBlendEnqueue(ts, tile, lo, hi, maps[i].ptr, [o.ptr for o in outs[i][2:4]])
            m.guardedBlendEnqueue(ts, tile, *gbm.GUARD_OFF, maps[2 + i].ptr, [o.ptr for o in outs[i][4:6]])
        batch.sync()
        got = [[o.download(np.uint8).reshape(H + H // 2, g.out_stride)[:, :W].copy() for o in outs[i][2:6]] for i in range(2)]
        batch.interpolatePeriod([ts] * 2, [[o.ptr for o in outs[i][:2]] for i in range(2)], 2)
        batch.sync()
        for i, m in enumerate(ms):
            flow = m.readBlurredFlow(0)
            want, wmaps, w = gbm.guarded_blend(fr[i][1], fr[i][2], flow, g, [np.float32(t) for t in ts], tile, lo, hi)
            raw = maps[i].download(np.uint8)
            assert np.array_equal(frame_error_maps(raw, 2, tw, th), wmaps) and np.array_equal(raw, maps[2 + i].download(np.uint8)), i
            for k in range(2):
                assert np.array_equal(got[i][k], want[k][:, :W]), (i, k)
                assert np.array_equal(got[i][2 + k], outs[i][k].download(np.uint8).reshape(H + H // 2, g.out_stride)[:, :W]), (i, k)
            assert 0 < w.mean() < 256 and len(np.unique(w)) > 2 and not np.array_equal(got[i][0], got[i][2])
        assert not np.array_equal(got[0][0], got[1][0])
    finally:
        batch.close()
        for m in ms:
            m.close()
        for b in [x for row in dev + outs for x in row] + maps:
            b.free()


CHILD = r"""
import sys, ctypes as C
sys.path.insert(0, {root!r}); sys.path.insert(0, {root!r} + "/tests")
from hopperrender_amd import capi
from hopperrender_amd.calc import OpticalFlowCalcSDR
import test_guarded_blend_gpu as GB

def violations(c):
    n = C.c_uint32(0); first = (C.c_uint32 * 4)()
    capi.check(c._lib.hf_debug_bounds_violations(c._ctx, C.byref(n), first, 0), c._ctx)
    return n.value, list(first)

assert capi.is_debug_bounds_build()
probe = OpticalFlowCalcSDR(64, 96)
for hdr in (False, True):
    GB.run_geometry("86x50", hdr, kinds=("far+", "far-", "random"))          # the mirror flows at every edge, rs 0 .. 3
    assert violations(probe)[0] == 0, ("86x50", hdr, violations(probe))
    GB.run_geometry("200x120-stride208-ref", hdr, kinds=("odd", "random"), rss=(3,), ts=GB.T24)
    assert violations(probe)[0] == 0, ("200x120", hdr, violations(probe))
probe.close()
print("GUARDED-BLEND-DEBUG-BOUNDS-OK")
"""


def test_subset_under_the_bounds_checking_build(native_lib):
    """The mirror flows at 86 x 50 and an rs = 3 case with 24 outputs under -DHF_DEBUG_BOUNDS in a child process: zero violations, the
    same frames (the cases' own assertions against the model and the composition)."""
    from hopperrender_amd import build
    dbg = build.build_flow(debug_bounds=True)
    env = dict(os.environ, HF_LIB=dbg)
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT)], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0 and "GUARDED-BLEND-DEBUG-BOUNDS-OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
