"""GPU: the device's warp disagreement maps (hf_warp_disagreement_map_enqueue, csrc/hf_kernels.hip) -- per blending scalar and tile, how far
the two warped halves of an output are apart, in one launch and without writing a frame.  Every case is held twice: to the model of
tests/warp_disagreement_model.py (the oracle's warps with modes 0 and 1 under the numpy error map), every field of every tile EQUAL, and
to the composition on the device -- warpFrames(t, 0) and warpFrames(t, 1) into two buffers, frameErrorMapEnqueue over them -- byte for
byte.  The flow is injected with writeBlurredFlow; map buffers are prefilled with 0xFF bytes, so an entry the launch did not write shows."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import warp_disagreement_model as wdm  # noqa: E402
from frame_error_map_model import TILES  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

INVALID = -1   # HF_ERR_INVALID_ARGUMENT
T5 = [0.0, 0.3996, 0.5, 0.998, 1.0]
T24 = [k / 23.0 for k in range(24)]   # HF_MAX_DISAGREEMENT_OUTPUTS: four trips of the kernel's loop over chunks of six outputs


def _cls(hdr):
    from hopperrender_amd.calc import OpticalFlowCalcHDR, OpticalFlowCalcSDR
    return OpticalFlowCalcHDR if hdr else OpticalFlowCalcSDR


def _geom(hdr, H, W, in_stride=0, out_stride=0, res=270):
    from oracle import oracle
    return oracle.make_geom(int(hdr), H, W, in_stride, out_stride, res)


def _random_frame(rng, hdr, g):
    from oracle import oracle
    return rng.integers(0, 65536 if hdr else 256, size=oracle.in_elems(g), dtype=oracle.frame_dtype(hdr))


def flows(g, rng):
    """the injected flows of a geometry, by name"""
    z = np.zeros((2, g.lh, g.lw), np.int16)
    far = lambda s: np.stack([np.full((g.lh, g.lw), s * (g.W + 5), np.int16), np.full((g.lh, g.lw), s * (g.H + 5), np.int16)])
    odd = z.copy()
    odd[0] = 2 * rng.integers(-4, 4, size=(g.lh, g.lw)) + 1   # odd x displacements at t = 1 and t = 0: the chroma parity rule
    odd[1] = rng.integers(-3, 4, size=(g.lh, g.lw))
    return {"zero": z, "far+": far(1), "far-": far(-1), "odd": odd, "random": rng.integers(-300, 301, size=z.shape).astype(np.int16)}


class Rig:
    """One context with frames N-2 / N-1 in its ring (a third on top), two output buffers and two map buffers."""

    def __init__(self, hdr, H, W, res=270, in_stride=0, out_stride=0, by_ref=False, flags=None, seed=1, frames=None):
        from hopperrender_amd import capi
        from hopperrender_amd.calc import DeviceBuffer
        self.hdr, self.H, self.W = hdr, H, W
        self.g = _geom(hdr, H, W, in_stride, out_stride, res)
        self.c = _cls(hdr)(H, W, in_stride, out_stride, 8, 6, 0.0, 255.0, res, flags=capi.HF_FLAG_ASYNC if flags is None else flags)
        assert self.c.m_opticalFlowResScalar == self.g.rs and (self.c.m_opticalFlowFrameWidth, self.c.m_opticalFlowFrameHeight) == (self.g.lw, self.g.lh)
        rng = np.random.default_rng(seed)
        self.f = frames if frames is not None else [_random_frame(rng, hdr, self.g) for _ in range(3)]
        self.bufs = []
        if by_ref:
            for x in self.f:
                b = DeviceBuffer(x.nbytes)
                b.upload(x)
                self.bufs.append(b)
                self.c.updateFrameDeviceRef(b.ptr)
        else:
            for x in self.f:
                self.c.updateFrame(x)
        self.out = [DeviceBuffer(self.c.output_frame_bytes) for _ in range(2)]
        self.maps = {}
        self.rng = rng

    def shape(self, tile):
        return self.c.frameErrorMapShape(tile)

    def _buf(self, nbytes):
        from hopperrender_amd.calc import DeviceBuffer
        if nbytes not in self.maps:
            self.maps[nbytes] = DeviceBuffer(nbytes + 64)
        self.maps[nbytes].upload(np.full(nbytes + 64, 0xFF, np.uint8))
        return self.maps[nbytes]

    def device(self, ts, tile):
        """the new call, enqueued behind whatever the context has in flight: raw bytes of len(ts) maps"""
        nbytes = self.shape(tile)[2] * len(ts)
        buf = self._buf(nbytes)
        self.c.warpDisagreementMapEnqueue(ts, tile, buf.ptr)
        self.c.sync()
        raw = buf.download(np.uint8)
        assert (raw[nbytes:] == 0xFF).all(), "bytes behind the last map were written"
        return raw[:nbytes].copy()

    def composed(self, ts, tile):
        """three launches per t: mode 0 and mode 1 into two buffers, the error map of the two"""
        one = self.shape(tile)[2]
        raw = np.empty(one * len(ts), np.uint8)
        done = {}
        for k, t in enumerate(ts):
            if float(t) not in done:
                buf = self._buf(one)
                for mode in (0, 1):
                    self.c.setOutputBuffer(self.out[mode].ptr)
                    self.c.warpFrames(t, mode)
                self.c.setOutputBuffer(None)
                self.c.frameErrorMapEnqueue([self.out[0].ptr], [self.out[1].ptr], tile, buf.ptr, self.g.out_stride, self.g.out_stride)
                self.c.sync()
                done[float(t)] = buf.download(np.uint8)[:one].copy()
            raw[k * one:(k + 1) * one] = done[float(t)]
        return raw

    def view(self, raw, n, tile):
        from hopperrender_amd.calc import frame_error_maps
        tw, th, _ = self.shape(tile)
        return frame_error_maps(raw, n, tw, th)

    def check(self, flow, ts, tile, what, model=True):
        """the flow injected, then the new call against the model and against the composition"""
        self.c.sync()
        self.c.writeBlurredFlow(0, flow)
        got = self.device(ts, tile)
        maps = self.view(got, len(ts), tile)
        if model:
            want = wdm.warp_disagreement_maps(self.f[0], self.f[1], flow, self.g, [np.float32(t) for t in ts], tile)
            if not np.array_equal(maps, want):
                bad = np.argwhere(maps != want)
                i = tuple(bad[0])
                raise AssertionError(f"{what}: {len(bad)} of {maps.size} entries differ from the model; first at [t, plane, ty, tx] = {i}: device {maps[i]}, model {want[i]}")
        comp = self.composed(ts, tile)
        assert np.array_equal(got, comp), f"{what}: {np.count_nonzero(got != comp)} bytes differ from the composition on the device"
        return maps

    def close(self):
        self.c.close()
        for b in self.bufs + self.out + list(self.maps.values()):
            b.free()


# (H, W, res values, in stride, out stride, by reference, tiles).  res halves the frame height rs times: rs = 0, 1, 2, 3 each.
GEOMETRIES = {
    # W no multiple of 16 or of a tile, W bytes no dword multiple in SDR (element loads, not dword ones), last tile row and column
    # partial, 25 chroma rows; an output stride of its own
    "86x50": (50, 86, (50, 25, 13, 7), 0, 96, False, TILES),
    "96x64": (64, 96, (64, 32, 16, 8), 0, 0, False, TILES),
    "200x120-stride208-ref": (120, 200, (120, 60, 30, 15), 208, 0, True, (16, 64)),
    "40x36-one-tile": (36, 40, (36, 18, 9, 5), 0, 0, False, (64,)),
}


def run_geometry(name, hdr, kinds=("zero", "far+", "far-", "odd", "random"), rss=(0, 1, 2, 3), ts=T5):
    H, W, res, si, so, by_ref, tiles = GEOMETRIES[name]
    for rs in rss:
        r = Rig(hdr, H, W, res[rs], si, so, by_ref, seed=17 + rs + 4 * hdr)
        try:
            assert r.c.m_opticalFlowResScalar == rs
            fl = flows(r.g, r.rng)
            for kind in kinds:
                for tile in tiles:
                    m = r.check(fl[kind], ts, tile, (name, hdr, rs, kind, tile))
                    if kind == "random":
                        assert all(np.count_nonzero(m["sse"][k][p]) for k in range(len(ts)) for p in range(3))
        finally:
            r.close()


@pytest.mark.parametrize("hdr", [False, True], ids=["sdr", "hdr"])
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_geometries_flows_tiles_and_resolution_scalars(native_lib, name, hdr):
    """Every geometry at rs 0 .. 3, every flow, every tile, t = 0, .3996, .5, .998 and 1 in one launch.  96 x 64 and 200 x 120 at
    tile 16 have four and eight bands of tile rows (blockIdx.y) and, at 200 wide with tile 64, two strips (blockIdx.x)."""
    run_geometry(name, hdr)


@pytest.mark.parametrize("hdr", [False, True], ids=["sdr", "hdr"])
@pytest.mark.parametrize("n", [1, 24])
def test_outputs_per_launch(native_lib, hdr, n):
    """n_t = 1, and n_t = 24: THE case in which the kernel's loop over chunks of six outputs runs more than one trip (four), each chunk's
    maps in their place in the one buffer.  (Its other loop, over a workgroup's items: 384 or 768 items for 256 lanes -- two or three
    trips -- but for 8-bit frames with 16-byte items, 192 at tile 16, which is one trip.)"""
    r = Rig(hdr, 50, 86, 25, seed=5 + hdr)
    try:
        fl = flows(r.g, r.rng)
        ts = T24[:n] if n > 1 else [0.3996]
        m = r.check(fl["random"], ts, 16, ("n_t", n))
        assert m.shape[0] == n
        if n > 1:
            assert len({m[k].tobytes() for k in range(n)}) > n // 2   # (distinct maps, so a map in the wrong place shows)
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
        m = r.check(flow, T5, 16, "chain")
        assert np.count_nonzero(m["sse"][2][0])
    finally:
        r.close()


def test_a_saturated_tile_needs_more_than_32_bits(native_lib):
    """64 x 64 HDR, frame N-2 all 0 against frame N-1 all 65535: at tile 64 the luma entry is 4096 x 65535^2 = 1.76e13."""
    H = W = 64
    g = _geom(True, H, W)
    n = H * W * 3 // 2
    r = Rig(True, H, W, frames=[np.zeros(n, np.uint16), np.full(n, 65535, np.uint16), np.zeros(n, np.uint16)])
    try:
        for tile in TILES:
            m = r.check(np.zeros((2, g.lh, g.lw), np.int16), [0.5], tile, ("saturated", tile))[0]
            cnt = tile * tile
            assert (m["sse"][0] == cnt * 65535 ** 2).all() and (m["sad"][0] == cnt * 65535).all() and (m["max_abs"] == 65535).all()
            assert (m["sse"][1:] == cnt // 4 * 65535 ** 2).all()
        assert 4096 * 65535 ** 2 > 1 << 43
    finally:
        r.close()


def test_refusals_enqueue_nothing(native_lib):
    """Every refusal is HF_ERR_INVALID_ARGUMENT and leaves the sentinel-filled buffer as it was."""
    from hopperrender_amd import capi
    r = Rig(False, 50, 86, 25)
    L = capi.load()
    try:
        nbytes = r.shape(16)[2]
        buf = r._buf(24 * nbytes)
        fl = lambda *v: (C.c_float * len(v))(*v)
        enq = lambda n, t, tile, maps: L.hf_warp_disagreement_map_enqueue(r.c._ctx, n, t, tile, C.c_void_p(maps))
        ok5 = fl(*T5)
        bad = {f"tile {t}": enq(5, ok5, t, buf.ptr) for t in (0, -16, 8, 17, 48, 128)}
        bad.update({
            "null t": enq(5, None, 16, buf.ptr), "n = 0": enq(0, ok5, 16, buf.ptr), "n < 0": enq(-1, ok5, 16, buf.ptr),
            "n = 25": enq(25, fl(*([0.5] * 25)), 16, buf.ptr),
            "t above 1": enq(3, fl(0.5, 1.0001, 0.2), 16, buf.ptr), "last t above 1": enq(24, fl(*([0.5] * 23 + [2.0])), 16, buf.ptr),
            "null maps": enq(5, ok5, 16, None), "maps 8 bytes in": enq(5, ok5, 16, buf.ptr + 8), "maps 4 bytes in": enq(5, ok5, 16, buf.ptr + 4),
            "null context": L.hf_warp_disagreement_map_enqueue(None, 5, ok5, 16, C.c_void_p(buf.ptr)),
        })
        assert {k: v for k, v in bad.items() if v != INVALID} == {}
        assert b"hf_warp_disagreement_map_enqueue" in L.hf_last_error(r.c._ctx)
        r.c.sync()
        assert (buf.download(np.uint8) == 0xFF).all()
        with pytest.raises(capi.HopperFlowError) as e:
            r.c.warpDisagreementMapEnqueue([0.5], 20, buf.ptr)
        assert e.value.code == INVALID
        assert enq(24, fl(*T24), 16, buf.ptr) == 0 and enq(1, fl(-0.25), 64, buf.ptr) == 0   # (a t below 0 is hf_warp_frames' to take, too)
        r.c.sync()
    finally:
        r.close()


@pytest.mark.parametrize("dual", [False, True], ids=["async", "dual-stream"])
def test_straight_behind_a_period_without_a_sync(native_lib, dual):
    """interpolatePeriod, then the call at once: equal to the composition made after a sync, on the frames and the flow that period's
    warps used; the output frame, m_warpCalcTime and the debug counters are as the period left them."""
    from hopperrender_amd import capi, synth
    from hopperrender_amd.calc import DeviceBuffer
    H, W, tile = 360, 640, 32
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
        r.c.interpolatePeriod(more[0].ptr, [0.5], [period_out.ptr])
        r.c.interpolatePeriod(more[1].ptr, [0.25, 0.5], [period_out.ptr, r.out[0].ptr])   # shows the pair (1, 2) with the flow of the period before
        got = r.device([0.25, 0.5], tile)                                                    # enqueued at once; the sync is behind it
        before = (r.c.downloadFrame().copy(), r.c.m_warpCalcTime, r.c.counters(), period_out.download(np.uint16))
        again = r.device([0.25, 0.5], tile)
        after = (r.c.downloadFrame().copy(), r.c.m_warpCalcTime, r.c.counters(), period_out.download(np.uint16))
        assert np.array_equal(before[0], after[0]) and before[1] == after[1] and before[2] == after[2] and np.array_equal(before[3], after[3])
        comp = r.composed([0.25, 0.5], tile)
        assert np.array_equal(got, comp) and np.array_equal(again, comp)
        flow = r.c.readBlurredFlow(0)
        want = wdm.warp_disagreement_maps(f[1], f[2], flow, r.g, [np.float32(0.25), np.float32(0.5)], tile)
        assert np.array_equal(r.view(got, 2, tile), want) and np.count_nonzero(want["sse"][1][0])
    finally:
        r.close()
        for b in more + [period_out]:
            b.free()


def test_the_next_asynchronous_upload_waits_for_the_launch(native_lib):
    """Asynchronous host input: the H2D of the next frame lands in the slot of frame N-2, which the launch reads.  Frames 0 .. 3 go in by
    updateFrameAsync, a chain is enqueued, the call behind it, and at once the upload of frame 4 -- the inverse of frame 1, whose slot
    it takes.  The maps must be those of frames 1 and 2: the model's, and the composition's on a second context fed the same frames
    synchronously."""
    from hopperrender_amd import capi, synth
    from hopperrender_amd.calc import PinnedArray
    H, W, tile, ts = 1080, 1920, 32, [0.3996, 0.7992]
    sc = synth.Scene(H, W, True, 9)
    f = [sc.frame(k) for k in range(4)]
    f.append((65535 - f[1]).astype(np.uint16))
    c = _cls(True)(H, W, search_radius=16, flags=capi.HF_FLAG_ASYNC)
    pins = []
    for x in f:
        pins.append(PinnedArray(x.size, x.dtype))
        pins[-1].array[:] = x
    twin = Rig(True, H, W, frames=f[1:4])
    try:
        for k in range(4):
            c.updateFrameAsync(pins[k])
            if k >= 1:
                c.calculateOpticalFlow()           # the last one is still queued when the call below is made
        nbytes = c.frameErrorMapShape(tile)[2] * len(ts)
        buf = twin._buf(nbytes)
        c.warpDisagreementMapEnqueue(ts, tile, buf.ptr)   # frames 1 and 2, the flow of (1, 2)
        c.updateFrameAsync(pins[4])
        c.sync()
        got = buf.download(np.uint8)[:nbytes].copy()
        flow = c.readBlurredFlow(0)
        want = wdm.warp_disagreement_maps(f[1], f[2], flow, twin.g, [np.float32(t) for t in ts], tile)
        assert np.array_equal(twin.view(got, len(ts), tile), want) and np.count_nonzero(want["sse"][0][0])
        twin.c.sync()
        twin.c.writeBlurredFlow(0, flow)
        assert np.array_equal(got, twin.composed(ts, tile))
    finally:
        c.close()
        twin.close()
        for p in pins:
            p.free()


def test_members_of_a_batch(native_lib):
    """Two members behind hf_batch_run_period: each member's maps equal the composition through hf_batch_interpolate_period with modes 0
    and 1 (the frames and the flow that period's warps used)."""
    from hopperrender_amd import capi, synth
    from hopperrender_amd.calc import DeviceBuffer, FlowBatch, frame_error_maps
    H, W, tile, ts = 180, 320, 16, [0.3996, 0.7992]
    scs = [synth.Scene(H, W, False, 31 + i) for i in range(2)]
    fr = [[sc.frame(k) for k in range(4)] for sc in scs]
    ms = [_cls(False)(H, W, search_radius=8, flags=capi.HF_FLAG_ASYNC) for _ in range(2)]
    dev = [[DeviceBuffer(x.nbytes) for x in f] for f in fr]
    for bs, f in zip(dev, fr):
        for b, x in zip(bs, f):
            b.upload(x)
    outs = [[DeviceBuffer(ms[0].output_frame_bytes) for _ in range(4)] for _ in range(2)]
    tw, th, nbytes = ms[0].frameErrorMapShape(tile)
    maps = [DeviceBuffer(2 * nbytes) for _ in range(4)]
    batch = FlowBatch(ms)
    try:
        for k in range(4):
            batch.runPeriod(batch.preparePeriod([dev[i][k].ptr for i in range(2)], [ts] * 2, [[o.ptr for o in outs[i][:2]] for i in range(2)], 2))
        for i, m in enumerate(ms):   # straight behind the period, no sync
            m.warpDisagreementMapEnqueue(ts, tile, maps[i].ptr)
        batch.sync()
        for mode in (0, 1):
            batch.interpolatePeriod([ts] * 2, [[o.ptr for o in outs[i][2 * mode:2 * mode + 2]] for i in range(2)], mode)
        for i, m in enumerate(ms):
            m.frameErrorMapEnqueue([o.ptr for o in outs[i][:2]], [o.ptr for o in outs[i][2:]], tile, maps[2 + i].ptr)
        batch.sync()
        for i in range(2):
            got, comp = maps[i].download(np.uint8), maps[2 + i].download(np.uint8)
            assert np.array_equal(got, comp), i
            assert np.count_nonzero(frame_error_maps(got, 2, tw, th)["sse"][0][0])
        assert not np.array_equal(maps[0].download(np.uint8), maps[1].download(np.uint8))
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
import test_warp_disagreement_gpu as WD

def violations(c):
    n = C.c_uint32(0); first = (C.c_uint32 * 4)()
    capi.check(c._lib.hf_debug_bounds_violations(c._ctx, C.byref(n), first, 0), c._ctx)
    return n.value, list(first)

assert capi.is_debug_bounds_build()
probe = OpticalFlowCalcSDR(64, 96)
for hdr in (False, True):
    WD.run_geometry("86x50", hdr, kinds=("far+", "far-", "random"))          # the mirror flows at every edge, rs 0 .. 3
    assert violations(probe)[0] == 0, ("86x50", hdr, violations(probe))
    WD.run_geometry("200x120-stride208-ref", hdr, kinds=("odd", "random"), rss=(3,), ts=WD.T24)
    assert violations(probe)[0] == 0, ("200x120", hdr, violations(probe))
probe.close()
print("DISAGREEMENT-DEBUG-BOUNDS-OK")
"""


def test_subset_under_the_bounds_checking_build(native_lib):
    """The mirror flows at 86 x 50 and an rs = 3 case under -DHF_DEBUG_BOUNDS in a child process: zero violations, the same maps (the
    cases' own assertions against the model and the composition)."""
    from hopperrender_amd import build
    dbg = build.build_flow(debug_bounds=True)
    env = dict(os.environ, HF_LIB=dbg)
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT)], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0 and "DISAGREEMENT-DEBUG-BOUNDS-OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
