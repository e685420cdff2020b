"""GPU: hf_batch_run_period_auto(_wide) on a batch that defers its phase planes, under HF_FLAG_BATCH_AUTO_DEFERRED on the leader
(include/hopperflow.h).  The period keeps the deferred order -- grid samples at update time, the warps of chunk 0 ahead of the chain, where
they build the planes -- and only chunk 0's predicated copy and planar conversion wait for the decision (csrc/hf_launch_plan.h
plan_auto_period; tests/test_auto_period_plan.py holds the plan).  The yardstick is the same library's HF_FLAG_BATCH_EAGER_PLANES twin, which
runs the order the auto call has always had: everything a host can observe is compared after every period, byte for byte.

Three 2160 x 3840 HDR members are the smallest batch that defers.  Seven frames of one synthetic scene, A0 .. A6, are generated once per
module; F0 .. F6 are the same frames upside down (Y and UV rows reversed: another picture with motion of its own, so A -> F is a hard cut).
(This file sorts behind tests/test_timeline_gpu.py, which has to stay the first of the suite to switch a timeline on: see
tests/test_chain_host_path_gpu.py.)"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H, W, RADIUS, SOURCE_24 = 2160, 3840, 8, 417083
N_FRAMES = 7
CHAIN_NAMES = {"large_windows_x", "large_windows_y", "large_windows_argmin", "level_32", "level_16", "level_8", "level_4", "level_2", "blur"}

_dev = {}


def _flip(f):
    a = f.reshape(H + H // 2, W)
    return np.ascontiguousarray(np.concatenate([a[:H][::-1], a[H:][::-1]])).reshape(-1)


def frames(planar=False):
    """{"A": [7 device buffers], "F": [7]}: P010 frames, or their yuv420p10le twins (tests/planar_ref.py).  Made once, never modified."""
    from hopperrender_amd import synth
    from hopperrender_amd.calc import DeviceBuffer
    import planar_ref
    if "host" not in _dev:
        sc = synth.Scene(H, W, True, 42)
        a = [sc.frame(k) for k in range(N_FRAMES)]
        _dev["host"] = {"A": a, "F": [_flip(f) for f in a]}
    key = "planar" if planar else "p010"
    if key not in _dev:
        _dev[key] = {}
        for name, fs in _dev["host"].items():
            _dev[key][name] = []
            for f in fs:
                b = DeviceBuffer(f.nbytes)
                b.upload(planar_ref.semiplanar_to_planar(f, H, W, W, True) if planar else f)
                _dev[key][name].append(b)
    return _dev[key]


@pytest.fixture(scope="module", autouse=True)
def _free_the_frames():
    yield
    for key in ("planar", "p010"):
        for row in _dev.pop(key, {}).values():
            for b in row:
                b.free()
    _dev.clear()


def clips(fr):
    """Member 0: cut at frame 5; member 1: cut at frame 4; member 2: no cut.  The delta of a cut at frame c is pushed in period c (0-based;
    m_frameCount c + 1) and decided on one period later (the decision needs the delta that follows it), so the copy periods are 6 and 5.
    (An earlier cut cannot be found in a clip that starts here: the average the spike is held against needs a delta from before it,
    and the first one is pushed in period 2.)"""
    A, F = fr["A"], fr["F"]
    return [A[:5] + F[5:7], F[:4] + A[4:7], F[:7]]


def scalars(n):
    return [(i + 1) / (n + 1) for i in range(n)]


class Side:
    """One batch of 2160p HDR members and its caller-owned output buffers (reused from period to period: consecutive periods show
    different frames, so a launch that did not write would leave the previous period's bytes and differ from the twin)."""

    def __init__(self, leader_flags, n=3, max_out=(5, 5, 5), marker=None):
        from hopperrender_amd import capi
        from hopperrender_amd.calc import DeviceBuffer, FlowBatch, OpticalFlowCalcHDR
        self.members = [OpticalFlowCalcHDR(H, W, search_radius=RADIUS, flags=capi.HF_FLAG_ASYNC | (leader_flags if i == 0 else 0)) for i in range(n)]
        self.batch = FlowBatch(self.members)
        self.n, self.nbytes = n, self.members[0].output_frame_bytes
        self.bufs = [[DeviceBuffer(self.nbytes) for _ in range(max_out[m % len(max_out)])] for m in range(n)]
        if marker is not None:
            self.mark(marker)
        for m in range(n):
            self.batch.sceneSet(m, SOURCE_24, 200)

    def mark(self, value):
        fill = np.full(self.nbytes, value, np.uint8)
        for row in self.bufs:
            for b in row:
                b.upload(fill)

    def period(self, ptrs, n_out, mode=2, force=None, null=()):
        outs = [[0 if (m, i) in null else self.bufs[m][i].ptr for i in range(n_out[m])] for m in range(self.n)]
        self.batch.runPeriodAuto(ptrs, [scalars(k) for k in n_out], outs, mode, force)

    def read(self, m, i, into):
        from hopperrender_amd import capi
        capi.check(self.batch._lib.hf_memcpy_d2h(0, into.ctypes.data_as(C.c_void_p), C.c_void_p(self.bufs[m][i].ptr), into.nbytes))
        return into

    def close(self):
        self.batch.close()
        for c in self.members:
            c.close()
        for row in self.bufs:
            for b in row:
                b.free()


class Twins:
    """The flagged batch and its HF_FLAG_BATCH_EAGER_PLANES twin, fed the same periods."""

    def __init__(self, extra=0, **kw):
        from hopperrender_amd import capi
        self.f = Side(capi.HF_FLAG_BATCH_AUTO_DEFERRED | extra, **kw)
        try:
            self.t = Side(capi.HF_FLAG_BATCH_EAGER_PLANES | extra, **kw)
        except Exception:
            self.f.close()
            raise
        assert self.f.batch.defersPlanes() and not self.t.batch.defersPlanes()
        self.a, self.b = np.empty(self.f.nbytes, np.uint8), np.empty(self.f.nbytes, np.uint8)
        self.records = [[] for _ in range(self.f.n)]

    def period(self, ptrs, n_out, what, members=None, **kw):
        self.f.period(ptrs, n_out, **kw)
        self.t.period(ptrs, n_out, **kw)
        self.compare(n_out, what, members, null=kw.get("null", ()))

    def compare(self, n_out, what, members=None, null=(), records=1):
        """Everything a host can observe of the two batches, after a sync of both."""
        self.f.batch.sync(); self.t.batch.sync()
        for m in (range(self.f.n) if members is None else members):
            p, q = self.f.members[m], self.t.members[m]
            for i in range(n_out[m]):
                if (m, i) in null:
                    assert np.array_equal(p.downloadFrame(), q.downloadFrame()), f"{what}: member {m}: the internal output frame differs"
                else:
                    assert np.array_equal(self.f.read(m, i, self.a), self.t.read(m, i, self.b)), f"{what}: member {m} output {i} differs"
            rp, rq = self.f.batch.sceneRead(m), self.t.batch.sceneRead(m)
            assert rp == rq and len(rp) == records, (what, m, rp, rq)
            self.records[m] += rp
            assert p.m_frameCount == q.m_frameCount and p.m_totalFrameDelta == q.m_totalFrameDelta, (what, m)
            for idx in (0, 1):
                assert np.array_equal(p.readBlurredFlow(idx), q.readBlurredFlow(idx)), f"{what}: member {m}: blurred flow {idx} differs"
            sp, sq = p.stats(), q.stats()
            assert (sp["iterations"], sp["initial_window"]) == (sq["iterations"], sq["initial_window"]), (what, m)
            if sp["iterations"]:
                assert np.array_equal(p.readOffsets(), q.readOffsets()), f"{what}: member {m}: hf_read_offsets differs"
            (pa, ca), (pb, cb) = p.readPhasePlane(1), q.readPhasePlane(1)
            assert ca and cb, f"{what}: member {m}: the older frame's plane is incomplete behind a chain"
            assert np.array_equal(pa, pb), f"{what}: member {m}: phase plane 1 differs"

    def deferral_was_taken(self, what):
        """The witness: the newest frame of the flagged batch has only its grid samples, the twin's has its full plane."""
        assert not self.f.members[0].readPhasePlane(2)[1], what
        assert self.t.members[0].readPhasePlane(2)[1], what

    def close(self):
        self.f.close(); self.t.close()


# 1. -- fails without the feature: HF_ERR_STATE ("defers its phase planes") on the first period
def test_whole_clips_from_the_first_frame(native_lib):
    """Seven periods from m_frameCount 0: periods 0 and 1 are warm-up rides (period 1 already goes early: the plane of frame 0 is pending),
    members 0 and 1 have their cut in different periods, member 2 has none; period 4 forces a warp on member 0 and a copy on member 2.
    Members take 5, 4 and 5 outputs."""
    cl = clips(frames())
    tw = Twins()
    try:
        n_out = (5, 4, 5)
        for k in range(N_FRAMES):
            tw.period([c[k].ptr for c in cl], n_out, f"period {k}", force=[1, -1, 0] if k == 4 else None)
            tw.deferral_was_taken(f"period {k}")
        kinds = [[r["kind"] for r in rs] for rs in tw.records]
        print("records:", tw.records)
        assert all([r["frame_count"] for r in rs] == list(range(1, N_FRAMES + 1)) for rs in tw.records)
        # warm-up copies, then warps; cuts the device decided on (not forced, not a warm-up period) in period 6 for member 0 and in period 5
        # for member 1; the copy forced on cut-free member 2 in period 4
        assert kinds == [[0, 0, 1, 1, 1, 1, 0], [0, 0, 1, 1, 1, 0, 1], [0, 0, 1, 1, 0, 1, 1]], kinds
    finally:
        tw.close()


# 2. -- fails without the feature
def test_wide_planar_periods(native_lib):
    """HF_FLAG_BATCH_PLANAR_IN | _OUT, row 13 with 13 / 7 / 6 outputs (three chunks) in periods 1 (warm-up ride), 4 and 5 (member 1's cut
    period): chunk 0's conversion has to follow its copy, which follows the decision.  Output 12 of member 0 and output 0 of member 1 are
    NULL entries (the internal frame, which stays P010)."""
    from hopperrender_amd import capi
    cl = clips(frames(planar=True))
    wide, narrow = (13, 7, 6), (2, 2, 2)
    tw = Twins(capi.HF_FLAG_BATCH_PLANAR_IN | capi.HF_FLAG_BATCH_PLANAR_OUT, max_out=wide)
    try:
        assert tw.f.batch.planar() == (True, True) and tw.t.batch.planar() == (True, True)
        for k in range(6):
            n_out = wide if k in (1, 4, 5) else narrow
            tw.period([c[k].ptr for c in cl], n_out, f"period {k}", null={(0, 12), (1, 0)})
        tw.deferral_was_taken("period 5")
        kinds = [[r["kind"] for r in rs] for rs in tw.records]
        print("records:", tw.records)
        assert kinds == [[0, 0, 1, 1, 1, 1], [0, 0, 1, 1, 1, 0], [0, 0, 1, 1, 1, 1]], kinds
    finally:
        tw.close()


# 3.
def test_periods_that_cannot_go_early(native_lib):
    """A member without outputs (period 3) and a diagnostic mode (period 4): the period takes the order it always had and the chain's
    stand-alone plane launch fills in.  A separate hf_batch_calculate_optical_flow between two periods (ahead of period 5: the flow buffers
    swap once more).  Each equals the twin, and so do the periods behind it."""
    cl = clips(frames())
    tw = Twins(max_out=(2, 2, 2))
    try:
        for k in range(N_FRAMES):
            n_out, mode = ((2, 0, 2) if k == 3 else (2, 2, 2)), (3 if k == 4 else 2)
            if k == 5:
                tw.f.batch.calculateOpticalFlow(); tw.t.batch.calculateOpticalFlow()
            tw.period([c[k].ptr for c in cl], n_out, f"period {k}", mode=mode)
            tw.deferral_was_taken(f"period {k}")
    finally:
        tw.close()


# 4. -- fails without the feature
def test_launch_order_on_the_timeline(native_lib):
    """The period of frame 3 on each batch's own timeline, kernel names in order.  Flagged: grid samples, the fused period warp AHEAD of the
    chain's first launch, the chain, scene_decide, scene_copy -- and no stand-alone plane launch.  Twin: the plane launch, the chain,
    scene_decide, the warp, scene_copy.  The names are the ones the library's launches have always carried (tests/test_warp_host_path_gpu.py)."""
    cl = clips(frames())
    tw = Twins(max_out=(2, 2, 2))
    try:
        for k in range(3):
            tw.period([c[k].ptr for c in cl], (2, 2, 2), f"period {k}")
        names = []
        for side in (tw.f, tw.t):
            side.batch.timelineEnable(256)
            side.period([c[3].ptr for c in cl], (2, 2, 2))
            names.append([r[0] for r in side.batch.timelineRead() if r[1] == 0])
            side.batch.timelineEnable(0)
        tw.compare((2, 2, 2), "period 3")
        flagged, twin = names
        print("flagged:", flagged, "twin:", twin)
        chain = twin[1:-3]
        assert chain and set(chain) <= CHAIN_NAMES and chain[-1] == "blur", twin
        assert twin == ["plane"] + chain + ["scene_decide", "warp_period", "scene_copy"]
        assert flagged == ["grid_samples", "warp_period"] + chain + ["scene_decide", "scene_copy"]
    finally:
        tw.close()


# 5.
def test_errors_and_refusals(native_lib):
    from hopperrender_amd import capi
    cl = clips(frames())
    tw = Twins(max_out=(2, 2, 2))
    try:
        for k in range(3):
            tw.period([c[k].ptr for c in cl], (2, 2, 2), f"period {k}")
        # a blending scalar above 1 for member 1: refused where the twin refuses it, before anything is enqueued
        errors = []
        for side in (tw.f, tw.t):
            outs = [[b.ptr for b in row] for row in side.bufs]
            with pytest.raises(capi.HopperFlowError) as e:
                side.batch.runPeriodAuto([c[3].ptr for c in cl], [[0.25, 0.75], [0.25, 1.5], [0.25, 0.75]], outs, 2)
            errors.append((e.value.code, str(e.value)))
        assert errors[0] == errors[1] and errors[0][0] == capi.HF_ERR_INVALID_ARGUMENT and "blending scalar" in errors[0][1], errors
        tw.compare((0, 0, 0), "after the refused scalar", records=0)
        tw.period([c[3].ptr for c in cl], (2, 2, 2), "period 3")
        # members that differ in search radius: the chain's own check, ahead of the early warps -- no output buffer is written
        tw.f.mark(0xA5)
        tw.f.members[1].m_opticalFlowSearchRadius = 4
        with pytest.raises(capi.HopperFlowError) as e:
            tw.f.period([c[4].ptr for c in cl], (2, 2, 2))
        assert e.value.code == capi.HF_ERR_INVALID_ARGUMENT and "members differ in search radius" in str(e.value), str(e.value)
        tw.f.batch.sync()
        for m in range(3):
            for i in range(2):
                assert (tw.f.read(m, i, tw.a) == 0xA5).all(), f"member {m} output {i} was written by a refused period"
        tw.f.members[1].m_opticalFlowSearchRadius = RADIUS
        tw.period([c[4].ptr for c in cl], (2, 2, 2), "period 4")
        tw.deferral_was_taken("period 4")
    finally:
        tw.close()
    # without the flag: the documented refusal of ABI 6, word for word
    plain = Side(0, max_out=(2, 2, 2))
    try:
        assert plain.batch.defersPlanes()
        with pytest.raises(capi.HopperFlowError) as e:
            plain.period([c[0].ptr for c in cl], (2, 2, 2))
        assert e.value.code == capi.HF_ERR_STATE
        assert str(e.value).endswith("hf_batch_run_period_auto: this batch defers its phase planes, so a period's warps are issued ahead of its chain and the "
                                     "decision does not exist yet; create the leader with HF_FLAG_BATCH_EAGER_PLANES"), str(e.value)
        assert [c.m_frameCount for c in plain.members] == [0, 0, 0]
    finally:
        plain.close()


# 6. -- fails without the feature
def test_a_batch_of_17(native_lib):
    """17 members = a warp launch of 16 (the staged kernel, which builds the planes) and one of a single member (too small for the staged
    kernel: its plane comes from the chain's stand-alone launch).  Three periods; members 0, 15 and 16 are compared."""
    fr = frames()
    rows = [fr["A"], fr["F"]]
    tw = Twins(n=17, max_out=(2,))
    try:
        for k in range(3):
            tw.period([rows[m % 2][(k + m) % N_FRAMES].ptr for m in range(17)], (2,) * 17, f"period {k}", members=(0, 15, 16))
        tw.deferral_was_taken("period 2")
    finally:
        tw.close()
