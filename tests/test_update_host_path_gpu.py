"""GPU: the one host path of a frame update (csrc/hf_calc.hip update_frames) where no other test holds it: every entry point -- host,
device, device reference, asynchronous, a batch of 1, a batch of 3 -- builds the same phase planes, with and without planar input; a refused
batch update leaves every member as it was; deferred and eager updates of one batch interleave; dual-stream contexts are updated directly
behind the warps that left them on their warp streams; a batch's update is one re-layout and one plane launch.  The yardstick is a plain
blocking context fed the same frames with updateFrame, bit for bit: the three phase planes with their `complete` flags after every update,
the newest blurred flow and m_totalFrameDelta after every chain.

180 x 320 SDR and 360 x 640 HDR (the shapes of tests/test_chain_host_path_gpu.py), 180 x 322 SDR, whose grid width is no multiple of 4 (its
planar frames take the element-by-element re-layout), and for the deferred planes 2160 x 3840 HDR in a batch of 4, the smallest shape of
tests/test_deferred_planes_gpu.py that defers.  Of these only 360 x 640 HDR takes the fast plane kernel (rs 1, lw 320, mx 296); 180 x 320
SDR runs at rs 0 with a margin of mx = 588 > lw = 320 columns, beyond the single reflection, so the generic kernel builds its planes as it
does those of 180 x 322 (tests/plane_builder_model.py builder, which tests/test_plane_builders_model.py holds to the compiled decision).
This file compares twins; the fast kernel on 8-bit frames is held to the layout model by tests/test_plane_builders_gpu.py.  (This file sorts behind
tests/test_timeline_gpu.py, which has to stay the first of the suite to switch a timeline on: see tests/test_chain_host_path_gpu.py.)"""
import numpy as np
import pytest

import planar_ref

pytestmark = pytest.mark.gpu

RADIUS = 8
SDR = (0, 180, 320)          # hdr, H, W
HDR = (1, 360, 640)
GENERIC = (0, 180, 322)
UHD = (1, 2160, 3840)
SEEDS = (42, 7, 23)
N_FRAMES = 6                 # the ring of three wraps twice
TS = (0.25, 0.75)            # the outputs of the period of frame 3
WARP_AT = 3

_frames, _plain = {}, {}


def make(case, flags=0):
    from hopperrender_amd.calc import OpticalFlowCalcHDR, OpticalFlowCalcSDR
    return (OpticalFlowCalcHDR if case[0] else OpticalFlowCalcSDR)(case[1], case[2], search_radius=RADIUS, flags=flags)


def frames(case, seed):
    """(planar frames, their NV12 / P010 twins): the twin is what the device makes of the planar frame, so one yardstick serves both."""
    from hopperrender_amd import synth
    if (case, seed) not in _frames:
        hdr, H, W = case
        sc = synth.Scene(H, W, bool(hdr), seed)
        # (the large shape: three pictures shown in turn -- a synthetic 2160p picture takes a second to draw)
        shown = [k % 3 for k in range(5)] if case == UHD else range(N_FRAMES)
        drawn = {k: planar_ref.semiplanar_to_planar(sc.frame(k), H, W, W, hdr) for k in set(shown)}
        planar = [drawn[k] for k in shown]
        _frames[case, seed] = (planar, [planar_ref.planar_to_semiplanar(p, H, W, W, hdr) for p in planar])
    return _frames[case, seed]


def state(c):
    """the three phase planes of a context with their complete flags, and m_frameCount"""
    planes = [c.readPhasePlane(s) for s in range(3)]
    return dict(planes=[p for p, _ in planes], complete=[done for _, done in planes], count=c.m_frameCount)


def plain(case, seed):
    """A plain blocking context shown the twins with updateFrame, calculateOpticalFlow after every frame but the first: per frame its
    state, flow and delta, and the outputs of TS (mode 2) behind the chain of frame WARP_AT.  Computed once, shared, never modified."""
    if (case, seed) not in _plain:
        c = make(case)
        out = []
        for k, f in enumerate(frames(case, seed)[1]):
            c.updateFrame(f)
            rec = state(c)
            assert all(rec["complete"]) and rec["count"] == k + 1
            if k >= 1:
                c.calculateOpticalFlow()
                rec.update(flow=c.readBlurredFlow(1), delta=c.m_totalFrameDelta)
            if k == WARP_AT and case != UHD:
                rec["outs"] = []
                for t in TS:
                    c.warpFrames(t, 2)
                    rec["outs"].append(c.downloadFrame().copy())
            out.append(rec)
        c.close()
        assert out[1]["delta"] > 0 and out[2]["flow"].any() and not np.array_equal(out[-1]["planes"][2], out[-2]["planes"][2])
        _plain[case, seed] = out
    return _plain[case, seed]


def assert_state(c, want, what, complete=(True, True, True)):
    """planes are compared where they are complete; `complete` is what the flags must read"""
    got = state(c)
    assert got["count"] == want["count"], what
    assert tuple(got["complete"]) == tuple(complete), (what, got["complete"])
    for s in range(3):
        if complete[s]:
            assert np.array_equal(got["planes"][s], want["planes"][s]), (what, "slot", s)


def assert_chain(c, want, what):
    assert np.array_equal(c.readBlurredFlow(1), want["flow"]), what
    assert c.m_totalFrameDelta == want["delta"], what


class Clips:
    """The frames of (case, seed) for every seed, planar or not, in device buffers -- one per frame: a referenced frame stays in the ring
    for three updates."""

    def __init__(self, case, seeds, planar):
        from hopperrender_amd.calc import DeviceBuffer
        self.dev = []
        for s in seeds:
            row = []
            for f in frames(case, s)[0 if planar else 1]:
                b = DeviceBuffer(f.nbytes)
                b.upload(f)
                row.append(b)
            self.dev.append(row)

    def feed(self, k):
        return [row[k].ptr for row in self.dev]

    def free(self):
        for row in self.dev:
            for b in row:
                b.free()


def free_all(*things):
    for x in things:
        (x.close if hasattr(x, "close") else x.free)()


# 1.
ENTRIES = ["host", "device", "device-ref", "async", "batch-1", "batch-3"]


@pytest.mark.parametrize("planar", [False, True], ids=["semi-planar", "planar"])
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("case", [SDR, HDR, GENERIC], ids=["sdr", "hdr", "generic-plane"])
def test_every_entry_point_reaches_the_same_planes(native_lib, case, entry, planar):
    from hopperrender_amd import capi
    from hopperrender_amd.calc import FlowBatch, PinnedArray
    n = 3 if entry == "batch-3" else 1
    seeds = SEEDS[:n]
    batch, clips, pins = None, None, []
    if entry.startswith("batch"):
        members = [make(case, capi.HF_FLAG_ASYNC | (capi.HF_FLAG_BATCH_PLANAR_IN if planar and m == 0 else 0)) for m in range(n)]
        batch = FlowBatch(members)
        assert batch.planar() == (planar, False)
    else:
        members = [make(case, (capi.HF_FLAG_ASYNC if entry == "async" else 0) | (capi.HF_FLAG_PLANAR_IN if planar else 0))]
    c = members[0]
    rs = c.m_opticalFlowResScalar
    assert ((case[2] >> rs) & 3 != 0) == (case == GENERIC)      # one of the things hf_flow.hip launch_prep_fast declines (see above)
    host = frames(case, seeds[0])[0 if planar else 1]
    if entry == "async":
        for f in host:
            pins.append(PinnedArray(f.size, f.dtype))
            pins[-1].array[:] = f
    elif entry != "host":
        clips = Clips(case, seeds, planar)
    try:
        for k in range(N_FRAMES):
            if entry == "host":
                c.updateFrame(host[k])
            elif entry == "device":
                c.updateFrameDevice(clips.feed(k)[0])
            elif entry == "device-ref":
                c.updateFrameDeviceRef(clips.feed(k)[0])
            elif entry == "async":
                c.updateFrameAsync(pins[k])
            else:
                batch.updateFramesDeviceRef(clips.feed(k))
            for m, x in enumerate(members):
                assert_state(x, plain(case, seeds[m])[k], (entry, "frame", k, "member", m))
            if k >= 1:
                if batch:
                    batch.calculateOpticalFlow()
                    batch.sync()
                else:
                    c.calculateOpticalFlow()
                    c.sync()
                for m, x in enumerate(members):
                    assert_chain(x, plain(case, seeds[m])[k], (entry, "chain", k, "member", m))
    finally:
        free_all(*([batch] if batch else []), *members, *([clips] if clips else []), *pins)


# 2.
def test_a_refused_batch_update_leaves_every_member_as_it_was(native_lib):
    from hopperrender_amd import capi
    from hopperrender_amd.calc import FlowBatch
    case = SDR
    clips = Clips(case, SEEDS, False)
    members = [make(case, capi.HF_FLAG_ASYNC) for _ in SEEDS]
    batch = FlowBatch(members)
    try:
        for k in range(3):
            batch.updateFramesDeviceRef(clips.feed(k))
        batch.calculateOpticalFlow()
        batch.sync()
        before = [state(c) for c in members]
        for null_at in (0, 1, 2):
            ptrs = clips.feed(3)
            ptrs[null_at] = 0
            with pytest.raises(capi.HopperFlowError) as e:
                batch.updateFramesDeviceRef(ptrs)
            assert e.value.code == capi.HF_ERR_INVALID_ARGUMENT
            for m, c in enumerate(members):
                assert c.m_frameCount == 3
                assert_state(c, before[m], ("null at", null_at, "member", m))
        batch.updateFramesDeviceRef(clips.feed(3))
        batch.calculateOpticalFlow()
        batch.sync()
        for m, c in enumerate(members):
            assert_state(c, plain(case, SEEDS[m])[3], ("the valid update", m))
            assert_chain(c, plain(case, SEEDS[m])[3], ("the valid chain", m))
    finally:
        free_all(batch, *members, clips)


# 3.
def test_deferred_and_eager_updates_interleave(native_lib):
    """Frame 0 and frame 1 come deferred (hf_batch_run_period: the newest slot holds
    grid samples only), frame 2 eager (hf_batch_update_frames_device_ref), frame 3 and frame 4 deferred again.  A plane is complete once the
    next period's warp launch or chain has built it (frame 0's in the period of frame 1, frame 3's in the period of frame 4); frame 1's
    never is -- the eager update of frame 2 moved it out of the chain's reach -- and its slot reads incomplete until frame 4 takes it over."""
    from hopperrender_amd import capi
    from hopperrender_amd.calc import DeviceBuffer, FlowBatch
    case, n = UHD, 4
    clips = Clips(case, (42,), False)
    members = [make(case, capi.HF_FLAG_ASYNC) for _ in range(n)]
    batch = FlowBatch(members)
    outs = [[DeviceBuffer(c.output_frame_bytes) for _ in TS] for c in members]
    try:
        assert batch.defersPlanes()

        def feed(k):
            return clips.feed(k) * n

        def period(k, flow):
            batch.runPeriod(batch.preparePeriod(feed(k), [TS] * n if flow else None, [[b.ptr for b in o] for o in outs] if flow else None, 2, calculate_flow=flow))
            batch.sync()

        def check(k, complete, chain):
            for m in (0, 3):
                want = plain(case, 42)[k]
                assert_state(members[m], want, ("frame", k, "member", m), complete)
                if chain:
                    assert_chain(members[m], want, ("chain", k, "member", m))

        period(0, False)
        check(0, (True, True, False), False)      # deferred: the newest slot is not complete
        period(1, True)
        check(1, (True, True, False), True)       # frame 0's plane has been built, frame 1 came deferred
        batch.updateFramesDeviceRef(feed(2))
        batch.sync()
        check(2, (True, False, True), False)      # eager: the newest slot is complete at once; frame 1's still is not
        period(3, True)
        check(3, (False, True, False), True)
        period(4, True)
        check(4, (True, True, False), True)       # frame 3's plane has been built; frame 4 took over the slot frame 1's grid samples were in
    finally:
        free_all(batch, *members, clips, *[b for o in outs for b in o])


# 4.
def _assert_outputs(case, seed, read, what):
    want = plain(case, seed)[WARP_AT]["outs"]
    for i in range(len(TS)):
        assert np.array_equal(read(i), want[i]), (what, "output", i)


def test_a_dual_stream_batch_is_updated_behind_its_warps(native_lib):
    from hopperrender_amd import capi
    from hopperrender_amd.calc import DeviceBuffer, FlowBatch
    case, seeds = SDR, SEEDS[:2]
    clips = Clips(case, seeds, False)
    members = [make(case, capi.HF_FLAG_ASYNC | capi.HF_FLAG_DUAL_STREAM) for _ in seeds]
    batch = FlowBatch(members)
    outs = [[DeviceBuffer(c.output_frame_bytes) for _ in TS] for c in members]
    try:
        for k in range(WARP_AT):
            batch.updateFramesDeviceRef(clips.feed(k))
            if k >= 1:
                batch.calculateOpticalFlow()
        # the period of frame 3 leaves both members on the batch's warp streams; the update of frame 4 follows at once
        batch.runPeriod(batch.preparePeriod(clips.feed(WARP_AT), [TS] * 2, [[b.ptr for b in o] for o in outs], 2))
        batch.updateFramesDeviceRef(clips.feed(WARP_AT + 1))
        batch.sync()
        for m, c in enumerate(members):
            _assert_outputs(case, seeds[m], lambda i: outs[m][i].download(c.dtype), ("member", m))
            assert_state(c, plain(case, seeds[m])[WARP_AT + 1], ("member", m))
        batch.calculateOpticalFlow()
        batch.sync()
        for m, c in enumerate(members):
            assert_chain(c, plain(case, seeds[m])[WARP_AT + 1], ("member", m))
    finally:
        free_all(batch, *members, clips, *[b for o in outs for b in o])


def test_a_lone_dual_stream_context_is_updated_asynchronously_behind_its_warps(native_lib):
    """The H2D of frame 4 overwrites the slot of frame 1, which the warps of the period of frame 3 read."""
    from hopperrender_amd import capi
    from hopperrender_amd.calc import DeviceBuffer, PinnedArray
    case, seed = SDR, 42
    c = make(case, capi.HF_FLAG_ASYNC | capi.HF_FLAG_DUAL_STREAM)
    pins = []
    for f in frames(case, seed)[1]:
        pins.append(PinnedArray(f.size, f.dtype))
        pins[-1].array[:] = f
    outs = [DeviceBuffer(c.output_frame_bytes) for _ in TS]
    try:
        for k in range(WARP_AT + 1):
            c.updateFrameAsync(pins[k])
            if k >= 1:
                c.calculateOpticalFlow()
        c.interpolateOnly(TS, [b.ptr for b in outs], 2)
        c.updateFrameAsync(pins[WARP_AT + 1])
        c.sync()
        _assert_outputs(case, seed, lambda i: outs[i].download(c.dtype), "lone")
        assert_state(c, plain(case, seed)[WARP_AT + 1], "lone")
        c.calculateOpticalFlow()
        c.sync()
        assert_chain(c, plain(case, seed)[WARP_AT + 1], "lone")
    finally:
        free_all(c, *pins, *outs)


# 5.
def test_a_batch_update_is_one_re_layout_and_one_plane_launch(native_lib):
    from hopperrender_amd import capi
    from hopperrender_amd.calc import FlowBatch
    case = SDR
    clips = Clips(case, SEEDS, True)
    members = [make(case, capi.HF_FLAG_ASYNC | (capi.HF_FLAG_BATCH_PLANAR_IN if m == 0 else 0)) for m in range(3)]
    batch = FlowBatch(members)
    try:
        for k in range(2):
            batch.updateFramesDeviceRef(clips.feed(k))
        batch.timelineEnable(64)
        batch.runPeriod(batch.preparePeriod(clips.feed(2), None, None, 2))
        names = [r[0] for r in batch.timelineRead() if r[1] == 0]
        batch.timelineEnable(0)
        print("timeline:", names)
        assert names.count("planar_in_batch") == 1
        assert names.count("plane") + names.count("grid_samples") == 1
        assert names[names.index("planar_in_batch") + 1] in ("plane", "grid_samples")
        batch.sync()
        for m, c in enumerate(members):
            assert_state(c, plain(case, SEEDS[m])[2], ("member", m))
            assert_chain(c, plain(case, SEEDS[m])[2], ("member", m))
    finally:
        free_all(batch, *members, clips)
