"""GPU: the one host path of a source period's warps (csrc/hf_calc.hip interpolate_period) where no other test holds it: a lone planar-out
context beyond six outputs (its stages are reused chunk by chunk), a lone period whose middle chunk alone falls back to one launch per
output, a refused period that has already updated and calculated, ragged wide batches whose chunks go fused or member by member, dual-stream
members on the batch's shared warp streams -- and the kernel names a batch's period puts on its timeline, in order.  The yardstick is a plain
blocking context fed the same frames, one warpFrames per output, byte for byte; planar sides through tests/planar_ref.py.

180 x 320 SDR and 360 x 640 HDR, the small shapes of the period tests, both with a half-resolution flow grid (maxCalcRes 135 for the SDR
shape: at the default 270 its grid is full resolution, where no fused launch applies and every output is a launch of the generic kernel):
they reach the fused launch, the per-output launch and every chunk boundary.  (This file sorts behind tests/test_timeline_gpu.py, which has to stay the first of the suite to switch a timeline on: see
tests/test_chain_host_path_gpu.py.)"""
import numpy as np
import pytest

import planar_ref

pytestmark = pytest.mark.gpu

RADIUS = 8
SDR = (0, 180, 320, 135)     # hdr, H, W, maxCalcRes
HDR = (1, 360, 640, 270)
TS = [(i + 1) / 14 for i in range(13)]      # 13 outputs: chunks of 6 + 6 + 1; a member of fewer outputs takes the first of them

_frames, _plain = {}, {}


def make(case, flags=0):
    from hopperrender_amd.calc import OpticalFlowCalcHDR, OpticalFlowCalcSDR
    c = (OpticalFlowCalcHDR if case[0] else OpticalFlowCalcSDR)(case[1], case[2], maxCalcRes=case[3], search_radius=RADIUS, flags=flags)
    assert c.m_opticalFlowResScalar == 1
    return c


def frames(case, seed):
    from hopperrender_amd import synth
    if (case, seed) not in _frames:
        sc = synth.Scene(case[1], case[2], bool(case[0]), seed)
        _frames[case, seed] = [sc.frame(k) for k in range(4)]
    return _frames[case, seed]


def plain(case, seed, mode):
    """A plain blocking context shown frames 0 .. 3 (a flow after the third and after the fourth): its newest blurred flow, and one
    warpFrames + downloadFrame per scalar of TS in `mode`.  Computed once, shared, never modified."""
    if (case, seed, mode) not in _plain:
        c = make(case)
        f = frames(case, seed)
        for x in f[:3]:
            c.updateFrame(x)
        c.calculateOpticalFlow()
        c.updateFrame(f[3])
        c.calculateOpticalFlow()
        outs = []
        for t in TS:
            c.warpFrames(t, mode)
            outs.append(c.downloadFrame().copy())
        _plain[case, seed, mode] = dict(outs=outs, flow=c.readBlurredFlow(1).copy(), stride=c.m_outputStride)
        c.close()
        assert mode != 2 or (not np.array_equal(outs[0], outs[7]) and not np.array_equal(outs[5], outs[6]))
    return _plain[case, seed, mode]


class Clip:
    """The four frames of (case, seed) in device buffers."""

    def __init__(self, case, seed):
        from hopperrender_amd.calc import DeviceBuffer
        self.bufs = []
        for f in frames(case, seed):
            b = DeviceBuffer(f.nbytes)
            b.upload(f)
            self.bufs.append(b)

    def prime(self, c):
        """frames 0 .. 2 and the flow of the third: the state in which the period of frame 3 is issued"""
        for b in self.bufs[:3]:
            c.updateFrameDeviceRef(b.ptr)
        c.calculateOpticalFlow()

    def free(self):
        for b in self.bufs:
            b.free()


class Outputs:
    """n output buffers of a context; `off` {index: bytes}: that output starts so many bytes into its (larger) buffer."""

    def __init__(self, c, n, off=None):
        from hopperrender_amd.calc import DeviceBuffer
        self.c, self.off = c, off or {}
        self.bufs = [DeviceBuffer(c.output_frame_bytes + 16) for _ in range(n)]
        self.ptrs = [b.ptr + self.off.get(i, 0) for i, b in enumerate(self.bufs)]

    def read(self, i):
        o = self.off.get(i, 0)
        return self.bufs[i].download(np.uint8)[o:o + self.c.output_frame_bytes].view(self.c.dtype)

    def free(self):
        for b in self.bufs:
            b.free()


def assert_planar(case, got, want_semiplanar, stride, what):
    hdr, H, W = case[:3]
    want = planar_ref.semiplanar_to_planar(want_semiplanar, H, W, stride, bool(hdr))
    for g, w in zip(planar_ref.planar_planes(got, H, W, stride), planar_ref.planar_planes(want, H, W, stride)):
        assert np.array_equal(g, w), what


# 1. -- the case whose stage policy changed: six stages, one conversion launch per chunk
@pytest.mark.parametrize("case", [SDR, HDR], ids=["sdr", "hdr"])
def test_lone_planar_out_context_of_13_outputs(native_lib, case):
    from hopperrender_amd import capi
    from hopperrender_amd.calc import DeviceBuffer
    want = plain(case, 42, 2)
    clip = Clip(case, 42)
    c = make(case, capi.HF_FLAG_ASYNC | capi.HF_FLAG_PLANAR_OUT)
    outs = Outputs(c, 13)
    last = DeviceBuffer(c.output_frame_bytes)
    try:
        assert c.m_outputStride == want["stride"]
        clip.prime(c)
        c.interpolatePeriod(clip.bufs[3].ptr, TS, outs.ptrs[:12] + [0], 2)      # the last entry NULL: the internal output frame
        c.downloadFrameDevice(last.ptr)
        c.sync()
        for i in range(12):
            assert_planar(case, outs.read(i), want["outs"][i], want["stride"], f"output {i}")
        assert_planar(case, last.download(c.dtype), want["outs"][12], want["stride"], "the internal frame")
        assert np.array_equal(c.readBlurredFlow(1), want["flow"])
    finally:
        c.close()
        outs.free(); last.free(); clip.free()


# 2.
@pytest.mark.parametrize("case", [SDR, HDR], ids=["sdr", "hdr"])
def test_lone_period_whose_middle_chunk_is_not_eligible(native_lib, case):
    """Output 8 only element-aligned: chunk 1 goes out as six launches of one output, chunks 0 and 2 as one launch each -- 8 launches of
    13 frames on the context's profile.  Then 7 outputs in mode 4, which no fused launch takes: 7 launches of 7 frames."""
    from hopperrender_amd import capi
    want2, want4 = plain(case, 42, 2), plain(case, 42, 4)
    clip = Clip(case, 42)
    c = make(case, capi.HF_FLAG_ASYNC | capi.HF_FLAG_PROFILE)
    c.setProfileInterval(1, 1)
    outs = Outputs(c, 13, off={8: np.dtype(c.dtype).itemsize})
    try:
        clip.prime(c)
        c.sync(); c.resetProfile()
        c.interpolatePeriod(clip.bufs[3].ptr, TS, outs.ptrs, 2)
        c.sync()
        pr = c.profile()
        print("13 outputs, output 8 misaligned: warp launches", pr["warp_launches"], "frames", pr["warp_frames"])
        for i in range(13):
            assert np.array_equal(outs.read(i), want2["outs"][i]), i
        assert (pr["warp_launches"], pr["warp_frames"]) == (8, 13)
        c.resetProfile()
        c.interpolateOnly(TS[:7], outs.ptrs[:7], 4)
        c.sync()
        pr = c.profile()
        print("7 outputs in mode 4: warp launches", pr["warp_launches"], "frames", pr["warp_frames"])
        for i in range(7):
            assert np.array_equal(outs.read(i), want4["outs"][i]), i
        assert (pr["warp_launches"], pr["warp_frames"]) == (7, 7)
    finally:
        c.close()
        outs.free(); clip.free()


# 3.
def test_a_refused_period_has_updated_and_calculated(native_lib):
    """t = 1.5 in a period that carries a new frame: refused with warpFrames' message -- after the update and the chain, where the three
    separate calls would have got to."""
    from hopperrender_amd import capi
    want = plain(SDR, 42, 2)
    clip = Clip(SDR, 42)
    c = make(SDR, capi.HF_FLAG_ASYNC)
    outs = Outputs(c, 2)
    try:
        clip.prime(c)
        assert c.m_frameCount == 3
        with pytest.raises(capi.HopperFlowError) as e:
            c.interpolatePeriod(clip.bufs[3].ptr, [0.5, 1.5], outs.ptrs, 2)
        assert e.value.code == capi.HF_ERR_INVALID_ARGUMENT
        assert "[HopperRender] Error in function warpFrames: blending scalar is greater than 1.0" in str(e.value)
        assert c.m_frameCount == 4
        c.sync()
        assert np.array_equal(c.readBlurredFlow(1), want["flow"])
    finally:
        c.close()
        outs.free(); clip.free()


# 4. and 6.
SEEDS = (42, 7, 23)
N_OUT = (13, 7, 2)
# The kernel names of the period of frame 3 (update, chain, 13 / 7 / 2 outputs in mode 2) on the batch's timeline, in order, as the
# library issued them before the two host paths of a period's warps became one (recorded by running this test body on that library).
CHAIN = ["plane", "large_windows_x", "large_windows_y", "large_windows_x", "large_windows_y", "level_32", "level_16", "level_8", "level_4", "level_2", "blur"]
TIMELINES = {
    "all-eligible": CHAIN + ["warp_period"] * 3,                         # one fused launch per chunk
    # chunk 0 fused; chunk 1: five of member 0's six one-output launches (the misaligned one is the generic kernel, which carries no
    # record) and member 1's one; chunk 2 fused
    "misaligned-m0-out8": CHAIN + ["warp_period"] * 8,
    "planar-out": CHAIN + ["warp_period", "planar_out_batch"] * 3,       # one conversion launch behind each chunk's warps
}


def _batch_period(variant, timeline):
    """Three SDR members of different content, row 13, n_out 13 / 7 / 2: hf_batch_run_period_wide in mode 2 (frame 3, its chain, the
    warps), then hf_batch_interpolate_period_wide in mode 3, which no fused launch takes.  Returns the timeline's kernel names."""
    from hopperrender_amd import capi
    from hopperrender_amd.calc import FlowBatch
    case = SDR
    no_fused = {"no-fused-member-0": 0, "no-fused-member-1": 1}.get(variant)
    # (the output that is only element-aligned: output 8 of member 0 -- members 1 and 2 have none -- or member 1's only output of chunk 1)
    off = {"misaligned-m0-out8": (0, 8), "misaligned-m1-out6": (1, 6)}.get(variant)
    planar = variant == "planar-out"
    clips = [Clip(case, s) for s in SEEDS]
    members = [make(case, capi.HF_FLAG_ASYNC | (capi.HF_FLAG_NO_FUSED_WARP if m == no_fused else 0) |
                    (capi.HF_FLAG_BATCH_PLANAR_OUT if planar and m == 0 else 0)) for m in range(3)]
    for clip, c in zip(clips, members):
        clip.prime(c)
        c.sync()
    batch = FlowBatch(members)
    outs = [Outputs(c, N_OUT[m], off={off[1]: 1} if off and off[0] == m else None) for m, c in enumerate(members)]
    names = []
    try:
        assert not batch.defersPlanes() and batch.planar() == (False, planar)
        ts = [TS[:k] for k in N_OUT]
        ptrs = [o.ptrs for o in outs]
        for mode in (2, 3):
            if mode == 2:
                if timeline:
                    batch.timelineEnable(256)
                prepared = batch.preparePeriod([clip.bufs[3].ptr for clip in clips], ts, ptrs, 2)
                assert len(prepared) == 7 and prepared[2] == 13
                batch.runPeriod(prepared)
                if timeline:
                    names = [r[0] for r in batch.timelineRead() if r[1] == 0]
                    batch.timelineEnable(0)
            else:
                batch.interpolatePeriod(ts, ptrs, 3)
            batch.sync()
            for m, c in enumerate(members):
                want = plain(case, SEEDS[m], mode)
                for i in range(N_OUT[m]):
                    if planar:
                        assert_planar(case, outs[m].read(i), want["outs"][i], want["stride"], (variant, mode, m, i))
                    else:
                        assert np.array_equal(outs[m].read(i), want["outs"][i]), (variant, mode, m, i)
                assert np.array_equal(c.readBlurredFlow(1), want["flow"]), (variant, m)
    finally:
        batch.close()
        for x in members + outs + clips:
            (x.close if hasattr(x, "close") else x.free)()
    return names


@pytest.mark.parametrize("variant", ["no-fused-member-0", "no-fused-member-1", "misaligned-m1-out6"])
def test_ragged_wide_batch(native_lib, variant):
    """HF_FLAG_NO_FUSED_WARP on one member (the leader; a member that is not): every chunk member by member.  Member 1's output 6
    misaligned: chunk 1 alone (members 0 and 1) goes member by member."""
    _batch_period(variant, False)


@pytest.mark.parametrize("variant", ["all-eligible", "misaligned-m0-out8", "planar-out"])
def test_ragged_wide_batch_and_its_launch_sequence(native_lib, variant):
    """All eligible (one fused launch per chunk); output 8 of member 0 misaligned (chunk 1 alone goes member by member: launches of one
    output, the misaligned one by the generic kernel, which carries no timeline record); the HF_FLAG_BATCH_PLANAR_OUT twin of the first (one
    conversion launch behind each chunk).  The kernel names of the period, in order, are the literal lists above: names and order, no
    times."""
    names = _batch_period(variant, True)
    print(variant, "timeline:", names)
    assert names == TIMELINES[variant]


# 5.
def test_dual_stream_members_on_the_shared_warp_streams(native_lib):
    """Two HF_FLAG_DUAL_STREAM members, 7 outputs each in mode 2: member by member on the batch's warp streams, beside the chain."""
    from hopperrender_amd import capi
    from hopperrender_amd.calc import FlowBatch
    case = SDR
    clips = [Clip(case, s) for s in SEEDS[:2]]
    members = [make(case, capi.HF_FLAG_ASYNC | capi.HF_FLAG_DUAL_STREAM) for _ in range(2)]
    for clip, c in zip(clips, members):
        clip.prime(c)
        c.sync()
    batch = FlowBatch(members)
    outs = [Outputs(c, 7) for c in members]
    try:
        prepared = batch.preparePeriod([clip.bufs[3].ptr for clip in clips], [TS[:7]] * 2, [o.ptrs for o in outs], 2)
        assert len(prepared) == 7
        batch.runPeriod(prepared)
        batch.sync()
        for m, c in enumerate(members):
            want = plain(case, SEEDS[m], 2)
            for i in range(7):
                assert np.array_equal(outs[m].read(i), want["outs"][i]), (m, i)
            assert np.array_equal(c.readBlurredFlow(1), want["flow"]), m
    finally:
        batch.close()
        for x in members + outs + clips:
            (x.close if hasattr(x, "close") else x.free)()
