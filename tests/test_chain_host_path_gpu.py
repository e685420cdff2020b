"""GPU: the one host path of a refinement chain (csrc/hf_calc.hip calculate_flow) where no other test holds it: a warm-up member of
hf_batch_run_period_auto keeps the chain statistics it had in the periods that capture a graph; the cached graphs of a batch after hf_debug_counters_enable on a member that is not its leader, and on its leader; a member's
HF_FLAG_NO_GRAPH in a batch.  The yardstick is a plain blocking context of the same geometry fed the same frames, bit for bit on the
blurred flow, the offsets and m_totalFrameDelta.

180 x 320 SDR and 360 x 640 HDR: the smallest shapes whose chain has the large-window steps (256, 128, 64) and all five small levels."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RADIUS = 16           # (the chain's table kernels, which feed the diagnostic counters, exist for radius 16)
SDR = (0, 180, 320)
HDR = (1, 360, 640)
N_FRAMES = 10         # nine chains: the six (ring phase, flow-buffer phase) keys of a member are all captured, then replayed

_frames, _plain = {}, {}


def calc_class(case):
    from hopperrender_amd.calc import OpticalFlowCalcHDR, OpticalFlowCalcSDR
    return OpticalFlowCalcHDR if case[0] else OpticalFlowCalcSDR


def frames(case, seed):
    from hopperrender_amd import synth
    if (case, seed) not in _frames:
        sc = synth.Scene(case[1], case[2], bool(case[0]), seed)
        _frames[case, seed] = [sc.frame(k) for k in range(N_FRAMES)]
    return _frames[case, seed]


def plain(case, seed):
    """A plain blocking context shown the clip: after every calculateOpticalFlow (frame counts 2 .. N_FRAMES; computed once, shared, never
    modified) the newest blurred flow, the offsets, m_totalFrameDelta and the chain statistics."""
    if (case, seed) not in _plain:
        c = calc_class(case)(case[1], case[2], search_radius=RADIUS)
        out = {}
        for k, f in enumerate(frames(case, seed)):
            c.updateFrame(f)
            if k >= 1:
                c.calculateOpticalFlow()
                st = c.stats()
                out[k + 1] = dict(flow=c.readBlurredFlow(1), offsets=c.readOffsets(), delta=c.m_totalFrameDelta,
                                  iterations=st["iterations"], initial_window=st["initial_window"])
        c.close()
        assert out[3]["iterations"] == 8 and out[3]["initial_window"] == 256 and out[3]["offsets"].any() and out[3]["delta"] > 0
        _plain[case, seed] = out
    return _plain[case, seed]


class Rig:
    """A batch of len(seeds) asynchronous members, member m shown the clip of seeds[m] from device buffers."""

    def __init__(self, case, seeds, member_flags=None, leader_flags=0):
        from hopperrender_amd import capi
        from hopperrender_amd.calc import DeviceBuffer, FlowBatch
        self.case, self.seeds, self.dev = case, seeds, []
        for s in seeds:
            row = []
            for f in frames(case, s):
                b = DeviceBuffer(f.nbytes)
                b.upload(f)
                row.append(b)
            self.dev.append(row)
        flags = member_flags or [0] * len(seeds)
        self.members = [calc_class(case)(case[1], case[2], search_radius=RADIUS, flags=capi.HF_FLAG_ASYNC | flags[i] | (leader_flags if i == 0 else 0))
                        for i in range(len(seeds))]
        self.batch = FlowBatch(self.members)
        self.outs = [[DeviceBuffer(c.output_frame_bytes) for _ in range(2)] for c in self.members]

    def feed(self, k):
        return [row[k].ptr for row in self.dev]

    def assert_members_equal_plain(self, frame_count, what):
        for m, c in enumerate(self.members):
            want = plain(self.case, self.seeds[m])[frame_count]
            assert c.m_totalFrameDelta == want["delta"], (what, m, frame_count)
            assert np.array_equal(c.readBlurredFlow(1), want["flow"]), (what, m, frame_count)
            assert np.array_equal(c.readOffsets(), want["offsets"]), (what, m, frame_count)

    def close(self):
        self.batch.close()
        for c in self.members:
            c.close()
        for b in [b for row in self.dev + self.outs for b in row]:
            b.free()


def test_a_warm_up_member_keeps_its_chain_statistics(native_lib):
    """hf_batch_run_period_auto: in periods 1 and 2 every member has m_frameCount < 3 and rides the batched chain; as far as the member can
    tell calculateOpticalFlow has not been called -- hf_get_stats reports no iterations and no window, hf_read_offsets zeros -- although both
    periods capture a new graph.  Period 3 is the first real chain: statistics, offsets, flow and delta of a plain context after its first
    calculateOpticalFlow at m_frameCount 3.

    (No timeline here.  The first hf_batch_timeline_enable of a process records the reference event every later timeline is read against, and
    hipEventElapsedTime is a float: minutes later it resolves ~30 us, coarser than the 1 us that tests/test_timeline_gpu.py allows between two
    dispatches.  That file therefore has to stay the first one of the suite that switches a timeline on.)"""
    from hopperrender_amd import capi
    rig = Rig(SDR, (42, 7), leader_flags=capi.HF_FLAG_BATCH_EAGER_PLANES)
    try:
        assert not rig.batch.defersPlanes()
        for m in range(2):
            rig.batch.sceneSet(m, 417083, -1)
        for k in range(3):
            rig.batch.runPeriodAuto(rig.feed(k), [[0.25, 0.75]] * 2, [[b.ptr for b in row] for row in rig.outs], 2)
            rig.batch.sync()
            for m, c in enumerate(rig.members):
                st, off = c.stats(), c.readOffsets()
                print(f"period {k + 1} member {m}: iterations {st['iterations']} initial_window {st['initial_window']} offsets set {int((off != 0).sum())}")
                if k < 2:
                    assert (st["iterations"], st["initial_window"]) == (0, 0) and not off.any(), (k + 1, m)
                    assert c.m_totalFrameDelta == 0
                else:
                    want = plain(SDR, rig.seeds[m])[3]
                    assert (st["iterations"], st["initial_window"]) == (want["iterations"], want["initial_window"]), m
        rig.assert_members_equal_plain(3, "first real chain")
    finally:
        rig.close()


@pytest.mark.parametrize("case,n", [(SDR, 1), (SDR, 2), (HDR, 2)], ids=["sdr-1", "sdr-2", "hdr-2"])
def test_counters_enabled_on_any_member_drop_the_batch_graphs(native_lib, case, n):
    """Seven chains capture every key of the batch and replay the first.  hf_debug_counters_enable on the LAST member (not the leader unless
    n == 1) clears the cache: the next chain is captured again and gives what the plain context gives.  Then on the leader, whose counters
    pointer every captured launch of the chain carries: the chain after it must count -- a graph kept from before would carry the null
    pointer and count nothing -- every member's windows in the leader, and still give the plain context's results.  (The leader pins the SAD
    tables on: the kernels that count are the table kernels, and fewer than four members run without them otherwise.)  The last member of
    a batch of 2 carries HF_FLAG_NO_GRAPH, which does not count in a batch: same results."""
    from hopperrender_amd import capi
    seeds = (42, 7)[:n]
    rig = Rig(case, seeds, member_flags=[0, capi.HF_FLAG_NO_GRAPH][:n], leader_flags=capi.HF_FLAG_SAD_REUSE_ALWAYS)
    try:
        def period(k):
            rig.batch.updateFramesDeviceRef(rig.feed(k))
            if k >= 1:
                rig.batch.calculateOpticalFlow()
                rig.batch.sync()
                rig.assert_members_equal_plain(k + 1, f"period {k}")

        for k in range(8):
            period(k)
        rig.members[-1].countersEnable(True)
        period(8)
        if n > 1:
            assert not rig.members[-1].counters()["levels"]      # the chain of a batch counts in its leader
            rig.members[0].countersEnable(True)
        rig.members[0].counters(reset=True)
        period(9)
        levels = rig.members[0].counters()["levels"]
        print("leader's level counters:", levels)
        assert sorted(levels) == [2, 4, 8, 16, 32]
        full_tiles = (rig.members[0].m_opticalFlowFrameWidth // 32) * (rig.members[0].m_opticalFlowFrameHeight // 32)   # (as tests/test_counters_gpu.py)
        for ws, lv in levels.items():
            assert lv["X"][0] == lv["Y"][0] == n * full_tiles * (32 // ws) ** 2, (ws, lv, n, full_tiles)
        for c in rig.members:
            c.countersEnable(False)
    finally:
        rig.close()
