"""GPU: every warp launch variant and every body of the staged kernel that element type, resolution scalar, frame bytes, strides, pointer
alignment, batch size, outputs per period and mode select (tests/warp_variant_model.py; csrc/hf_kernels.hip launch_warp_fast,
launch_warp_periods, launch_warp_t, launch_copy_t, warp_wg_body) against the CPU oracle.  The model's CASES is the matrix;
tests/test_warp_variant_model.py proves on the CPU that it reaches every label in each mode and every workgroup class.

Each case: its members on frames of full-range noise (any misplaced element shows), flows INJECTED with writeBlurredFlow so that the warp is
judged apart from the chain ("period" cases: synthetic scenes through the real chain with runPeriod), member-specific output counts and
blend scalars (0 and 1 exactly among them), sources and outputs at the case's byte offsets inside larger buffers.
Bar: EVERY output of EVERY member bit-exact over the W valid columns with oracle.warp_frames on the same frames and flow
(warpFrameKernel{SDR,HDR}.h:116-184: integer coordinates, one fp32 blend and level step that the oracle restates operation by operation), and
every byte of the output buffer outside the W valid columns -- stride padding, the bytes before and behind the frame -- still the sentinel.
Staged launches: the three device counters of member 0 equal the model's sums over all members EXACTLY, and the pixels are identical with
the counters on and off.  Deferring batches: defersPlanes() equals the model, the chain that follows the warp period gives the oracle's
blurred flow (it ran on the planes the warp launch built) and every member's plane is reported complete."""
import ctypes as C
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import warp_variant_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

SLACK = 64                         # bytes around a frame inside its device buffer
_frames = {}
_pool = ThreadPoolExecutor(12)     # (the oracle is plain C behind ctypes: a case's distinct outputs are computed side by side)


def case_frames(case, n):
    """n frames at the case's geometry: full-range noise, or -- through the real chain -- a synthetic scene (kept while the geometry stays)."""
    g = M.geometry(case)
    key = (case.hdr, case.H, case.W, g.in_stride, case.path == "period")
    if _frames.get("key") != key:
        _frames.clear()
        _frames["key"] = key
        _frames["f"] = []
    f = _frames["f"]
    if case.path == "period":
        from hopperrender_amd import synth
        sc = synth.Scene(case.H, case.W, bool(case.hdr), 4242, in_stride=g.in_stride)
        while len(f) < n:
            f.append(sc.frame(len(f)))
    else:
        rng = np.random.default_rng(1000 + len(f))
        while len(f) < n:
            f.append(rng.integers(0, 65536 if case.hdr else 256, size=(case.H + case.H // 2) * g.in_stride, dtype=np.uint16 if case.hdr else np.uint8))
    return f[:n]


class Buf:
    """A frame at byte offset `off` inside a device buffer with SLACK bytes of sentinel around it."""

    def __init__(self, nbytes, off, fill=0xA5):
        from hopperrender_amd.calc import DeviceBuffer
        self.n, self.off, self.fill = nbytes, off, fill
        self.dev = DeviceBuffer(nbytes + SLACK)
        self.ptr = self.dev.ptr + off
        self.reset()

    def reset(self):
        self.dev.upload(np.full(self.n + SLACK, self.fill, np.uint8))

    def put(self, a):
        from hopperrender_amd import capi
        assert a.nbytes == self.n
        capi.check(capi.load().hf_memcpy_h2d(0, C.c_void_p(self.ptr), a.ctypes.data_as(C.c_void_p), a.nbytes))

    def get(self, dtype):
        raw = self.dev.download(np.uint8)
        assert (raw[:self.off] == self.fill).all() and (raw[self.off + self.n:] == self.fill).all(), "bytes outside the frame were written"
        return raw[self.off:self.off + self.n].copy().view(dtype)

    def free(self):
        self.dev.free()


def make_context(case, R=5):
    from hopperrender_amd import capi
    from hopperrender_amd.calc import OpticalFlowCalcHDR, OpticalFlowCalcSDR
    cls = OpticalFlowCalcHDR if case.hdr else OpticalFlowCalcSDR
    return cls(case.H, case.W, case.in_stride, case.out_stride, 8, 6, case.levels[0], case.levels[1], case.max_res, search_radius=R,
               flags=capi.HF_FLAG_ASYNC | capi.HF_FLAG_NO_TIMING)


def expected(case, g, jobs):
    """{key: frame} for jobs = {key: (f12, f21, flow, t, mode)} -- the oracle, side by side."""
    from oracle import oracle
    og = oracle.make_geom(case.hdr, case.H, case.W, case.in_stride, case.out_stride, case.max_res)
    keys = list(jobs)
    run = lambda k: oracle.warp_frames(jobs[k][0], jobs[k][1], jobs[k][2], og, np.float32(jobs[k][3]), jobs[k][4], *case.levels)
    return dict(zip(keys, _pool.map(run, keys)))


def assert_frame(case, g, got, want, what):
    got, want = got.reshape(-1, g.out_stride), want.reshape(-1, g.out_stride)
    bad = got[:, :g.W] != want[:, :g.W]
    assert not bad.any(), (case.name, what, int(bad.sum()), [tuple(int(v) for v in p) for p in np.argwhere(bad)[:4]])
    pad = got[:, g.W:]
    assert (pad.view(np.uint8) == 0xA5).all(), (case.name, what, "stride padding written")


def sources(case, frames, ms):
    """Device copies of the frames per distinct source offset: {offset: [Buf per frame]}."""
    out = {}
    for off in sorted({m.src_off for m in ms}):
        out[off] = []
        for f in frames:
            b = Buf(f.nbytes, off)
            b.put(f)
            out[off].append(b)
    return out


def check_counters(case, mode, leader, flows=None):
    got = leader.counters(reset=True)["warp_workgroups"]
    want, _, _ = M.case_counts(case, mode, flows)
    assert (got["staged"], got["interior_global"], got["generic"]) == want, (case.name, mode, got, want)
    return sum(want)


def run_batch_case(case):
    """Members with injected flows, FlowBatch.interpolatePeriod in each of the case's modes."""
    from hopperrender_amd.calc import FlowBatch
    g, ms = M.geometry(case), M.members(case)
    dt = np.uint16 if case.hdr else np.uint8
    frames = case_frames(case, 3)
    flows = {k: M.flow_field(k, g) for k in dict.fromkeys(m.flow for m in ms)}
    src = sources(case, frames, ms)
    cs = [make_context(case) for _ in ms]
    outs, batch = [], None
    try:
        for c, m in zip(cs, ms):
            for k in range(3):
                c.updateFrameDeviceRef(src[m.src_off][k].ptr)
            c.sync()
            c.writeBlurredFlow(0, flows[m.flow])
        outs = [[Buf(c.output_frame_bytes, m.out_off) for _ in range(m.n_out)] for c, m in zip(cs, ms)]
        batch = FlowBatch(cs)
        assert batch.defersPlanes() == M.defers_planes(g, len(ms)), case.name
        for mode in case.modes:
            staged = any(ln.staged for ln in M.launches(case, mode))
            want = expected(case, g, {(m.flow, t): (frames[0], frames[1], flows[m.flow], t, mode) for m in ms for t in m.ts})
            first = {}
            for counted in ((False, True) if staged else (False,)):
                if counted:
                    for row in outs:
                        for b in row:
                            b.reset()
                    cs[0].countersEnable(True)
                batch.interpolatePeriod([list(m.ts) for m in ms], [[b.ptr for b in row] for row in outs], mode)
                batch.sync()
                for i, m in enumerate(ms):
                    for j, t in enumerate(m.ts):
                        got = outs[i][j].get(dt)
                        if counted:
                            assert np.array_equal(got, first[(i, j)]), (case.name, mode, i, j, "differs with the counters on")
                        else:
                            assert_frame(case, g, got, want[(m.flow, t)], (mode, i, j, t, m.flow))
                            first[(i, j)] = got
                if counted:
                    assert check_counters(case, mode, cs[0]) > 0
                    cs[0].countersEnable(False)
    finally:
        if batch is not None:
            batch.close()
        for c in cs:
            c.close()
        for b in [x for row in outs for x in row] + [x for v in src.values() for x in v]:
            b.free()


def run_period_case(case):
    """The real chain: FlowBatch.runPeriod, one source period per mode.  Period k warps frames k-2 and k-1 with the flow of that pair and
    computes the flow of (k-1, k); a deferring batch issues the warps first and lets that launch build frame k-1's plane for the chain."""
    from hopperrender_amd.calc import FlowBatch
    from oracle import oracle
    g, ms = M.geometry(case), M.members(case)
    og = oracle.make_geom(case.hdr, case.H, case.W, case.in_stride, case.out_stride, case.max_res)
    dt = np.uint16 if case.hdr else np.uint8
    R = 16
    frames = case_frames(case, 2 + len(case.modes))
    chain = _pool.map(lambda k: oracle.calculate_optical_flow(frames[k - 1], frames[k], og, R)[1], range(1, len(frames)))
    src = sources(case, frames, ms)
    cs = [make_context(case, R) for _ in ms]
    outs, batch = [], None
    try:
        outs = [[Buf(c.output_frame_bytes, m.out_off) for _ in range(m.n_out)] for c, m in zip(cs, ms)]
        batch = FlowBatch(cs)
        defers = M.defers_planes(g, len(ms))
        assert batch.defersPlanes() == defers, case.name
        ptrs = lambda k: [src[m.src_off][k].ptr for m in ms]
        batch.runPeriod(batch.preparePeriod(ptrs(0), None, None, calculate_flow=False))
        batch.runPeriod(batch.preparePeriod(ptrs(1), None, None))
        batch.sync()
        flows = dict(zip(range(1, len(frames)), chain))
        cs[0].countersEnable(True)
        plans, optr = [list(m.ts) for m in ms], [[b.ptr for b in row] for row in outs]
        for k, mode in enumerate(case.modes, start=2):
            staged = any(ln.staged for ln in M.launches(case, mode))
            assert staged == (defers and mode <= 2), case.name
            want = expected(case, g, {t: (frames[k - 2], frames[k - 1], flows[k - 1], t, mode) for m in ms for t in m.ts})
            batch.runPeriod(batch.preparePeriod(ptrs(k), plans, optr, mode))
            batch.sync()
            for i, (c, m) in enumerate(zip(cs, ms)):
                assert np.array_equal(c.readBlurredFlow(0), flows[k - 1]), (case.name, k, i, "flow of the warped pair")
                assert np.array_equal(c.readBlurredFlow(1), flows[k]), (case.name, k, i, "flow of the chain behind the warp period")
                if defers:
                    assert c.readPhasePlane(1)[1], (case.name, k, i, "plane not complete")
                for j, t in enumerate(m.ts):
                    assert_frame(case, g, outs[i][j].get(dt), want[t], (mode, i, j, t))
            if staged:
                assert check_counters(case, mode, cs[0], {m.flow: flows[k - 1] for m in ms}) > 0
            else:
                assert sum(cs[0].counters(reset=True)["warp_workgroups"].values()) == 0, case.name
    finally:
        if batch is not None:
            batch.close()
        for c in cs:
            c.close()
        for b in [x for row in outs for x in row] + [x for v in src.values() for x in v]:
            b.free()


def run_single_case(case):
    """One context: a fused period (interpolateOnly), single outputs (warpFrames into setOutputBuffer) or copyFrame."""
    from oracle import oracle
    g, m = M.geometry(case), M.members(case)[0]
    og = oracle.make_geom(case.hdr, case.H, case.W, case.in_stride, case.out_stride, case.max_res)
    dt = np.uint16 if case.hdr else np.uint8
    frames = case_frames(case, 3)
    flow = M.flow_field(m.flow, g)
    src = sources(case, frames, [m])[m.src_off]
    c = make_context(case)
    ts = m.ts if case.path == "single" else case.ts
    outs = [Buf(c.output_frame_bytes, m.out_off) for _ in ts]
    try:
        for k in range(3):
            c.updateFrameDeviceRef(src[k].ptr)
        c.sync()
        c.writeBlurredFlow(0, flow)
        if case.path == "copy":
            c.setOutputBuffer(outs[0].ptr)
            c.copyFrame()
            c.sync()
            assert_frame(case, g, outs[0].get(dt), oracle.copy_frame(frames[0], og, *case.levels), "copy")
            return
        for mode in case.modes:
            want = expected(case, g, {t: (frames[0], frames[1], flow, t, mode) for t in ts})
            if case.path == "single":
                c.interpolateOnly(list(ts), [b.ptr for b in outs], mode)
            else:
                for b, t in zip(outs, ts):
                    c.setOutputBuffer(b.ptr)
                    c.warpFrames(t, mode)
            c.sync()
            for b, t in zip(outs, ts):
                assert_frame(case, g, b.get(dt), want[t], (mode, t))
                b.reset()
    finally:
        c.setOutputBuffer(0)
        c.close()
        for b in outs + src:
            b.free()


def run_case(case):
    from oracle import oracle
    oracle.set_flavour(1, 1, None)      # 0 / 255 and 16 / 235 are pinned by tests/golden/levels_ramp.npz with the oracle's default reciprocal
    {"batch": run_batch_case, "period": run_period_case}.get(case.path, run_single_case)(case)


@pytest.mark.parametrize("case", M.CASES, ids=lambda c: c.name)
def test_warp_variant_matches_oracle(native_lib, case):
    run_case(case)
