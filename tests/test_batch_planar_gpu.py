"""GPU: planar 4:2:0 clips through a batch (HF_FLAG_BATCH_PLANAR_IN / HF_FLAG_BATCH_PLANAR_OUT on the leader, include/hopperflow.h;
planar_in_batch_kernel / planar_out_batch_kernel, csrc/hf_planar.hip).  The yardstick everywhere is a TWIN batch of plain members fed
planar_ref.planar_to_semiplanar(frame): the planar batch's outputs must equal the twin's through planar_ref.valid_planes_of_output,
byte for byte, and flow, m_totalFrameDelta, phase planes (with their completeness) and, in auto mode, the scene records must be equal.
Planar inputs carry random garbage in their padding columns; every planar member's input lives in ONE device buffer that is overwritten
before the next period (the batch keeps no reference), and every caller-owned output sits between sentinel bytes.  The shapes are those
of tests/batch_planar_cases.py, which tests/test_batch_planar.py holds to the access paths of the two launches."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import batch_planar_cases as cases
import planar_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN, BOUT, EAGER = 0x20000, 0x40000, 0x1000
GUARD = 256
TS = [0.1988, 0.3996, 0.5984, 0.7992, 0.998, 0.25]


def _cls(hdr):
    from hopperrender_amd.calc import OpticalFlowCalcHDR, OpticalFlowCalcSDR
    return OpticalFlowCalcHDR if hdr else OpticalFlowCalcSDR


def _pictures(H, W, S, hdr, n, seed=9, wrap=False, cut_at=None):
    """(planar frames of stride S, their NV12 / P010 twins) -- n pictures of a moving synthetic scene (a hard cut at cut_at); the
    construction of tests/test_planar_io_gpu.py"""
    from hopperrender_amd import synth
    a, b = synth.Scene(H, W, hdr, seed), synth.Scene(H, W, hdr, seed + 999)
    rng = np.random.default_rng(seed)
    planar, twin = [], []
    for k in range(n):
        nv = (b if cut_at is not None and k >= cut_at else a).frame(k)
        p = planar_ref.semiplanar_to_planar(nv, H, W, W, hdr)
        y, u, v = planar_ref.planar_planes(p, H, W, W)
        dt = np.uint16 if hdr else np.uint8
        q = rng.integers(0, 65536 if hdr else 256, H * S * 3 // 2).astype(dt)    # padding garbage
        qy, qu, qv = planar_ref.planar_planes(q, H, W, S)
        qy[:], qu[:], qv[:] = y, u, v
        if wrap:   # LSB-aligned values above 1023 lose their top bits on the way in
            qy[::7, ::3] |= 0xA800
            qu[::3, ::5] |= 0x4400
            qv[1::4, ::2] |= 0xFC00
        planar.append(q)
        twin.append(planar_ref.planar_to_semiplanar(q, H, W, S, hdr))
    return planar, twin


def _same_output(planar_side_out, plain_out, H, W, S, hdr, planar, what=""):
    a = planar_ref.valid_planes_of_output(planar_side_out, H, W, S, hdr, planar)
    b = planar_ref.valid_planes_of_output(plain_out, H, W, S, hdr, False)
    for x, y, name in zip(a, b, "YUV"):
        assert x.shape == y.shape and (x == y).all(), f"{what}: plane {name} differs in {(x != y).sum()} elements"


def _same_state(A, B, what=""):
    assert A.m_totalFrameDelta == B.m_totalFrameDelta, what
    for i in (0, 1):
        assert (A.readBlurredFlow(i) == B.readBlurredFlow(i)).all(), what
    for s in (0, 1, 2):
        pa, ca = A.readPhasePlane(s)
        pb, cb = B.readPhasePlane(s)
        assert ca == cb and (pa == pb).all(), (what, s, ca, cb)


def _h2d(ptr, a):
    from hopperrender_amd import capi
    a = np.ascontiguousarray(a)
    capi.check(capi.load().hf_memcpy_h2d(0, C.c_void_p(ptr), a.ctypes.data_as(C.c_void_p), a.nbytes))


class Guarded:
    """A caller-owned output frame `off` bytes into a device buffer, GUARD sentinel bytes before and after it."""

    def __init__(self, nbytes, off=0):
        from hopperrender_amd.calc import DeviceBuffer
        self.nbytes, self.off = nbytes, off
        self.buf = DeviceBuffer(nbytes + 2 * GUARD + 16)
        self.buf.upload(np.full(self.buf.nbytes, 0xA5, np.uint8))
        self.ptr = self.buf.ptr + GUARD + off

    def read(self, dtype):
        raw = self.buf.download(np.uint8)
        lo = GUARD + self.off
        assert (raw[:lo] == 0xA5).all() and (raw[lo + self.nbytes:] == 0xA5).all(), "sentinel bytes around an output frame were written"
        return raw[lo:lo + self.nbytes].copy().view(dtype)

    def free(self):
        self.buf.free()


class Pair:
    """A batch under test (leader flags `leader`) and its plain twin, member for member, on pictures of their own."""

    def __init__(self, c, leader, n_periods, R=8, wrap=False, cut_at=None, extra=0, levels=(0.0, 255.0), shared_pictures=False, seeds=None):
        from hopperrender_amd import capi
        from hopperrender_amd.calc import DeviceBuffer, FlowBatch
        self.c, self.leader, self.n = c, leader, len(c.in_offsets)
        n, hdr = self.n, c.hdr
        seeds = seeds or ([9] * n if shared_pictures else [9 + (m % 4) for m in range(n)])
        made = {}
        for s in sorted(set(seeds)):
            made[s] = _pictures(c.H, c.W, c.S_in, hdr, n_periods, seed=s, wrap=wrap, cut_at=cut_at)
        self.planar = [made[s][0] for s in seeds]
        self.twin = [made[s][1] for s in seeds]
        mk = lambda fl: _cls(hdr)(c.H, c.W, c.S_in, c.S_out, 8, 6, levels[0], levels[1], search_radius=R, flags=capi.HF_FLAG_ASYNC | extra | fl)
        self.P = [mk(leader if i == 0 else 0) for i in range(n)]
        self.Q = [mk((leader & EAGER) if i == 0 else 0) for i in range(n)]
        self.bp, self.bq = FlowBatch(self.P), FlowBatch(self.Q)
        assert self.bp.planar() == (bool(leader & BIN), bool(leader & BOUT)) and self.bq.planar() == (False, False)
        assert self.bp.defersPlanes() == self.bq.defersPlanes()
        self.dt = np.uint16 if hdr else np.uint8
        in_bytes = self.P[0].input_frame_bytes
        self.in_bufs = [DeviceBuffer(in_bytes + 16) for _ in range(n)]              # ONE input buffer per planar-side member
        self.in_ptrs = [b.ptr + off for b, off in zip(self.in_bufs, c.in_offsets)]
        self.q_frames = []                                                           # the twin references its frames: all kept
        self.outs_p, self.outs_q = [], []

    def feed(self, k):
        """Uploads period k's pictures; returns (planar side's, twin's) device pointers."""
        from hopperrender_amd.calc import DeviceBuffer
        self.bp.sync()                                     # the batch stream has passed the previous call: the one buffer is free
        rows = []
        for _ in range(1 if self.leader & BIN else 2):     # without PLANAR_IN the batch under test references its frames too
            row = []
            for m in range(self.n):
                b = DeviceBuffer(self.twin[m][k].nbytes)
                b.upload(self.twin[m][k])
                row.append(b)
            self.q_frames.append(row)
            rows.append([b.ptr for b in row])
        if self.leader & BIN:
            for m in range(self.n):
                _h2d(self.in_ptrs[m], self.planar[m][k])
            return self.in_ptrs, rows[0]
        return rows[1], rows[0]

    def new_outputs(self, n_outs, null=()):
        """Fresh caller-owned outputs of one period: (planar side's pointers, twin's pointers); `null` = {(member, i)} left NULL."""
        out_bytes = self.P[0].output_frame_bytes
        rp = [[None if (m, i) in null else Guarded(out_bytes, self.c.out_offsets[m]) for i in range(n_outs[m])] for m in range(self.n)]
        rq = [[None if (m, i) in null else Guarded(out_bytes) for i in range(n_outs[m])] for m in range(self.n)]
        self.outs_p.append(rp); self.outs_q.append(rq)
        ptrs = lambda rows: [[(g.ptr if g else 0) for g in row] for row in rows]
        return ptrs(rp), ptrs(rq)

    def check_outputs(self, k=-1, what=""):
        c = self.c
        for m, (rp, rq) in enumerate(zip(self.outs_p[k], self.outs_q[k])):
            for i, (gp, gq) in enumerate(zip(rp, rq)):
                if gp:
                    _same_output(gp.read(self.dt), gq.read(self.dt), c.H, c.W, c.S_out, c.hdr, bool(self.leader & BOUT), f"{what} member {m} output {i}")

    def check_state(self, members=None, what=""):
        for m in (range(self.n) if members is None else members):
            _same_state(self.P[m], self.Q[m], f"{what} member {m}")

    def run_period(self, k, n_outs, mode=2, null=(), check=True, state=True):
        """Period k through hf_batch_run_period on both batches: frame k, the chain from the second frame on, warps from the third."""
        fp, fq = self.feed(k)
        warp = k >= 2 and n_outs is not None
        op, oq = self.new_outputs(n_outs, null) if warp else (None, None)
        sc = [TS[:x] for x in n_outs] if warp else None
        self.bp.runPeriod(self.bp.preparePeriod(fp, sc, op, mode, calculate_flow=k >= 1))
        self.bq.runPeriod(self.bq.preparePeriod(fq, sc, oq, mode, calculate_flow=k >= 1))
        self.bp.sync(); self.bq.sync()
        if warp and check:
            self.check_outputs(-1, f"period {k}")
        if k >= 1 and state:
            self.check_state(what=f"period {k}")

    def close(self):
        self.bp.close(); self.bq.close()
        for x in self.P + self.Q:
            x.close()
        for b in self.in_bufs + [b for row in self.q_frames for b in row]:
            b.free()
        for rows in self.outs_p + self.outs_q:
            for row in rows:
                for g in row:
                    if g:
                        g.free()


def _four_periods(name, leader, n_outs, mode=2, **kw):
    pair = Pair(cases.case(name), leader, 4, **kw)
    try:
        for k in range(4):
            pair.run_period(k, n_outs, mode)
    finally:
        pair.close()


# 1. -- fails without the feature: the flags are ignored and the frames are read as NV12 / P010
@pytest.mark.parametrize("name", ["basic-sdr", "basic-hdr"])
def test_basic_parity_both_sides_planar(native_lib, name):
    _four_periods(name, BIN | BOUT, (2, 3))


# 2.
@pytest.mark.parametrize("name", ["ragged-sdr", "ragged-hdr", "ragged-in-sdr", "offset-sdr", "offset-hdr", "mid-hdr"])
def test_element_paths_and_tails(native_lib, name):
    _four_periods(name, BIN | BOUT, (2, 3), R=16 if name == "mid-hdr" else 8)


# 3.
@pytest.mark.parametrize("leader", [BIN, BOUT], ids=["in-only", "out-only"])
@pytest.mark.parametrize("name", ["basic-sdr", "basic-hdr"])
def test_only_one_side_planar(native_lib, name, leader):
    _four_periods(name, leader, (2, 3))


# 4.
def test_null_outputs_and_empty_members(native_lib):
    """Member 1 has n_out == 0 (no pairs; the period goes member by member); then member 0's second output is NULL: it lands in the member's
    internal output frame, semi-planar, as the twin's does."""
    from hopperrender_amd.calc import DeviceBuffer
    c = cases.case("basic-sdr")
    pair = Pair(c, BIN | BOUT, 5)
    try:
        for k in range(3):
            pair.run_period(k, (3, 0))
        assert pair.outs_p[-1][1] == []
        pair.run_period(3, (3, 2), null={(0, 1)})
        a, b = DeviceBuffer(pair.P[0].output_frame_bytes), DeviceBuffer(pair.P[0].output_frame_bytes)
        pair.P[0].downloadFrameDevice(a.ptr); pair.Q[0].downloadFrameDevice(b.ptr)
        pair.bp.sync(); pair.bq.sync()
        _same_output(a.download(pair.dt), b.download(pair.dt), c.H, c.W, c.S_out, c.hdr, False, "the internal output frame")
        pair.run_period(4, (0, 0))
        a.free(); b.free()
    finally:
        pair.close()


# 5.
@pytest.mark.parametrize("mode", [3, 5])
def test_diagnostic_modes_member_by_member(native_lib, mode):
    _four_periods("basic-sdr", BIN | BOUT, (2, 3), mode=mode)


# 6.
def test_auto_periods_through_run_clips_with_a_cut_and_a_rearmed_slot(native_lib):
    """Four members, leader EAGER_PLANES | PLANAR_IN | PLANAR_OUT: seven periods of clips with a hard cut at frame 4 through run_clips, then
    slot 1 is re-armed (m_frameCount = 0) and three more periods go through runPeriodAuto -- members below m_frameCount 3 among the others,
    and a copy period forced on member 2.  Outputs, kinds and records equal the plain twin batch's: copy periods arrive planar with the
    levels (16 / 235) applied."""
    from hopperrender_amd import batch as hbatch
    from hopperrender_amd.calc import DeviceBuffer
    c = cases.Case("auto", 180, 320, 320, 320, 0, (0,) * 4, (0,) * 4)
    n1, n2 = 7, 3
    pair = Pair(c, EAGER | BIN | BOUT, n1 + n2, cut_at=4, levels=(16.0, 235.0), seeds=[7, 42, 11, 3])
    try:
        assert not pair.bp.defersPlanes()
        dev = {}
        for side, frames in (("p", pair.planar), ("q", pair.twin)):
            dev[side] = [[DeviceBuffer(f.nbytes) for f in fs] for fs in frames]
            for bufs, fs in zip(dev[side], frames):
                for b, f in zip(bufs, fs):
                    b.upload(f)
        clips = lambda side: [[b.ptr for b in bufs[:n1]] for bufs in dev[side]]
        out_p, kinds_p = hbatch.run_clips(pair.bp, clips("p"), threshold=200)
        out_q, kinds_q = hbatch.run_clips(pair.bq, clips("q"), threshold=200)
        assert kinds_p == kinds_q and all(k[:2] == ["copy", "copy"] for k in kinds_p)
        for m in range(4):
            assert len(out_p[m]) == len(out_q[m]) == len(kinds_p[m]) > n1
            for i, (a, b) in enumerate(zip(out_p[m], out_q[m])):
                _same_output(a.download(pair.dt), b.download(pair.dt), c.H, c.W, c.S_out, c.hdr, True, f"clip {m} output {i} ({kinds_p[m][i]})")
                a.free(); b.free()
        for b_, ms in ((pair.bp, pair.P), (pair.bq, pair.Q)):
            ms[1].m_frameCount = 0
            b_.sceneSet(1, 417083, 200)
        for k in range(n1, n1 + n2):
            force = [-1, -1, 0 if k == n1 + 1 else -1, -1]
            op, oq = pair.new_outputs((2, 2, 2, 2))
            pair.bp.runPeriodAuto([dev["p"][m][k].ptr for m in range(4)], [TS[:2]] * 4, op, 2, force)
            pair.bq.runPeriodAuto([dev["q"][m][k].ptr for m in range(4)], [TS[:2]] * 4, oq, 2, force)
        pair.bp.sync(); pair.bq.sync()
        for k in range(n2):
            pair.check_outputs(k, f"auto period {n1 + k}")
        for m in range(4):
            rp, rq = pair.bp.sceneRead(m), pair.bq.sceneRead(m)
            assert rp == rq and len(rp) == n2
            if m == 1:
                assert [r["frame_count"] for r in rp] == [1, 2, 3] and [r["kind"] for r in rp][:2] == [0, 0]
            if m == 2:
                assert rp[1]["kind"] == 0
        pair.check_state(what="after the auto periods")
        for side in dev.values():
            for bufs in side:
                for b in bufs:
                    b.free()
    finally:
        pair.close()


# 7.
def test_deferred_phase_planes(native_lib):
    """Three 2160 x 3840 HDR members, the smallest batch that defers: the early warp goes through the stages too and the conversion follows it."""
    c = cases.case("deferred-2160p")
    pair = Pair(c, BIN | BOUT, 4, R=16, shared_pictures=True)
    try:
        assert pair.bp.defersPlanes()
        for k in range(4):
            pair.run_period(k, (2, 2, 2), state=k == 3)
    finally:
        pair.close()


# 8.
def test_full_table_of_192_pairs(native_lib):
    _four_periods("full-table", BIN | BOUT, (6,) * 32)


# 9.
def test_hdr_values_above_1023_wrap(native_lib):
    _four_periods("basic-hdr", BIN | BOUT, (2, 3), wrap=True)


# 10.
@pytest.mark.parametrize("H,W,n", [(180, 320, 2), (180, 320, 12), (1080, 1920, 2)])
def test_one_launch_each_way(native_lib, H, W, n):
    """The recorded fourth period of case 1, of 12 members, and of a 1080p pair (whose fused period warp the timeline records): exactly one
    planar_in_batch record, first and directly ahead of the phase-plane launch, exactly one planar_out_batch record, last -- behind every
    warp -- and between them the launches of the plain twin's period, which holds neither."""
    c = cases.Case("timeline", H, W, W, W, 0, (0,) * n, (0,) * n)
    pair = Pair(c, BIN | BOUT, 4, R=8 if H == 180 else 16, shared_pictures=H != 180)
    try:
        pair.bp.timelineEnable(64, 3)
        pair.bq.timelineEnable(64, 3)
        n_outs = tuple(2 + (m % 2) for m in range(n))
        for k in range(4):
            pair.run_period(k, n_outs, state=False)
        rp = [r[0] for r in pair.bp.timelineRead() if r[1] == 0]
        rq = [r[0] for r in pair.bq.timelineRead() if r[1] == 0]
        print("planar period:", rp, "plain period:", rq)
        assert rp.count("planar_in_batch") == 1 and rp.count("planar_out_batch") == 1, rp
        assert rp[0] == "planar_in_batch" and rp[1] in ("plane", "grid_samples") and rp[-1] == "planar_out_batch", rp
        assert rp[1:-1] == rq and len(rq) >= 3, (rp, rq)            # everything between: the unchanged launches of the plain period
        assert not [x for x in rq if x.startswith("planar")], rq
        if H == 1080:
            assert rq.count("warp_period") == 1, rq
    finally:
        pair.close()


# 11.
def test_refusals_and_hf_batch_planar(native_lib):
    from hopperrender_amd import capi
    from hopperrender_amd.calc import DeviceBuffer, FlowBatch, OpticalFlowCalcSDR
    lib = capi.load()
    assert lib.hf_batch_planar(None) == 0

    def refused(members, *words):
        with pytest.raises(capi.HopperFlowError) as e:
            FlowBatch(members)
        assert e.value.code == capi.HF_ERR_INVALID_ARGUMENT, str(e.value)
        for w in words:
            assert w in str(e.value), str(e.value)

    def plain_batch_works(members):
        """a plain batch of the same contexts (another leader): three periods, outputs written"""
        b = FlowBatch(members)
        assert b.planar() == (False, False) and lib.hf_batch_planar(b._b) == 0
        rng = np.random.default_rng(3)
        f = DeviceBuffer(members[0].input_frame_bytes)
        f.upload(rng.integers(0, 256, members[0].input_frame_bytes).astype(np.uint8))
        outs = [[DeviceBuffer(members[0].output_frame_bytes)] for _ in members]
        for o in outs:
            o[0].upload(np.full(o[0].nbytes, 0xA5, np.uint8))
        for _ in range(3):
            b.runPeriod(b.preparePeriod([f.ptr] * len(members), [[0.5]] * len(members), [[o[0].ptr] for o in outs], 2))
        b.sync()
        assert not (outs[0][0].download(np.uint8) == 0xA5).all()
        b.close()
        for x in [f] + [o[0] for o in outs]:
            x.free()

    A = capi.HF_FLAG_ASYNC
    for (si, so, flag) in ((321, 320, BIN), (320, 321, BOUT), (321, 321, BIN | BOUT)):
        ms = [OpticalFlowCalcSDR(180, 320, si, so, search_radius=8, flags=A | (flag if i == 0 else 0)) for i in range(2)]
        refused(ms, "even stride")
        plain_batch_works(ms[::-1])
        for m in ms:
            m.close()
    # an odd stride on the side that is not planar is no obstacle
    ms = [OpticalFlowCalcSDR(180, 320, 321, 320, search_radius=8, flags=A | (BOUT if i == 0 else 0)) for i in range(2)]
    b = FlowBatch(ms); assert b.planar() == (False, True); b.close()
    for m in ms:
        m.close()
    for flag in (BIN, BOUT):
        ms = [OpticalFlowCalcSDR(180, 320, search_radius=8, flags=A | capi.HF_FLAG_DUAL_STREAM | (flag if i == 0 else 0)) for i in range(2)]
        refused(ms, "HF_FLAG_DUAL_STREAM")
        plain_batch_works(ms[::-1])
        for m in ms:
            m.close()
    # contexts with planar flags of their own: refused as before, whatever the leader says
    ms = [OpticalFlowCalcSDR(180, 320, search_radius=8, flags=A | (BIN if i == 0 else capi.HF_FLAG_PLANAR_IN)) for i in range(2)]
    refused(ms, "HF_FLAG_PLANAR_IN")
    for m in ms:
        m.close()
    for flag, bits in ((0, 0), (BIN, 1), (BOUT, 2), (BIN | BOUT, 3)):
        ms = [OpticalFlowCalcSDR(180, 320, search_radius=8, flags=A | (flag if i == 0 else BIN | BOUT)) for i in range(2)]   # only the leader's count
        b = FlowBatch(ms)
        assert lib.hf_batch_planar(b._b) == bits and b.planar() == (bool(bits & 1), bool(bits & 2))
        b.close()
        for m in ms:
            m.close()


CHILD = r"""
import sys, ctypes as C
sys.path.insert(0, {root!r}); sys.path.insert(0, {root!r} + "/tests")
from hopperrender_amd import capi
from hopperrender_amd.calc import OpticalFlowCalcSDR
import test_batch_planar_gpu as T
assert capi.is_debug_bounds_build()
T._four_periods("ragged-sdr", T.BIN | T.BOUT, (2, 3))
T._four_periods("offset-sdr", T.BIN | T.BOUT, (2, 3))
probe = OpticalFlowCalcSDR(64, 96)
n = C.c_uint32(0); first = (C.c_uint32 * 4)()
capi.check(probe._lib.hf_debug_bounds_violations(probe._ctx, C.byref(n), first, 0), probe._ctx)
assert n.value == 0, (n.value, list(first))
probe.close()
print("BATCH-PLANAR-BOUNDS-OK")
"""


# 12.
def test_ragged_case_under_the_bounds_checking_build(native_lib):
    """Case 2's SDR variant (and its offset twin) in a child process on libhopperflow_dbg.so -- every index of the two batched kernels
    checked: zero violations."""
    from hopperrender_amd import build
    dbg = build.build_flow(debug_bounds=True)
    env = dict(os.environ, HF_LIB=dbg)
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT)], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0 and "BATCH-PLANAR-BOUNDS-OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
