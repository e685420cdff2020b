"""GPU: whole clips through a batch with the warp-or-copy decision taken on the device (hf_batch_scene_set / hf_batch_run_period_auto /
hf_batch_scene_read, csrc/hf_scene.hip).  The yardstick is the sequential filter on plain blocking contexts of the same library -- the
loop of hopperrender_amd/batch.py run_chunk: NativeFilter + updateFrame / calculateOpticalFlow / warpFrames or copyFrame /
downloadFrame -- output byte for output byte over the valid columns, kind for kind, record for record.

Four clips of 14 frames with a hard cut (two synthetic scenes spliced, as tests/test_filter_gpu.py builds its clips), search radius 8,
threshold 200, 24 fps source.  The copied periods below were taken from the CPU oracle and protocol.SceneChangeDetector; the tests
assert that the sequential run shows exactly them, so a change of the content generator cannot make the comparison vacuous:

    member  seed  frames   copied period (source frame k, 0-based; periods 0 and 1 are copies for every clip: m_frameCount < 3)
    A       42    7 + 7    8
    B       7     5 + 9    6
    C       11    14 + 0   none
    D       3     9 + 5    10
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CLIPS = {"A": (42, 7, 7), "B": (7, 5, 9), "C": (11, 14, 0), "D": (3, 9, 5)}
COPIED = {"A": [8], "B": [6], "C": [], "D": [10]}
N_FRAMES, RADIUS, GUARD = 14, 8, 256
# hdr, H, W, input stride, output stride, target frame time (24 -> 60 / 24 -> 120)
SDR = (0, 180, 320, 323, 325, 166667)
HDR = (1, 360, 640, 0, 0, 83333)
SOURCE_24 = 417083


def cut_clip(case, name):
    """tests/test_filter_gpu.py cut_clip, with the case's input stride"""
    from hopperrender_amd import synth
    hdr, H, W, si = case[:4]
    seed, n_before, n_after = CLIPS[name]
    a = synth.Scene(H, W, bool(hdr), seed, in_stride=si)
    b = synth.Scene(H, W, bool(hdr), seed + 999, in_stride=si)
    return [a.frame(k) for k in range(n_before)] + [b.frame(n_before + k) for k in range(n_after)]


_clips, _plans, _seq = {}, {}, {}


def clip(case, name):
    if (case, name) not in _clips:
        _clips[case, name] = cut_clip(case, name)
    return _clips[case, name]


def plan(case, n=N_FRAMES):
    from hopperrender_amd.protocol import BlendSchedule
    if (case, n) not in _plans:
        _plans[case, n] = BlendSchedule(SOURCE_24, case[5]).plan(n)
    return _plans[case, n]


def calc_class(case):
    from hopperrender_amd.calc import OpticalFlowCalcHDR, OpticalFlowCalcSDR
    return OpticalFlowCalcHDR if case[0] else OpticalFlowCalcSDR


def valid(case, frame):
    """The valid columns of an output frame: [H + H / 2][W]"""
    hdr, H, W, _, so = case[:5]
    S = so if so > 0 else W
    return frame.reshape(H + H // 2, S)[:, :W]


def sequential(case, segments, mode, scalars, force=None):
    """The sequential filter on one plain context: `segments` = clips shown one after the other (NewSegment between them), scalars[k] = the
    blending scalars of period k over all segments (an empty list: no output, the history still advances).  force: {period: kind}.
    Returns per period (outputs, record) with record = frame_count, total_delta (0: nothing pushed), kind, average, d1, d2."""
    from hopperrender_amd.protocol import NativeFilter
    hdr, H, W, si, so, target = case
    calc = calc_class(case)(H, W, si, so, search_radius=RADIUS)
    host = NativeFilter(SOURCE_24, target, mode, 200)
    out, k = [], 0
    for s, frames in enumerate(segments):
        if s:
            calc.m_frameCount = 0          # NewSegment (HopperRender.cpp:840)
            host.new_segment(1.0)
        for f in frames:
            calc.updateFrame(f)
            count, delta = calc.m_frameCount, 0
            if count >= 3:
                calc.calculateOpticalFlow()
                delta = calc.m_totalFrameDelta
                host.push(count, delta)
            cut = host.detect(count)
            kind = 1 if count >= 3 and not cut else 0
            if force and k in force:
                kind = force[k]
            frames_out = []
            for t in scalars[k]:
                if kind:
                    calc.warpFrames(t, mode)
                else:
                    calc.copyFrame()
                frames_out.append(valid(case, calc.downloadFrame()).copy())
            st = host.state()
            out.append((frames_out, dict(frame_count=count, total_delta=delta, kind=kind, average=st["average_frame_delta"],
                                         d1=st["scene_change_delta1"], d2=st["scene_change_delta2"])))
            k += 1
    host.close(); calc.close()
    return out


def sequential_clip(case, name, mode):
    """The sequential run of one of the four clips (computed once, shared, never modified), checked against the table above."""
    key = (case, name, mode)
    if key not in _seq:
        ref = sequential(case, [clip(case, name)], mode, plan(case))
        copied = [k for k, (_, r) in enumerate(ref) if r["kind"] == 0]
        assert copied == [0, 1] + COPIED[name], (name, copied, [r["total_delta"] for _, r in ref])
        _seq[key] = ref
    return _seq[key]


class Outputs:
    """Device buffers for the outputs of one member: every output in a buffer of its own, GUARD sentinel bytes before and after the frame."""

    def __init__(self, calc):
        self.calc, self.bufs = calc, []
        self.fill = np.full(calc.output_frame_bytes + 2 * GUARD, 0xA5, np.uint8)

    def new(self, n):
        from hopperrender_amd.calc import DeviceBuffer
        row = []
        for _ in range(n):
            b = DeviceBuffer(len(self.fill), self.calc.device_index)
            b.upload(self.fill)
            row.append(b)
        self.bufs.append(row)
        return [b.ptr + GUARD for b in row]

    def read(self, case):
        """[period][output] valid columns; asserts the sentinels around every frame"""
        out = []
        for row in self.bufs:
            frames = []
            for b in row:
                raw = b.download(np.uint8)
                assert (raw[:GUARD] == 0xA5).all() and (raw[-GUARD:] == 0xA5).all(), "sentinel bytes around an output frame were written"
                frames.append(valid(case, raw[GUARD:-GUARD].view(self.calc.dtype)))
            out.append(frames)
        return out

    def free(self):
        for row in self.bufs:
            for b in row:
                b.free()


def upload_frames(frames_by_name):
    from hopperrender_amd.calc import DeviceBuffer
    dev = {}
    for name, frames in frames_by_name.items():
        dev[name] = []
        for f in frames:
            b = DeviceBuffer(f.nbytes)
            b.upload(f)
            dev[name].append(b)
    return dev


def run_batch(case, mode, slots, feed, scalars, force=None, rearm=None, keep=None):
    """One batch, one member per entry of `slots`, all periods through runPeriodAuto, ONE sync at the end.
    feed(m, k) = the device frame member m is fed in period k; scalars(m, k) = its blending scalars; force(k) = force_kind list or None;
    rearm = {period: [members]} re-armed (m_frameCount = 0, sceneSet) before that period; keep = the members whose results are read.
    Returns {m: [(outputs, record)] per period}."""
    from hopperrender_amd import capi
    from hopperrender_amd.calc import FlowBatch
    hdr, H, W, si, so, target = case
    n = len(slots)
    members = [calc_class(case)(H, W, si, so, search_radius=RADIUS, flags=capi.HF_FLAG_ASYNC | (capi.HF_FLAG_BATCH_EAGER_PLANES if i == 0 else 0))
               for i in range(n)]
    batch = FlowBatch(members)
    assert not batch.defersPlanes()
    for m in range(n):
        batch.sceneSet(m, SOURCE_24, -1)
    outs = [Outputs(c) for c in members]
    n_periods = len(slots[0])
    for k in range(n_periods):
        for m in (rearm or {}).get(k, []):
            members[m].m_frameCount = 0
            batch.sceneSet(m, SOURCE_24, 200)
        ts = [scalars(m, k) for m in range(n)]
        batch.runPeriodAuto([feed(m, k) for m in range(n)], ts, [outs[m].new(len(ts[m])) for m in range(n)], mode, force(k) if force else None)
    batch.sync()                                   # the only wait of the whole run
    res = {}
    for m in (range(n) if keep is None else keep):
        recs = batch.sceneRead(m)
        assert len(recs) == n_periods and batch.sceneRead(m) == []
        res[m] = list(zip(outs[m].read(case), recs))
    batch.close()
    for c in members:
        c.close()
    for o in outs:
        o.free()
    return res


def assert_same(got, want, what):
    assert len(got) == len(want), what
    for k, ((g_out, g_rec), (w_out, w_rec)) in enumerate(zip(got, want)):
        assert g_rec == w_rec, (what, k, g_rec, w_rec)
        assert len(g_out) == len(w_out), (what, k)
        for i, (a, b) in enumerate(zip(g_out, w_out)):
            assert np.array_equal(a, b), f"{what}: period {k} output {i} ({'warp' if w_rec['kind'] else 'copy'}) differs in {(a != b).sum()} elements"


def run_four_clips(case, mode):
    names = "ABCD"
    dev = upload_frames({nm: clip(case, nm) for nm in names})
    p = plan(case)
    try:
        return run_batch(case, mode, [dev[nm] for nm in names], lambda m, k: dev[names[m]][k].ptr, lambda m, k: p[k])
    finally:
        for row in dev.values():
            for b in row:
                b.free()


@pytest.mark.parametrize("case,mode", [(SDR, 2), (HDR, 2), (SDR, 0)], ids=["sdr-blend", "hdr-blend", "sdr-warp12"])
def test_whole_clips_with_one_sync_equal_the_sequential_filter(native_lib, case, mode):
    got = run_four_clips(case, mode)
    for m, name in enumerate("ABCD"):
        assert_same(got[m], sequential_clip(case, name, mode), f"member {name}")


def test_a_slot_starts_a_new_clip_while_the_others_continue(native_lib):
    """Period 6: member 1 is re-armed (m_frameCount = 0, sceneSet) and fed clip D from its first frame.  Its outputs are those of the sequential
    filter shown B's first six frames and then D after a NewSegment: copies of D's frames 0 and 1 out of ring slots 2 and 1, no delta of B in
    the new history, and the previous flow of the first warp is the one the sequential run has there."""
    case, mode = SDR, 2
    names = "ABCD"
    dev = upload_frames({nm: clip(case, nm) for nm in names})
    p = plan(case)
    try:
        feed = lambda m, k: dev["D"][k - 6].ptr if (m == 1 and k >= 6) else dev[names[m]][k].ptr
        got = run_batch(case, mode, [dev[nm] for nm in names], feed, lambda m, k: p[k], rearm={6: [1]})
    finally:
        for row in dev.values():
            for b in row:
                b.free()
    want = sequential(case, [clip(case, "B")[:6], clip(case, "D")[:8]], mode, p)
    assert [r["frame_count"] for _, r in want[6:9]] == [1, 2, 3] and [r["kind"] for _, r in want[6:9]] == [0, 0, 1]
    assert_same(got[1], want, "member 1 (B, then D from period 6)")
    for m in (0, 2, 3):
        assert_same(got[m], sequential_clip(case, names[m], mode), f"member {names[m]}")


def test_forced_kinds_and_a_member_without_outputs(native_lib):
    """force_kind 1 on A's cut period gives the warp, force_kind 0 on a period of cut-free C gives copies, D has n_out == 0 in period 4:
    nothing is written for it and its history still advances (its cut at period 10 is found, every record equals the sequential run's)."""
    case, mode = SDR, 2
    names = "ABCD"
    dev = upload_frames({nm: clip(case, nm) for nm in names})
    p = plan(case)
    p_d = [([] if k == 4 else ts) for k, ts in enumerate(p)]
    force = lambda k: {8: [1, -1, -1, -1], 5: [-1, -1, 0, -1]}.get(k)
    try:
        got = run_batch(case, mode, [dev[nm] for nm in names], lambda m, k: dev[names[m]][k].ptr, lambda m, k: p_d[k] if m == 3 else p[k], force=force)
    finally:
        for row in dev.values():
            for b in row:
                b.free()
    want_a = sequential(case, [clip(case, "A")], mode, p, force={8: 1})
    want_c = sequential(case, [clip(case, "C")], mode, p, force={5: 0})
    assert want_a[8][1]["kind"] == 1 and want_c[5][1]["kind"] == 0
    assert not np.array_equal(want_a[8][0][0], sequential_clip(case, "A", mode)[8][0][0])      # (the warp of a cut period is not its copy)
    assert_same(got[0], want_a, "member A, warp forced on the cut period")
    assert_same(got[2], want_c, "member C, copy forced on period 5")
    assert_same(got[1], sequential_clip(case, "B", mode), "member B")
    ref_d = sequential_clip(case, "D", mode)
    assert_same(got[3], [(([] if k == 4 else o), r) for k, (o, r) in enumerate(ref_d)], "member D, no outputs in period 4")


@pytest.mark.parametrize("n,slots", [(1, (0,)), (32, (0, 17, 31))], ids=["batch-of-1", "batch-of-32"])
def test_smallest_and_largest_batch(native_lib, n, slots):
    case, mode = SDR, 2
    dev = upload_frames({nm: clip(case, nm) for nm in "AC"})
    p = plan(case)
    try:
        rows = [dev["A"] if m in slots else dev["C"] for m in range(n)]
        got = run_batch(case, mode, rows, lambda m, k: rows[m][k].ptr, lambda m, k: p[k], keep=slots + ((5,) if n > 5 else ()))
    finally:
        for row in dev.values():
            for b in row:
                b.free()
    for m in slots:
        assert_same(got[m], sequential_clip(case, "A", mode), f"clip A in slot {m} of {n}")
    if n > 5:
        assert_same(got[5], sequential_clip(case, "C", mode), f"clip C in slot 5 of {n}")


def _plain_periods(batch, members, dev, outs, k0):
    """Three periods of the plain path (hf_batch_run_period) on frames dev[0 .. 2]; returns the outputs of the third."""
    n = len(members)
    for k in range(3):
        batch.runPeriod(batch.preparePeriod([dev[k].ptr] * n, [[0.25, 0.75]] * n, [[b.ptr for b in row] for row in outs], 2))
    batch.sync()
    assert [c.m_frameCount for c in members] == [k0 + 3] * n
    return [[b.download(members[0].dtype) for b in row] for row in outs]


def _refused(batch, args, *words):
    from hopperrender_amd import capi
    with pytest.raises(capi.HopperFlowError) as e:
        batch.runPeriodAuto(*args)
    assert e.value.code == capi.HF_ERR_STATE, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_rejections_enqueue_nothing_and_leave_the_plain_path_alone(native_lib):
    """HF_ERR_STATE with a message that says what to do; after each one the batch's plain path gives what it gave before: periods 4-6 on the
    frames of periods 1-3 repeat the third period's outputs (same ring frames, same previous flow) only if nothing was enqueued or moved."""
    from hopperrender_amd import capi
    from hopperrender_amd.calc import DeviceBuffer, FlowBatch, OpticalFlowCalcHDR, OpticalFlowCalcSDR
    rng = np.random.default_rng(1)

    def setup(cls, H, W, n, flags, leader_flags=0):
        members = [cls(H, W, search_radius=RADIUS, flags=flags | (leader_flags if i == 0 else 0)) for i in range(n)]
        base = rng.integers(0, 1 << (16 if cls.is_hdr else 8), size=members[0].input_frame_bytes // np.dtype(members[0].dtype).itemsize)
        dev = []
        for k in range(3):
            b = DeviceBuffer(members[0].input_frame_bytes)
            b.upload(np.roll(base, 7 * k).astype(members[0].dtype))
            dev.append(b)
        outs = [[DeviceBuffer(members[0].output_frame_bytes) for _ in range(2)] for _ in range(n)]
        return members, FlowBatch(members), dev, outs

    def teardown(members, batch, dev, outs):
        batch.close()
        for c in members:
            c.close()
        for b in dev + [b for row in outs for b in row]:
            b.free()

    def auto_args(n, dev, outs):
        return ([dev[0].ptr] * n, [[0.25, 0.75]] * n, [[b.ptr for b in row] for row in outs], 2)

    # never armed / armed in part; then a record ring that would overflow
    members, batch, dev, outs = setup(OpticalFlowCalcSDR, 180, 320, 2, capi.HF_FLAG_ASYNC, capi.HF_FLAG_BATCH_EAGER_PLANES)
    first = _plain_periods(batch, members, dev, outs, 0)
    _refused(batch, auto_args(2, dev, outs), "never armed", "hf_batch_scene_set")
    batch.sceneSet(0, SOURCE_24, -1)
    _refused(batch, auto_args(2, dev, outs), "member 1", "hf_batch_scene_set")
    again = _plain_periods(batch, members, dev, outs, 3)
    assert all(np.array_equal(a, b) for ra, rb in zip(first, again) for a, b in zip(ra, rb))
    batch.sceneSet(1, SOURCE_24, -1)
    for _ in range(128):                                   # the ring holds 128 periods (at least 64) ...
        batch.runPeriodAuto(*auto_args(2, dev, outs))
    count = members[0].m_frameCount
    _refused(batch, auto_args(2, dev, outs), "ring", "hf_batch_scene_read")    # ... the 129th unread one is refused
    assert [c.m_frameCount for c in members] == [count] * 2
    batch.sync()
    assert len(batch.sceneRead(0)) == 128
    _refused(batch, auto_args(2, dev, outs), "member 1")   # member 1's ring is still full
    assert len(batch.sceneRead(1)) == 128
    batch.runPeriodAuto(*auto_args(2, dev, outs))          # room again
    batch.sync()
    assert [len(batch.sceneRead(m)) for m in (0, 1)] == [1, 1]
    a = _plain_periods(batch, members, dev, outs, count + 1)
    assert all(np.array_equal(x, y) for ra, rb in zip(first, a) for x, y in zip(ra, rb))
    teardown(members, batch, dev, outs)

    # HF_FLAG_DUAL_STREAM members
    members, batch, dev, outs = setup(OpticalFlowCalcSDR, 180, 320, 2, capi.HF_FLAG_ASYNC | capi.HF_FLAG_DUAL_STREAM, capi.HF_FLAG_BATCH_EAGER_PLANES)
    first = _plain_periods(batch, members, dev, outs, 0)
    for m in range(2):
        batch.sceneSet(m, SOURCE_24, -1)
    _refused(batch, auto_args(2, dev, outs), "HF_FLAG_DUAL_STREAM")
    again = _plain_periods(batch, members, dev, outs, 3)
    assert all(np.array_equal(a, b) for ra, rb in zip(first, again) for a, b in zip(ra, rb))
    teardown(members, batch, dev, outs)

    # a batch that defers its phase planes (three 2160p HDR members: the smallest that does)
    members, batch, dev, outs = setup(OpticalFlowCalcHDR, 2160, 3840, 3, capi.HF_FLAG_ASYNC)
    assert batch.defersPlanes()
    first = _plain_periods(batch, members, dev, outs, 0)
    for m in range(3):
        batch.sceneSet(m, SOURCE_24, -1)
    _refused(batch, auto_args(3, dev, outs), "defers", "HF_FLAG_BATCH_EAGER_PLANES")
    again = _plain_periods(batch, members, dev, outs, 3)
    assert all(np.array_equal(a, b) for ra, rb in zip(first, again) for a, b in zip(ra, rb))
    teardown(members, batch, dev, outs)


CHILD = r"""
import sys, ctypes as C
sys.path.insert(0, {root!r}); sys.path.insert(0, {root!r} + "/tests")
from hopperrender_amd import capi
from hopperrender_amd.calc import OpticalFlowCalcSDR
import test_batch_scene_gpu as T
assert capi.is_debug_bounds_build()
got = T.run_four_clips(T.SDR, 2)
for m, name in enumerate("ABCD"):
    T.assert_same(got[m], T.sequential_clip(T.SDR, name, 2), "member " + name)
probe = OpticalFlowCalcSDR(64, 96)
n = C.c_uint32(0); first = (C.c_uint32 * 4)()
capi.check(probe._lib.hf_debug_bounds_violations(probe._ctx, C.byref(n), first, 0), probe._ctx)
assert n.value == 0, (n.value, list(first))
probe.close()
print("SCENE-BOUNDS-OK")
"""


def test_whole_clips_under_the_bounds_checking_build(native_lib):
    """The SDR case of the first test in a child process on libhopperflow_dbg.so (every gather index of every kernel checked, the two new
    ones included): zero violations -- also with members whose m_frameCount is below 3 in the batched chain and warp launches."""
    from hopperrender_amd import build
    dbg = build.build_flow(debug_bounds=True)
    env = dict(os.environ, HF_LIB=dbg)
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT)], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0 and "SCENE-BOUNDS-OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
