"""GPU: source periods of more than six outputs through a batch (hf_batch_interpolate_period_wide / hf_batch_run_period_wide /
hf_batch_run_period_auto_wide, include/hopperflow.h): 23.976 fps to 144, 165, 240 and 480 Hz.  A wide period is a few launches of the
kernels the batch already has -- chunks of six outputs per member (csrc/hf_launch_plan.h plan_period_chunks; tests/test_period_chunks.py
holds the split) -- so every yardstick here is an existing path of the same library, byte for byte: the sequential filter on a plain
context (tests/test_batch_scene_gpu.py, imported for its helpers), the same periods issued member by member with
hf_interpolate_period_ex on a twin batch, the plain twin of a planar batch (tests/planar_ref.py), the eager twin of a plane-deferring
batch.  Shapes are the small ones of those tests; the deferring batch is three 2160p HDR members, the smallest that defers."""
import ctypes as C

import numpy as np
import pytest

import test_batch_planar_gpu as P   # (its Pair compares through tests/planar_ref.py)
import test_batch_scene_gpu as T

pytestmark = pytest.mark.gpu

HZ60, HZ144, HZ165, HZ240, HZ480 = 166667, 69444, 60606, 41667, 20833
SDR144 = T.SDR[:5] + (HZ144,)
SDR165 = T.SDR[:5] + (HZ165,)
HDR240 = T.HDR[:5] + (HZ240,)
SDR480 = T.SDR[:5] + (HZ480,)


def _scalars(n):
    return [(i + 1) / (n + 1) for i in range(n)]


# 1. -- fails without the feature: "n_out outside [0, 6]" on the first period of every clip
@pytest.mark.parametrize("case,mode", [(SDR144, 2), (SDR165, 0), (HDR240, 2)], ids=["sdr-144hz-blend", "sdr-165hz-warp12", "hdr-240hz-blend"])
def test_whole_clips_at_high_rates_equal_the_sequential_filter(native_lib, case, mode):
    """Four clips with a hard cut each, one sync at the end.  The copied periods are T.COPIED whatever the rate (sequential_clip asserts it):
    they depend on the content.  Period 0 at 144 Hz is a 7-output copy period: the predicated copy runs in two chunks."""
    counts = [len(ts) for ts in T.plan(case)]
    assert max(counts) > 6 and counts[0] >= 7, counts
    got = T.run_four_clips(case, mode)
    for m, name in enumerate("ABCD"):
        ref = T.sequential_clip(case, name, mode)
        assert [k for k, (_, r) in enumerate(ref) if r["kind"] == 0] == [0, 1] + T.COPIED[name]
        T.assert_same(got[m], ref, f"member {name}")


def test_run_clips_at_480_hz(native_lib):
    """batch.run_clips at 21 / 20 outputs per period (four chunks): outputs and kinds of the sequential filter, one sync at the end."""
    from hopperrender_amd import batch as hbatch, capi
    from hopperrender_amd.calc import FlowBatch
    case, mode = SDR480, 2
    hdr, H, W, si, so, target = case
    plan = T.plan(case)
    assert [len(ts) for ts in plan[:3]] == [21, 20, 20]
    names = "ABCD"
    dev = T.upload_frames({nm: T.clip(case, nm) for nm in names})
    members = [T.calc_class(case)(H, W, si, so, search_radius=T.RADIUS, flags=capi.HF_FLAG_ASYNC | (capi.HF_FLAG_BATCH_EAGER_PLANES if i == 0 else 0))
               for i in range(4)]
    batch = FlowBatch(members)
    try:
        outs, kinds = hbatch.run_clips(batch, [[b.ptr for b in dev[nm]] for nm in names], T.SOURCE_24, target, mode, 200)
        for m, name in enumerate(names):
            ref = T.sequential_clip(case, name, mode)
            want = [f for frames, _ in ref for f in frames]
            assert kinds[m] == [("warp" if r["kind"] else "copy") for frames, r in ref for _ in frames]
            assert len(outs[m]) == len(want) == sum(len(ts) for ts in plan)
            for i, (b, w) in enumerate(zip(outs[m], want)):
                assert np.array_equal(T.valid(case, b.download(members[0].dtype)), w), (name, i, kinds[m][i])
    finally:
        batch.close()
        for c in members:
            c.close()
        for row in list(dev.values()) + (outs if "outs" in locals() else []):
            for b in row:
                b.free()


# 2.
def test_members_of_different_widths_in_one_period(native_lib):
    """Members on schedules of 60, 165, 240 and 480 Hz in one batch: chunks that hold one, two, three or all four members.  Member D has
    n_out == 0 in period 4; force_kind 1 on A's cut period (8), 0 on period 5 of cut-free C."""
    mode = 2
    names, targets = "ABCD", (HZ60, HZ165, HZ240, HZ480)
    cs = [T.SDR[:5] + (t,) for t in targets]
    plans = [list(T.plan(c)) for c in cs]
    plans[3] = [([] if k == 4 else ts) for k, ts in enumerate(plans[3])]
    assert [max(len(ts) for ts in p) for p in plans] == [3, 7, 11, 21]
    dev = T.upload_frames({nm: T.clip(T.SDR, nm) for nm in names})
    force = {8: [1, -1, -1, -1], 5: [-1, -1, 0, -1]}
    try:
        got = T.run_batch(T.SDR, mode, [dev[nm] for nm in names], lambda m, k: dev[names[m]][k].ptr, lambda m, k: plans[m][k], force=force.get)
    finally:
        for row in dev.values():
            for b in row:
                b.free()
    want = [T.sequential(cs[0], [T.clip(T.SDR, "A")], mode, plans[0], force={8: 1}),
            T.sequential(cs[1], [T.clip(T.SDR, "B")], mode, plans[1]),
            T.sequential(cs[2], [T.clip(T.SDR, "C")], mode, plans[2], force={5: 0}),
            T.sequential(cs[3], [T.clip(T.SDR, "D")], mode, plans[3])]
    assert want[0][8][1]["kind"] == 1 and want[2][5][1]["kind"] == 0 and want[3][4][0] == []
    assert [k for k, (_, r) in enumerate(want[1]) if r["kind"] == 0] == [0, 1] + T.COPIED["B"]
    assert [k for k, (_, r) in enumerate(want[3]) if r["kind"] == 0] == [0, 1] + T.COPIED["D"]
    for m in range(4):
        T.assert_same(got[m], want[m], f"member {names[m]} at {targets[m]}")


# 3.
N_OUT_CYCLE = (13, 1, 7, 6, 24)


@pytest.mark.parametrize("hdr,H,W,n,start", [(0, 180, 320, 2, 0), (0, 180, 320, 17, 0), (1, 360, 640, 2, 2), (1, 360, 640, 17, 3)],
                         ids=["sdr-2", "sdr-17", "hdr-2", "hdr-17"])
def test_the_plain_wide_calls_equal_member_by_member_periods(native_lib, hdr, H, W, n, start):
    """hf_batch_run_period_wide (period 2) and hf_batch_interpolate_period_wide (the same period again in mode 0, and in diagnostic mode 3)
    against a twin batch that updates and calculates as a batch and warps with hf_interpolate_period_ex member by member.  17 members: two
    fused launches per chunk.  n_out of member m is N_OUT_CYCLE[start + m]: (13, 1), (7, 6) and all five values.  Every member of more than
    six outputs has one NULL device_out entry in its last chunk (its internal output frame)."""
    from hopperrender_amd import capi, synth
    from hopperrender_amd.calc import FlowBatch
    cls = T.calc_class((hdr,))
    sc = synth.Scene(H, W, bool(hdr), 23)
    dev = T.upload_frames({"f": [sc.frame(k) for k in range(3)]})["f"]
    n_out = [N_OUT_CYCLE[(start + m) % len(N_OUT_CYCLE)] for m in range(n)]
    ts = [_scalars(k) for k in n_out]
    null = [k - 1 if k > 6 else None for k in n_out]                 # (a member of 13 outputs: output 12, in its third chunk)
    sides = []
    for wide in (True, False):
        members = [cls(H, W, search_radius=T.RADIUS, flags=capi.HF_FLAG_ASYNC | (capi.HF_FLAG_BATCH_EAGER_PLANES if i == 0 else 0)) for i in range(n)]
        batch = FlowBatch(members)
        outs = [T.Outputs(c) for c in members]
        internal = []
        for k in range(2):
            batch.runPeriod(batch.preparePeriod([dev[k].ptr] * n, None, None, calculate_flow=k >= 1))
        for mode in (2, 0, 3):
            ptrs = [outs[m].new(n_out[m]) for m in range(n)]
            for m in range(n):
                if null[m] is not None:
                    ptrs[m][null[m]] = 0
            if wide:
                if mode == 2:
                    prepared = batch.preparePeriod([dev[2].ptr] * n, ts, ptrs, mode)
                    assert len(prepared) == 7 and prepared[2] == max(n_out)
                    batch.runPeriod(prepared)
                else:
                    batch.interpolatePeriod(ts, ptrs, mode)
            else:
                if mode == 2:
                    batch.updateFramesDeviceRef([dev[2].ptr] * n)
                    batch.calculateOpticalFlow()
                for m, c in enumerate(members):
                    c.interpolateOnly(ts[m], ptrs[m], mode)
            batch.sync()
            internal.append([T.valid((hdr, H, W, 0, 0), c.downloadFrame()).copy() for c in members])
        frames = [o.read((hdr, H, W, 0, 0)) for o in outs]          # [member][call][output]
        sides.append((frames, internal))
        batch.close()
        for c in members:
            c.close()
        for o in outs:
            o.free()
    for b in dev:
        b.free()
    (fw, iw), (fm, im) = sides
    for m in range(n):
        for call in range(3):
            if null[m] is not None:
                assert np.array_equal(iw[call][m], im[call][m]), f"member {m} call {call}: the internal output frame differs"
            for i in range(n_out[m]):
                if i != null[m]:
                    assert np.array_equal(fw[m][call][i], fm[m][call][i]), f"member {m} (n_out {n_out[m]}) call {call} output {i} differs"
    if n_out[0] > 7:
        assert not np.array_equal(fw[0][0][0], fw[0][0][7])          # (outputs of different chunks are different frames)


def test_lists_longer_than_24_raise_the_librarys_error(native_lib):
    from hopperrender_amd import capi
    from hopperrender_amd.calc import FlowBatch, OpticalFlowCalcSDR
    members = [OpticalFlowCalcSDR(180, 320, flags=capi.HF_FLAG_ASYNC) for _ in range(2)]
    batch = FlowBatch(members)
    try:
        with pytest.raises(capi.HopperFlowError) as e:
            batch.interpolatePeriod([_scalars(25), _scalars(2)], [[0] * 25, [0] * 2], 2)
        assert e.value.code == capi.HF_ERR_INVALID_ARGUMENT and "row outside [1, 24]" in str(e.value)
    finally:
        batch.close()
        for c in members:
            c.close()


# 4.
def _planar_period(pair, k, n_outs, auto=False, force=None):
    """Period k on both batches of the pair.  The plain call warps from the third frame on (before that the ring holds frames nobody
    wrote); the auto call delivers every period -- the first two are copies of the valid columns."""
    fp, fq = pair.feed(k)
    warp = auto or k >= 2
    op, oq = pair.new_outputs(n_outs) if warp else (None, None)
    sc = [_scalars(x) for x in n_outs] if warp else None
    if auto:
        pair.bp.runPeriodAuto(fp, sc, op, 2, force)
        pair.bq.runPeriodAuto(fq, sc, oq, 2, force)
    else:
        for b, f, o in ((pair.bp, fp, op), (pair.bq, fq, oq)):
            prepared = b.preparePeriod(f, sc, o, 2, calculate_flow=k >= 1)
            assert len(prepared) == (7 if warp else 6)
            b.runPeriod(prepared)
    pair.bp.sync(); pair.bq.sync()
    if warp:
        pair.check_outputs(-1, f"period {k}")
    if k >= 1:
        pair.check_state(what=f"period {k}")


@pytest.mark.parametrize("name", ["ragged-sdr", "basic-hdr"])
def test_planar_outputs_of_wide_periods(native_lib, name):
    """HF_FLAG_BATCH_PLANAR_IN | _OUT with 7 and 11 outputs: the planar re-layout of the plain twin batch's outputs; a member never owns
    more than six stages, so the second chunk's warps reuse the stages the first chunk's conversion has read."""
    pair = P.Pair(P.cases.case(name), P.BIN | P.BOUT, 5)
    try:
        for k in range(5):
            _planar_period(pair, k, (7, 11) if k != 3 else (11, 7))
    finally:
        pair.close()


def test_planar_outputs_of_wide_auto_periods_with_a_cut(native_lib):
    """The auto call on a planar batch: per chunk the predicated copy writes the stages ahead of the chunk's conversion.  Periods 0 and 1
    are copies (m_frameCount < 3), the cut at frame 4 is a copy period, and a copy is forced on member 1 in period 3."""
    c = P.cases.Case("auto-wide", 180, 320, 320, 320, 0, (0, 0), (0, 0))
    pair = P.Pair(c, P.EAGER | P.BIN | P.BOUT, 7, cut_at=4, levels=(16.0, 235.0), seeds=[42, 7])
    try:
        for b in (pair.bp, pair.bq):
            for m in range(2):
                b.sceneSet(m, T.SOURCE_24, 200)
        for k in range(7):
            _planar_period(pair, k, (7, 11), auto=True, force=[-1, 0] if k == 3 else None)
        rp, rq = [pair.bp.sceneRead(m) for m in range(2)], [pair.bq.sceneRead(m) for m in range(2)]
        assert rp == rq and all(len(r) == 7 for r in rp)
        assert all([x["kind"] for x in r[:3]] == [0, 0, 1] for r in rp) and rp[0][3]["kind"] == 1 and rp[1][3]["kind"] == 0, rp
    finally:
        pair.close()


# 5.
def test_wide_periods_on_a_batch_that_defers_its_planes(native_lib):
    """Three 2160p HDR members, three periods of hf_batch_run_period_wide with 7 outputs: chunk 0 goes out ahead of the chain and builds the
    planes; output 7 of member 1 sits 4 bytes off 16-byte alignment, so chunk 1 does not qualify for the fused launch and must follow the
    chain member by member (it reads flow buffer 0).  Everything equals the HF_FLAG_BATCH_EAGER_PLANES twin."""
    from hopperrender_amd import capi, synth
    from hopperrender_amd.calc import DeviceBuffer, FlowBatch, OpticalFlowCalcHDR
    H, W, n, n_out = 2160, 3840, 3, 7
    sc = synth.Scene(H, W, True, 77)
    dev = T.upload_frames({"f": [sc.frame(k) for k in range(5)]})["f"]
    ts = [_scalars(n_out)] * n
    logs = []
    for flags in (capi.HF_FLAG_ASYNC | capi.HF_FLAG_BATCH_EAGER_PLANES, capi.HF_FLAG_ASYNC):
        members = [OpticalFlowCalcHDR(H, W, search_radius=8, flags=flags) for _ in range(n)]
        batch = FlowBatch(members)
        assert batch.defersPlanes() == (not flags & capi.HF_FLAG_BATCH_EAGER_PLANES)
        bufs = [[DeviceBuffer(members[0].output_frame_bytes + 16) for _ in range(n_out)] for _ in range(n)]
        ptrs = [[b.ptr + (4 if (m, i) == (1, 6) else 0) for i, b in enumerate(row)] for m, row in enumerate(bufs)]
        log = []
        for k in range(5):
            frames = [dev[(k + m) % 5].ptr for m in range(n)]                # members see the clip at different offsets
            warp = k >= 2
            prepared = batch.preparePeriod(frames, ts if warp else None, ptrs if warp else None, 2, calculate_flow=k >= 1)
            assert len(prepared) == (7 if warp else 6)
            batch.runPeriod(prepared)
            batch.sync()
            if warp:
                rec = {"planes": [c.readPhasePlane(1) for c in members], "flows": [c.readBlurredFlow(1).copy() for c in members],
                       "delta": [c.m_totalFrameDelta for c in members],
                       "outs": [[b.download(np.uint8)[off:off + members[0].output_frame_bytes].copy()
                                 for b, off in zip(row, [p - b.ptr for p, b in zip(prow, row)])] for row, prow in zip(bufs, ptrs)]}
                log.append(rec)
        logs.append(log)
        batch.close()
        for c in members:
            c.close()
        for row in bufs:
            for b in row:
                b.free()
    for b in dev:
        b.free()
    eager, lazy = logs
    assert len(eager) == len(lazy) == 3
    for k, (a, b) in enumerate(zip(eager, lazy)):
        for m in range(n):
            (pa, ca), (pb, cb) = a["planes"][m], b["planes"][m]
            assert ca and cb, (k, m)                                  # the older frame's plane is complete after each period
            assert np.array_equal(pa, pb), (k, m)
            assert np.array_equal(a["flows"][m], b["flows"][m]), (k, m)
            assert a["delta"][m] == b["delta"][m], (k, m)
            for i in range(n_out):
                assert np.array_equal(a["outs"][m][i], b["outs"][m][i]), (k, m, i)
        assert not np.array_equal(b["outs"][0][5], b["outs"][0][6])
    assert not np.array_equal(lazy[0]["outs"][1][6], lazy[1]["outs"][1][6])


# 6.
def _rc(batch, rc, code, *words):
    msg = (batch._lib.hf_batch_last_error(batch._b) or b"").decode()
    assert rc == code, (rc, msg)
    for w in words:
        assert w in msg, msg


def _arrays(n, row, counts, outs):
    cnt = (C.c_int * n)(*counts)
    t = (C.c_float * (n * max(row, 1)))(*([0.5] * (n * max(row, 1))))
    o = (C.c_void_p * (n * max(row, 1)))(*([outs[0][0].ptr] * (n * max(row, 1))))
    return cnt, t, o


def test_refusals_enqueue_nothing(native_lib):
    """row 0 and 25, n_out[m] > row, a seventh output through the narrow calls, the wide auto call on a deferring batch: refused with the
    narrow calls' codes, and the plain path then repeats its earlier outputs (T._plain_periods: same ring frames, same previous flow -- only
    if nothing was enqueued or moved)."""
    from hopperrender_amd import capi
    from hopperrender_amd.calc import DeviceBuffer, FlowBatch, OpticalFlowCalcHDR, OpticalFlowCalcSDR
    rng = np.random.default_rng(1)
    INVALID, STATE = capi.HF_ERR_INVALID_ARGUMENT, capi.HF_ERR_STATE

    def setup(cls, H, W, n, leader_flags=0):
        members = [cls(H, W, search_radius=T.RADIUS, flags=capi.HF_FLAG_ASYNC | (leader_flags if i == 0 else 0)) for i in range(n)]
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

    members, batch, dev, outs = setup(OpticalFlowCalcSDR, 180, 320, 2, capi.HF_FLAG_BATCH_EAGER_PLANES)
    L, B = batch._lib, batch._b
    first = T._plain_periods(batch, members, dev, outs, 0)
    for m in range(2):
        batch.sceneSet(m, T.SOURCE_24, -1)
    frames = (C.c_void_p * 2)(dev[0].ptr, dev[0].ptr)
    for row in (0, 25, -1):
        cnt, t, o = _arrays(2, row, [1, 1], outs)
        _rc(batch, L.hf_batch_interpolate_period_wide(B, row, cnt, t, o, 2), INVALID, "row outside [1, 24]")
        _rc(batch, L.hf_batch_run_period_wide(B, frames, 1, row, cnt, t, o, 2), INVALID, "row outside [1, 24]")
        _rc(batch, L.hf_batch_run_period_auto_wide(B, frames, row, cnt, t, o, 2, None), INVALID, "row outside [1, 24]")
    cnt, t, o = _arrays(2, 7, [7, 8], outs)                           # n_out[1] > row
    _rc(batch, L.hf_batch_interpolate_period_wide(B, 7, cnt, t, o, 2), INVALID, "n_out outside [0, 7]")
    _rc(batch, L.hf_batch_run_period_wide(B, None, 0, 7, cnt, t, o, 2), INVALID, "n_out outside [0, 7]")
    _rc(batch, L.hf_batch_run_period_auto_wide(B, frames, 7, cnt, t, o, 2, None), INVALID, "n_out outside [0, 7]")
    cnt, t, o = _arrays(2, 24, [25, 1], outs)
    _rc(batch, L.hf_batch_interpolate_period_wide(B, 24, cnt, t, o, 2), INVALID, "n_out outside [0, 24]")
    cnt, t, o = _arrays(2, 7, [2, 7], outs)                           # the narrow calls keep refusing a seventh output
    _rc(batch, L.hf_batch_interpolate_period(B, cnt, t, o, 2), INVALID, "n_out outside [0, 6]")
    _rc(batch, L.hf_batch_run_period(B, None, 0, cnt, t, o, 2), INVALID, "n_out outside [0, 6]")
    _rc(batch, L.hf_batch_run_period_auto(B, frames, cnt, t, o, 2, None), INVALID, "n_out outside [0, 6]")
    cnt, t, o = _arrays(2, 7, [7, 7], outs)                           # what the narrow auto call checks, in the wide one: force_kind, a blending scalar
    _rc(batch, L.hf_batch_run_period_auto_wide(B, frames, 7, cnt, t, o, 2, (C.c_int32 * 2)(-1, 2)), INVALID, "force_kind")
    t[7 + 6] = 1.5
    _rc(batch, L.hf_batch_run_period_auto_wide(B, frames, 7, cnt, t, o, 2, None), INVALID, "blending scalar")
    _rc(batch, L.hf_batch_interpolate_period_wide(B, 7, cnt, t, o, 2), INVALID, "blending scalar")
    assert [c.m_frameCount for c in members] == [3, 3]
    assert batch.sceneRead(0) == [] and batch.sceneRead(1) == []     # no record was written
    again = T._plain_periods(batch, members, dev, outs, 3)
    assert all(np.array_equal(a, b) for ra, rb in zip(first, again) for a, b in zip(ra, rb))
    teardown(members, batch, dev, outs)

    # a batch that defers its phase planes (three 2160p HDR members: the smallest that does): HF_ERR_STATE, as the narrow auto call
    members, batch, dev, outs = setup(OpticalFlowCalcHDR, 2160, 3840, 3)
    assert batch.defersPlanes()
    first = T._plain_periods(batch, members, dev, outs, 0)
    for m in range(3):
        batch.sceneSet(m, T.SOURCE_24, -1)
    cnt, t, o = _arrays(3, 7, [7, 7, 7], outs)
    frames = (C.c_void_p * 3)(*[dev[0].ptr] * 3)
    _rc(batch, batch._lib.hf_batch_run_period_auto_wide(batch._b, frames, 7, cnt, t, o, 2, None), STATE, "defers", "HF_FLAG_BATCH_EAGER_PLANES")
    again = T._plain_periods(batch, members, dev, outs, 3)
    assert all(np.array_equal(a, b) for ra, rb in zip(first, again) for a, b in zip(ra, rb))
    teardown(members, batch, dev, outs)
