"""GPU: the device's frame error sums (hf_frame_error_enqueue / _read / hf_frame_error, csrc/hf_metrics.hip) against the numpy model of
tests/frame_error_model.py.  Integer sums: every field of every plane must be EQUAL.  Frames are made on the host and uploaded."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from frame_error_model import frame_error  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID = -1   # HF_ERR_INVALID_ARGUMENT


def _dt(hdr):
    return np.uint16 if hdr else np.uint8


def _n_el(H, S):
    return H * S + (H // 2) * S


def _random(rng, hdr, H, S):
    return rng.integers(0, 65536 if hdr else 256, size=_n_el(H, S), dtype=_dt(hdr))


class Dev:
    """Host frames on the device, optionally `off` elements into their allocation (an unaligned base)."""

    def __init__(self):
        self.bufs = []

    def put(self, a, off=0):
        from hopperrender_amd import capi
        from hopperrender_amd.calc import DeviceBuffer
        a = np.ascontiguousarray(a)
        b = DeviceBuffer(a.nbytes + 64)
        self.bufs.append(b)
        p = b.ptr + off * a.itemsize
        capi.check(capi.load().hf_memcpy_h2d(0, C.c_void_p(p), a.ctypes.data_as(C.c_void_p), a.nbytes))
        return p

    def free(self):
        for b in self.bufs:
            b.free()
        self.bufs = []


@pytest.fixture()
def dev():
    d = Dev()
    yield d
    d.free()


@pytest.fixture(scope="module")
def ctx(native_lib):
    """One context per geometry for the whole module (the calls only need its W, H and bit depth)."""
    from hopperrender_amd import capi
    from hopperrender_amd.calc import OpticalFlowCalcHDR, OpticalFlowCalcSDR
    made = {}

    def get(hdr, H, W, flags=capi.HF_FLAG_ASYNC):
        k = (hdr, H, W, flags)
        if k not in made:
            made[k] = (OpticalFlowCalcHDR if hdr else OpticalFlowCalcSDR)(H, W, flags=flags)
        return made[k]
    yield get
    for c in made.values():
        c.close()


@pytest.mark.parametrize("planar", [False, True], ids=["semi", "planar"])
@pytest.mark.parametrize("hdr", [False, True], ids=["sdr", "hdr"])
def test_layouts_strides_offsets_and_padding(ctx, dev, hdr, planar):
    """70 x 38 (ragged row tail, H/2 odd) with strides 70 / 74 / 80 on either side -- unaligned pitch, aligned pitch with padding -- bases
    at the allocation and 2 elements into it, every element random INCLUDING the padding columns (different garbage on the two sides,
    which must contribute nothing); 4 x 4 is smaller than one work item.  All pairs of a geometry go out in one launch each way."""
    rng = np.random.default_rng(11 + 2 * hdr + planar)
    for (H, W, strides) in ((38, 70, ((70, 70), (74, 80), (80, 80), (80, 74), (80, 70))), (4, 4, ((4, 4), (4, 16), (16, 16)))):
        c = ctx(hdr, H, W)
        for sa, sb in strides:
            fa = [_random(rng, hdr, H, sa) for _ in range(3)]
            fb = [_random(rng, hdr, H, sb) for _ in range(3)]
            fb[1] = fb[1].copy()
            want = [frame_error(a, b, H, W, sa, sb, planar) for a, b in zip(fa, fb)]
            for off in (0, 2):   # all bases aligned (wide accesses where the pitches allow them), then all 2 elements in (element by element)
                pa, pb = [dev.put(a, off) for a in fa], [dev.put(b, off) for b in fb]
                c.frameErrorEnqueue(pa, pb, 5, sa, sb, planar)
                got = c.frameErrorRead(5, 3)
                assert got == want, (H, W, sa, sb, off)
                assert c.frameError(pa[0], pb[0], sa, sb, planar) == want[0]
            assert want[0]["Y"]["count"] == H * W and want[0]["U"]["count"] == want[0]["V"]["count"] == (H // 2) * (W // 2)


@pytest.mark.parametrize("planar", [False, True], ids=["semi", "planar"])
@pytest.mark.parametrize("hdr", [False, True], ids=["sdr", "hdr"])
def test_single_differences_land_in_their_plane(ctx, dev, hdr, planar):
    """A difference only in the last column of the last luma row; only in U; only in V (channel assignment in both layouts); and padding
    that differs while every compared element is equal."""
    H, W, S = 38, 70, 80
    c = ctx(hdr, H, W)
    rng = np.random.default_rng(5)
    base = _random(rng, hdr, H, S)
    hc, sc = H // 2, S // 2
    top = 65535 if hdr else 255

    def flip(i):
        f = base.copy()
        f[i] = top - f[i]   # differs from base[i] for every value (top is odd)
        return f
    last_y = (H - 1) * S + (W - 1)
    if planar:
        u_last = H * S + (hc - 1) * sc + (W // 2 - 1)
        v_last = H * S + hc * sc + (hc - 1) * sc + (W // 2 - 1)
        pad = [H * S + 0 * sc + W // 2, (H - 1) * S + W]
    else:
        u_last = H * S + (hc - 1) * S + (W - 2)
        v_last = u_last + 1
        pad = [H * S + W, (H - 1) * S + W]
    cases = {"Y": flip(last_y), "U": flip(u_last), "V": flip(v_last)}
    pb = dev.put(base)
    for plane, f in cases.items():
        got = c.frameError(dev.put(f), pb, S, S, planar)
        assert got == frame_error(f, base, H, W, S, S, planar)
        assert [got[p]["n_differ"] for p in "YUV"] == [int(p == plane) for p in "YUV"], plane
        assert got[plane]["max_abs"] > 0 and got[plane]["sad"] == got[plane]["max_abs"] and got[plane]["sse"] == got[plane]["max_abs"] ** 2
    f = base.copy()
    for i in pad:
        f[i] = top - f[i]
    got = c.frameError(dev.put(f), pb, S, S, planar)
    assert all(got[p]["sse"] == 0 and got[p]["n_differ"] == 0 and got[p]["max_abs"] == 0 for p in "YUV")


def _saturated(ctx, dev, H, W):
    c = ctx(True, H, W)
    n = _n_el(H, W)
    a, b = np.zeros(n, np.uint16), np.full(n, 65535, np.uint16)
    got = c.frameError(dev.put(a), dev.put(b))
    for p, cnt in (("Y", H * W), ("U", H * W // 4), ("V", H * W // 4)):
        assert got[p] == {"sse": cnt * 65535 ** 2, "sad": cnt * 65535, "max_abs": 65535, "n_differ": cnt, "count": cnt}, p
    return got


def test_every_element_saturated_needs_64_bits(ctx, dev):
    """256 x 128 HDR, 0 against 65535 everywhere: the luma sse is 1.4e14."""
    got = _saturated(ctx, dev, 128, 256)
    assert got["Y"]["sse"] > 1 << 46


def test_every_element_saturated_at_2160p(ctx, dev):
    """... and at 3840 x 2160 HDR, where a lane sums many items and a workgroup's counts are large: luma sse 3.6e16."""
    got = _saturated(ctx, dev, 2160, 3840)
    assert got["Y"]["sse"] > 1 << 54


@pytest.mark.parametrize("n", [1, 7, 192])
def test_pairs_per_launch(ctx, dev, n):
    """1, 7 and HF_MAX_ERROR_PAIRS pairs in one launch (the x extent shrinks to 10 workgroups per pair at 192); distinct content per pair."""
    H, W = 38, 70
    c = ctx(False, H, W)
    rng = np.random.default_rng(n)
    uniq = [_random(rng, False, H, W) for _ in range(8)]
    ptrs = [dev.put(f) for f in uniq]
    ia, ib = rng.integers(0, 8, size=n), rng.integers(0, 8, size=n)
    c.frameErrorEnqueue([ptrs[i] for i in ia], [ptrs[i] for i in ib], 256 - n)
    got = c.frameErrorRead(256 - n, n)
    model = {}
    for k, (i, j) in enumerate(zip(ia, ib)):
        if (i, j) not in model:
            model[(i, j)] = frame_error(uniq[i], uniq[j], H, W)
        assert got[k] == model[(i, j)], k


def test_slots_are_zeroed_per_call_and_ranges_are_independent(ctx, dev):
    """The same slot used twice holds the second result, not the sum of both; two enqueues on disjoint slot ranges are read together and
    a re-used range leaves its neighbours alone."""
    H, W = 38, 70
    c = ctx(True, H, W)
    rng = np.random.default_rng(3)
    f = [_random(rng, True, H, W) for _ in range(5)]
    p = [dev.put(x) for x in f]
    E = lambda i, j: frame_error(f[i], f[j], H, W)
    c.frameErrorEnqueue([p[0]], [p[1]], 10)
    c.frameErrorEnqueue([p[2]], [p[3]], 10)
    assert c.frameErrorRead(10, 1) == [E(2, 3)]
    c.frameErrorEnqueue([p[0], p[1]], [p[4], p[4]], 0)
    c.frameErrorEnqueue([p[2], p[3], p[0]], [p[4], p[4], p[0]], 2)
    assert c.frameErrorRead(0, 5) == [E(0, 4), E(1, 4), E(2, 4), E(3, 4), E(0, 0)]
    c.frameErrorEnqueue([p[1]], [p[2]], 2)
    assert c.frameErrorRead(0, 5) == [E(0, 4), E(1, 4), E(1, 2), E(3, 4), E(0, 0)]


def test_error_returns_enqueue_nothing(ctx, dev):
    """Every refusal is HF_ERR_INVALID_ARGUMENT and leaves the slots as they were."""
    from hopperrender_amd import capi
    H, W = 38, 70
    c = ctx(False, H, W)
    L = capi.load()
    rng = np.random.default_rng(9)
    fa, fb = _random(rng, False, H, 80), _random(rng, False, H, 80)
    pa, pb = dev.put(fa), dev.put(fb)
    c.frameErrorEnqueue([pa] * 4, [pb] * 4, 0, 80, 80)
    c.frameErrorEnqueue([pa] * 4, [pb] * 4, 252, 80, 80)
    before = c.frameErrorRead(0, 256)
    assert before[0] == frame_error(fa, fb, H, W, 80, 80) and before[255] == before[0]
    tab = lambda *ps: (C.c_void_p * len(ps))(*ps)
    A, B, hole = tab(pa, pa), tab(pb, pb), tab(pa, None)
    big = (C.c_void_p * 193)(*([pa] * 193))
    enq = lambda n, a, b, sa, sb, planar, slot: L.hf_frame_error_enqueue(c._ctx, n, a, b, sa, sb, planar, slot)
    bad = {
        "null a": enq(2, None, B, 80, 80, 0, 0), "null b": enq(2, A, None, 80, 80, 0, 0),
        "null entry a": enq(2, hole, B, 80, 80, 0, 0), "null entry b": enq(2, A, hole, 80, 80, 0, 0),
        "n = 0": enq(0, A, B, 80, 80, 0, 0), "n < 0": enq(-1, A, B, 80, 80, 0, 0), "n = 193": enq(193, big, big, 80, 80, 0, 0),
        "slot < 0": enq(2, A, B, 80, 80, 0, -1), "slot range past 256": enq(2, A, B, 80, 80, 0, 255), "slot 256": enq(1, A, B, 80, 80, 0, 256),
        "stride a below W": enq(2, A, B, 69, 80, 0, 0), "stride b below W": enq(2, A, B, 80, 68, 0, 0),
        "odd planar stride a": enq(2, A, B, 71, 80, 1, 0), "odd planar stride b": enq(2, A, B, 80, 79, 1, 0),
        "null context": L.hf_frame_error_enqueue(None, 2, A, B, 80, 80, 0, 0),
    }
    out = capi.HfFrameError()
    bad["one pair: null a"] = L.hf_frame_error(c._ctx, None, pb, 80, 80, 0, C.byref(out))
    bad["one pair: null b"] = L.hf_frame_error(c._ctx, pa, None, 80, 80, 0, C.byref(out))
    bad["one pair: null out"] = L.hf_frame_error(c._ctx, pa, pb, 80, 80, 0, None)
    bad["one pair: stride"] = L.hf_frame_error(c._ctx, pa, pb, 80, 60, 0, C.byref(out))
    bad["one pair: odd planar stride"] = L.hf_frame_error(c._ctx, pa, pb, 81, 80, 1, C.byref(out))
    outs = (capi.HfFrameError * 2)()
    bad["read: null out"] = L.hf_frame_error_read(c._ctx, 0, 2, None)
    bad["read: n = 0"] = L.hf_frame_error_read(c._ctx, 0, 0, outs)
    bad["read: range"] = L.hf_frame_error_read(c._ctx, 255, 2, outs)
    bad["read: slot < 0"] = L.hf_frame_error_read(c._ctx, -1, 2, outs)
    assert {k: v for k, v in bad.items() if v != INVALID} == {}
    assert b"hf_frame_error" in L.hf_last_error(c._ctx)
    assert c.frameErrorRead(0, 256) == before
    with pytest.raises(capi.HopperFlowError) as e:
        c.frameErrorEnqueue([pa], [pb], 0, 60, 80)
    assert e.value.code == INVALID


def test_batch_member_compares_its_periods_outputs_without_a_sync(native_lib, dev):
    """A FlowBatch of 3 members at 640 x 360: runPeriod with two outputs each, then the six comparisons against uploaded truths enqueued
    on a member straight away (the member issues on the batch's stream, behind the warps); equal to numpy on the frames downloaded after."""
    from hopperrender_amd import capi, synth
    from hopperrender_amd.calc import DeviceBuffer, FlowBatch, OpticalFlowCalcSDR
    H, W, n = 360, 640, 3
    scenes = [synth.Scene(H, W, False, 40 + m) for m in range(n)]
    frames = [[sc.frame(k) for k in range(5)] for sc in scenes]
    calcs = [OpticalFlowCalcSDR(H, W, search_radius=8, flags=capi.HF_FLAG_ASYNC) for _ in range(n)]
    ptr = [[dev.put(frames[m][k]) for k in (0, 2, 4)] for m in range(n)]
    truth = [[frames[m][1], frames[m][3]] for m in range(n)]
    tptr = [[dev.put(t) for t in truth[m]] for m in range(n)]
    outs = [[DeviceBuffer(calcs[0].output_frame_bytes) for _ in range(2)] for _ in range(n)]
    batch = FlowBatch(calcs)
    try:
        for k in range(2):
            batch.runPeriod(batch.preparePeriod([ptr[m][k] for m in range(n)], None, None))
        batch.runPeriod(batch.preparePeriod([ptr[m][2] for m in range(n)], [[0.25, 0.5]] * n, [[b.ptr for b in o] for o in outs]))
        calcs[1].frameErrorEnqueue([outs[m][i].ptr for m in range(n) for i in range(2)], [tptr[m][i] for m in range(n) for i in range(2)], 100)
        got = calcs[1].frameErrorRead(100, 6)
        batch.sync()
        k = 0
        for m in range(n):
            for i in range(2):
                o = outs[m][i].download(np.uint8)
                assert got[k] == frame_error(o, truth[m][i], H, W), (m, i)
                assert got[k]["Y"]["n_differ"] > 0
                k += 1
    finally:
        batch.close()
        for c in calcs:
            c.close()
        for o in outs:
            for b in o:
                b.free()


def test_dual_stream_context_warp_then_enqueue_then_read(native_lib, dev):
    """HF_FLAG_DUAL_STREAM: the warps run on the context's second stream; the comparison is ordered behind them."""
    from hopperrender_amd import capi, synth
    from hopperrender_amd.calc import DeviceBuffer, OpticalFlowCalcHDR
    H, W = 360, 640
    sc = synth.Scene(H, W, True, 77)
    f = [sc.frame(k) for k in range(4)]
    c = OpticalFlowCalcHDR(H, W, search_radius=8, flags=capi.HF_FLAG_ASYNC | capi.HF_FLAG_DUAL_STREAM)
    outs = [DeviceBuffer(c.output_frame_bytes) for _ in range(2)]
    try:
        p = [dev.put(x) for x in f]
        c.updateFrameDeviceRef(p[0]); c.updateFrameDeviceRef(p[1])
        c.interpolatePeriod(p[2], [0.5], [outs[0].ptr])
        c.interpolatePeriod(p[3], [0.5], [outs[1].ptr])
        c.frameErrorEnqueue([outs[1].ptr, outs[0].ptr], [p[2], p[2]], 0)
        got = c.frameErrorRead(0, 2)
        assert got[0] == frame_error(outs[1].download(np.uint16), f[2], H, W)
        assert got[1] == frame_error(outs[0].download(np.uint16), f[2], H, W)
        assert got[0]["Y"]["n_differ"] > 0
    finally:
        c.close()
        for b in outs:
            b.free()
