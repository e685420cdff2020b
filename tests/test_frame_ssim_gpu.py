"""GPU: the device's windowed SSIM (hf_frame_ssim_enqueue / _read / hf_frame_ssim, csrc/hf_metrics.hip) against the numpy model of
tests/frame_ssim_model.py.  Integer losses: every field of every plane must be EQUAL.  Frames are made on the host and uploaded."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from frame_error_model import frame_error  # noqa: E402
from frame_ssim_cases import RAGGED, Dev, check_floats, ints, n_el, random_frame, run_layout_case  # noqa: E402
from frame_ssim_model import frame_ssim  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

INVALID, STATE = -1, -5   # HF_ERR_INVALID_ARGUMENT, HF_ERR_STATE
ZERO = {"sum_loss_q32": 0, "max_loss_q32": 0, "count": 0}


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
def test_layouts_strides_offsets_and_remainders(ctx, dev, hdr, planar):
    """70 x 38 (w & 3 = h & 3 = 2, chroma 35 x 19) with strides 70 / 74 / 80 on either side, bases at the allocation and 2 elements into
    it, every element random INCLUDING the padding and the unused remainder; then the smallest planes: 4 x 4 has no window, 8 x 8 one luma
    window and no chroma window, 16 x 16 nine and one."""
    H, W, strides = RAGGED
    want = run_layout_case(ctx(hdr, H, W), dev, hdr, planar, H, W, strides, seed=11 + 2 * hdr + planar)
    assert [want[0][p]["count"] for p in "YUV"] == [16 * 8, 7 * 3, 7 * 3]
    for S, counts in ((4, [0, 0, 0]), (8, [1, 0, 0]), (16, [9, 1, 1])):
        want = run_layout_case(ctx(hdr, S, S), dev, hdr, planar, S, S, ((S, S), (S, 16), (16, 16)), seed=S)
        assert [want[0][p]["count"] for p in "YUV"] == counts
        assert all(want[0][p] == ZERO for p, n in zip("YUV", counts) if n == 0)
        assert all(want[0][p]["sum_loss_q32"] > 0 for p, n in zip("YUV", counts) if n)


@pytest.mark.parametrize("planar", [False, True], ids=["semi", "planar"])
@pytest.mark.parametrize("hdr", [False, True], ids=["sdr", "hdr"])
def test_more_than_one_tile_each_way_with_a_ragged_last_tile(ctx, dev, hdr, planar):
    """A workgroup's tile is 31 sixteen-byte units by 15 block rows of windows: at most 124 x 15 windows, 496 x 60 elements.  1018 x 262
    has 253 x 64 luma windows (8 bit: two tiles and five windows across, four and four down) and 126 x 31 chroma windows (two tiles and two
    across where U and V share a unit, two and one down).  A window dropped or counted twice at a seam changes count or the sums.  Stride
    1024: wide loads; stride 1018 on one side: element by element."""
    H, W = 262, 1018
    want = run_layout_case(ctx(hdr, H, W), dev, hdr, planar, H, W, ((1024, 1024), (1018, 1024)), offsets=(0,), seed=3)
    assert [want[0][p]["count"] for p in "YUV"] == [253 * 64, 126 * 31, 126 * 31]


@pytest.mark.parametrize("planar", [False, True], ids=["semi", "planar"])
@pytest.mark.parametrize("hdr", [False, True], ids=["sdr", "hdr"])
def test_single_differences_land_in_their_plane(ctx, dev, hdr, planar):
    """One flipped element in the last USED luma column and row (67, 35 of 70 x 38) changes Y only; one in U only U, one in V only V, in
    both layouts; differences confined to the padding and to the unused w & 3 columns / h & 3 rows give all zeros."""
    H, W, S = 38, 70, 80
    c = ctx(hdr, H, W)
    base = random_frame(np.random.default_rng(5), hdr, H, S)
    hc, sc = H // 2, S // 2
    top = 65535 if hdr else 255

    def flip(*idx):
        f = base.copy()
        for i in idx:
            f[i] = top - f[i]   # differs from base[i] for every value (top is odd)
        return f
    uw, uh = (W >> 2) * 4, (H >> 2) * 4                    # used luma extent 68 x 36
    cw, ch = ((W // 2) >> 2) * 4, ((H // 2) >> 2) * 4      # used chroma extent 32 x 16 of 35 x 19
    if planar:
        u_at = lambda y, x: H * S + y * sc + x
        v_at = lambda y, x: H * S + hc * sc + y * sc + x
        pad = [u_at(0, W // 2), v_at(3, W // 2 + 1)]
    else:
        u_at = lambda y, x: H * S + y * S + 2 * x
        v_at = lambda y, x: H * S + y * S + 2 * x + 1
        pad = [H * S + W, H * S + 5 * S + W + 1]
    pb = dev.put(base)
    cases = {"Y": flip((uh - 1) * S + uw - 1), "U": flip(u_at(ch - 1, cw - 1)), "V": flip(v_at(ch - 1, cw - 1))}
    for plane, f in cases.items():
        got = ints(c.frameSsim(dev.put(f), pb, S, S, planar))
        assert got == frame_ssim(f, base, H, W, S, S, planar)
        assert [got[p]["sum_loss_q32"] > 0 for p in "YUV"] == [p == plane for p in "YUV"], plane
        assert got[plane]["max_loss_q32"] == got[plane]["sum_loss_q32"]   # the last used block lies in one window only
    unused = [(H - 1) * S + 3, (uh) * S + uw - 1, 5 * S + uw, 5 * S + W - 1, (H - 1) * S + W,          # luma: remainder rows, columns, padding
              u_at(ch, 0), u_at(hc - 1, cw - 1), u_at(2, cw), v_at(ch, 3), v_at(1, W // 2 - 1)] + pad   # chroma: the same
    got = ints(c.frameSsim(dev.put(flip(*unused)), pb, S, S, planar))
    assert got == {"Y": dict(ZERO, count=16 * 8), "U": dict(ZERO, count=7 * 3), "V": dict(ZERO, count=7 * 3)}


def test_magnitudes_at_16_bits(ctx, dev):
    """256 x 128 P010: 0 against 65535 (every window 4294960585) and the anti-checkerboard a = 65535 ((x + y) & 1) against 65535 - a
    (ssim about -0.9965: every luma window 8574741222, a loss above 2^32; U and V of an interleaved checkerboard are stripes)."""
    H, W = 128, 256
    c = ctx(True, H, W)
    n = n_el(H, W)
    lo, hi = np.zeros(n, np.uint16), np.full(n, 65535, np.uint16)
    got = ints(c.frameSsim(dev.put(lo), dev.put(hi)))
    assert got == frame_ssim(lo, hi, H, W)
    for p, cnt in (("Y", 63 * 31), ("U", 31 * 15), ("V", 31 * 15)):
        assert got[p] == {"sum_loss_q32": cnt * 4294960585, "max_loss_q32": 4294960585, "count": cnt}, p
    y, x = np.mgrid[0:H + H // 2, 0:W]
    a = (65535 * ((x + y) & 1)).astype(np.uint16).reshape(-1)
    got = ints(c.frameSsim(dev.put(a), dev.put(65535 - a)))
    assert got == frame_ssim(a, 65535 - a, H, W)
    assert got["Y"] == {"sum_loss_q32": 63 * 31 * 8574741222, "max_loss_q32": 8574741222, "count": 63 * 31}


def test_zero_against_65535_at_2160p(ctx, dev):
    """3840 x 2160 P010, where a workgroup walks many tiles and the sums are large: 959 x 539 luma windows of 4294960585 each."""
    H, W = 2160, 3840
    c = ctx(True, H, W)
    n = n_el(H, W)
    got = ints(c.frameSsim(dev.put(np.zeros(n, np.uint16)), dev.put(np.full(n, 65535, np.uint16))))
    for p, cnt in (("Y", 959 * 539), ("U", 479 * 269), ("V", 479 * 269)):
        assert got[p] == {"sum_loss_q32": cnt * 4294960585, "max_loss_q32": 4294960585, "count": cnt}, p


def test_peaks(ctx, dev):
    """peak = 0 on planar 16-bit frames is 1023 (LSB-aligned yuv420p10le) and an explicit 1023 is the same; an explicit 65535 there and an
    explicit 100 or 255 on 8 bit follow the model with those constants."""
    H, W = 38, 70
    rng = np.random.default_rng(21)
    a, b = random_frame(rng, True, H, W, 1023), random_frame(rng, True, H, W, 1023)
    c = ctx(True, H, W)
    pa, pb = dev.put(a), dev.put(b)
    want = frame_ssim(a, b, H, W, planar=True, peak=1023)
    assert ints(c.frameSsim(pa, pb, planar=True)) == want == ints(c.frameSsim(pa, pb, planar=True, peak=1023))
    assert ints(c.frameSsim(pa, pb, planar=True, peak=65535)) == frame_ssim(a, b, H, W, planar=True, peak=65535) != want
    assert ints(c.frameSsim(pa, pb, planar=False, peak=1023)) == frame_ssim(a, b, H, W, peak=1023)
    z, full = np.zeros(n_el(H, W), np.uint16), np.full(n_el(H, W), 1023, np.uint16)
    assert ints(c.frameSsim(dev.put(z), dev.put(full), planar=True))["Y"] == {"sum_loss_q32": 128 * 4294960585, "max_loss_q32": 4294960585, "count": 128}
    a8, b8 = random_frame(rng, False, H, W, 100), random_frame(rng, False, H, W, 100)
    c8 = ctx(False, H, W)
    pa, pb = dev.put(a8), dev.put(b8)
    for peak in (100, 255, 16):
        assert ints(c8.frameSsim(pa, pb, peak=peak)) == frame_ssim(a8, b8, H, W, peak=peak), peak
    assert ints(c8.frameSsim(pa, pb)) == frame_ssim(a8, b8, H, W, peak=255)


@pytest.mark.parametrize("n", [1, 7, 192])
def test_pairs_per_launch(ctx, dev, n):
    """1, 7 and HF_MAX_ERROR_PAIRS pairs in one launch; distinct content per pair."""
    H, W = 38, 70
    c = ctx(False, H, W)
    rng = np.random.default_rng(n)
    uniq = [random_frame(rng, False, H, W) for _ in range(8)]
    ptrs = [dev.put(f) for f in uniq]
    ia, ib = rng.integers(0, 8, size=n), rng.integers(0, 8, size=n)
    c.frameSsimEnqueue([ptrs[i] for i in ia], [ptrs[i] for i in ib], 256 - n)
    got = c.frameSsimRead(256 - n, n)
    model = {}
    for k, (i, j) in enumerate(zip(ia, ib)):
        if (i, j) not in model:
            model[(i, j)] = frame_ssim(uniq[i], uniq[j], H, W)
        assert ints(got[k]) == model[(i, j)], k


def test_slots_are_zeroed_per_call_independent_and_apart_from_the_error_slots(ctx, dev):
    """The same slot used twice holds the second result; disjoint ranges are independent; hf_frame_error_enqueue on the same slot numbers
    in between leaves both sets of results right."""
    H, W = 38, 70
    c = ctx(True, H, W)
    rng = np.random.default_rng(3)
    f = [random_frame(rng, True, H, W) for _ in range(5)]
    p = [dev.put(x) for x in f]
    S = lambda i, j: frame_ssim(f[i], f[j], H, W)
    E = lambda i, j: frame_error(f[i], f[j], H, W)
    rd = lambda first, n: [ints(g) for g in c.frameSsimRead(first, n)]
    c.frameSsimEnqueue([p[0]], [p[1]], 10)
    c.frameSsimEnqueue([p[2]], [p[3]], 10)
    assert rd(10, 1) == [S(2, 3)]
    c.frameSsimEnqueue([p[0], p[1]], [p[4], p[4]], 0)
    c.frameErrorEnqueue([p[3], p[2]], [p[4], p[4]], 0)
    c.frameSsimEnqueue([p[2], p[3], p[0]], [p[4], p[4], p[0]], 2)
    c.frameErrorEnqueue([p[1]], [p[0]], 2)
    assert rd(0, 5) == [S(0, 4), S(1, 4), S(2, 4), S(3, 4), S(0, 0)]
    assert c.frameErrorRead(0, 3) == [E(3, 4), E(2, 4), E(1, 0)]
    c.frameSsimEnqueue([p[1]], [p[2]], 2)
    assert rd(0, 5) == [S(0, 4), S(1, 4), S(1, 2), S(3, 4), S(0, 0)]
    assert c.frameErrorRead(0, 3) == [E(3, 4), E(2, 4), E(1, 0)]
    assert S(0, 0)["Y"] == dict(ZERO, count=128)


def test_error_returns_enqueue_nothing(native_lib, dev):
    """_read before any enqueue is HF_ERR_STATE; every refusal is HF_ERR_INVALID_ARGUMENT, names its call and leaves all 256 slots as they were."""
    from hopperrender_amd import capi
    from hopperrender_amd.calc import OpticalFlowCalcHDR, OpticalFlowCalcSDR
    H, W = 38, 70
    L = capi.load()
    rng = np.random.default_rng(9)
    fa, fb = random_frame(rng, False, H, 80), random_frame(rng, False, H, 80)
    pa, pb = dev.put(fa), dev.put(fb)
    c, c16 = OpticalFlowCalcSDR(H, W, flags=capi.HF_FLAG_ASYNC), OpticalFlowCalcHDR(H, W, flags=capi.HF_FLAG_ASYNC)
    try:
        outs = (capi.HfFrameSsim * 2)()
        assert L.hf_frame_ssim_read(c._ctx, 0, 1, outs) == STATE and b"hf_frame_ssim_read" in L.hf_last_error(c._ctx)
        c.frameSsimEnqueue([pa] * 4, [pb] * 4, 0, 80, 80)
        c.frameSsimEnqueue([pa] * 4, [pb] * 4, 252, 80, 80)
        before = c.frameSsimRead(0, 256)
        assert ints(before[0]) == frame_ssim(fa, fb, H, W, 80, 80) and before[255] == before[0] and ints(before[100]) == {p: ZERO for p in "YUV"}
        tab = lambda *ps: (C.c_void_p * len(ps))(*ps)
        A, B, hole = tab(pa, pa), tab(pb, pb), tab(pa, None)
        big = (C.c_void_p * 193)(*([pa] * 193))
        enq = lambda n, a, b, sa, sb, planar, slot, peak=0, cc=c: L.hf_frame_ssim_enqueue(cc._ctx, n, a, b, sa, sb, planar, peak, slot)
        bad = {
            "null a": enq(2, None, B, 80, 80, 0, 0), "null b": enq(2, A, None, 80, 80, 0, 0),
            "null entry a": enq(2, hole, B, 80, 80, 0, 0), "null entry b": enq(2, A, hole, 80, 80, 0, 0),
            "n = 0": enq(0, A, B, 80, 80, 0, 0), "n < 0": enq(-1, A, B, 80, 80, 0, 0), "n = 193": enq(193, big, big, 80, 80, 0, 0),
            "slot < 0": enq(2, A, B, 80, 80, 0, -1), "slot range past 256": enq(2, A, B, 80, 80, 0, 255), "slot 256": enq(1, A, B, 80, 80, 0, 256),
            "stride a below W": enq(2, A, B, 69, 80, 0, 0), "stride b below W": enq(2, A, B, 80, 68, 0, 0),
            "odd planar stride a": enq(2, A, B, 71, 80, 1, 0), "odd planar stride b": enq(2, A, B, 80, 79, 1, 0),
            "peak < 0": enq(2, A, B, 80, 80, 0, 0, -1), "peak 256 on 8 bit": enq(2, A, B, 80, 80, 0, 0, 256), "peak 1023 on 8 bit": enq(2, A, B, 80, 80, 1, 0, 1023),
            "peak 65536 on 16 bit": enq(2, A, B, 80, 80, 0, 0, 65536, c16),
            "null context": L.hf_frame_ssim_enqueue(None, 2, A, B, 80, 80, 0, 0, 0),
        }
        assert b"hf_frame_ssim_enqueue" in L.hf_last_error(c16._ctx) and b"peak" in L.hf_last_error(c16._ctx)
        assert L.hf_frame_ssim_read(c16._ctx, 0, 1, outs) == STATE   # (the refused call allocated and enqueued nothing)
        out = capi.HfFrameSsim()
        bad["one pair: null a"] = L.hf_frame_ssim(c._ctx, None, pb, 80, 80, 0, 0, C.byref(out))
        bad["one pair: null b"] = L.hf_frame_ssim(c._ctx, pa, None, 80, 80, 0, 0, C.byref(out))
        bad["one pair: null out"] = L.hf_frame_ssim(c._ctx, pa, pb, 80, 80, 0, 0, None)
        bad["one pair: stride"] = L.hf_frame_ssim(c._ctx, pa, pb, 80, 60, 0, 0, C.byref(out))
        bad["one pair: odd planar stride"] = L.hf_frame_ssim(c._ctx, pa, pb, 81, 80, 1, 0, C.byref(out))
        bad["one pair: peak"] = L.hf_frame_ssim(c._ctx, pa, pb, 80, 80, 0, 300, C.byref(out))
        assert b"hf_frame_ssim:" in L.hf_last_error(c._ctx)
        bad["read: null out"] = L.hf_frame_ssim_read(c._ctx, 0, 2, None)
        bad["read: n = 0"] = L.hf_frame_ssim_read(c._ctx, 0, 0, outs)
        bad["read: range"] = L.hf_frame_ssim_read(c._ctx, 255, 2, outs)
        bad["read: slot < 0"] = L.hf_frame_ssim_read(c._ctx, -1, 2, outs)
        assert {k: v for k, v in bad.items() if v != INVALID} == {}
        assert b"hf_frame_ssim_read" in L.hf_last_error(c._ctx)
        assert c.frameSsimRead(0, 256) == before
        with pytest.raises(capi.HopperFlowError) as e:
            c.frameSsimEnqueue([pa], [pb], 0, 80, 80, peak=256)
        assert e.value.code == INVALID
        assert c.frameSsimRead(0, 256) == before
    finally:
        c.close()
        c16.close()


def test_batch_member_scores_its_periods_outputs_without_a_sync(native_lib, dev):
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
        calcs[1].frameSsimEnqueue([outs[m][i].ptr for m in range(n) for i in range(2)], [tptr[m][i] for m in range(n) for i in range(2)], 100)
        got = calcs[1].frameSsimRead(100, 6)
        batch.sync()
        k = 0
        for m in range(n):
            for i in range(2):
                o = outs[m][i].download(np.uint8)
                assert ints(got[k]) == frame_ssim(o, truth[m][i], H, W), (m, i)
                assert got[k]["Y"]["sum_loss_q32"] > 0 and got[k]["Y"]["count"] == 159 * 89
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
        c.frameSsimEnqueue([outs[1].ptr, outs[0].ptr], [p[2], p[2]], 0)
        got = c.frameSsimRead(0, 2)
        assert ints(got[0]) == frame_ssim(outs[1].download(np.uint16), f[2], H, W)
        assert ints(got[1]) == frame_ssim(outs[0].download(np.uint16), f[2], H, W)
        assert got[0]["Y"]["sum_loss_q32"] > 0
        check_floats(got[0])
    finally:
        c.close()
        for b in outs:
            b.free()


CHILD = r"""
import sys, ctypes as C
sys.path.insert(0, {root!r}); sys.path.insert(0, {root!r} + "/tests")
from hopperrender_amd import capi
from hopperrender_amd.calc import OpticalFlowCalcHDR, OpticalFlowCalcSDR
from frame_ssim_cases import RAGGED, Dev, run_layout_case

def violations(c):
    n = C.c_uint32(0); first = (C.c_uint32 * 4)()
    capi.check(c._lib.hf_debug_bounds_violations(c._ctx, C.byref(n), first, 0), c._ctx)
    return n.value, list(first)

H, W, strides = RAGGED
dev = Dev()
for hdr in (False, True):
    c = (OpticalFlowCalcHDR if hdr else OpticalFlowCalcSDR)(H, W, flags=capi.HF_FLAG_ASYNC)
    assert violations(c) == (0, [0, 0, 0, 0])
    for planar in (False, True):
        run_layout_case(c, dev, hdr, planar, H, W, strides, seed=11 + 2 * hdr + planar)
        assert violations(c)[0] == 0, (hdr, planar, violations(c))
    c.close()
dev.free()
print("SSIM-DEBUG-BOUNDS-OK")
"""


def test_ragged_layouts_under_the_bounds_checking_build(native_lib):
    """The ragged 70 x 38 case with every stride pair and both base offsets, all four kernels, in a fresh child process under
    libhopperflow_dbg.so (every load of the kernel checked against its frame's extent): the same results and zero violations."""
    from hopperrender_amd import build
    dbg = build.build_flow(debug_bounds=True)
    env = dict(os.environ, HF_LIB=dbg)
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT)], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0 and "SSIM-DEBUG-BOUNDS-OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
