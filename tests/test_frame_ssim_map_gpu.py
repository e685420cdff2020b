"""GPU: the device's per-tile SSIM maps (hf_frame_ssim_map_shape / _enqueue, csrc/hf_metrics.hip) against the numpy model of
tests/frame_ssim_map_model.py.  Integer losses: every field of every tile of every plane must be EQUAL.  Frames are made on the host
and uploaded; every map buffer is prefilled with 0xFF bytes and 64 guard bytes, so an entry the launch did not write, or a write past
the end, shows."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_frame_ssim_gpu as fsg  # noqa: E402
from frame_error_model import frame_error  # noqa: E402
from frame_ssim_cases import RAGGED, ints, n_el, random_frame  # noqa: E402
from frame_ssim_map_cases import maps, prefilled, run_map_layout_case, same  # noqa: E402
from frame_ssim_map_model import TILES, frame_ssim_map, map_shape, totals  # noqa: E402
from frame_ssim_model import frame_ssim  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

INVALID = -1   # HF_ERR_INVALID_ARGUMENT
dev, ctx = fsg.dev, fsg.ctx   # the fixtures of the SSIM tests: uploaded frames, one context per geometry
FULL = 4294960585             # the loss of a window of 0 against the peak


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("planar", [False, True], ids=["semi", "planar"])
@pytest.mark.parametrize("hdr", [False, True], ids=["sdr", "hdr"])
def test_layouts_strides_offsets_and_remainders(ctx, dev, hdr, planar, tile):
    """70 x 38 (w & 3 = h & 3 = 2, chroma 35 x 19: tiles without a window on both edges, partly filled chroma tiles, an odd number of
    chroma rows) with strides 70 / 74 / 80 on either side, bases at the allocation and 2 elements into it, every element random
    INCLUDING the padding and the unused remainder; 128 x 64 with everything aligned, whose last tile column and row own one window
    fewer.  Three pairs a launch.  Planar 8-bit frames at tile 16 are the case in which a 16-byte item holds two chroma tiles; in the
    semi-planar ones U and V of a tile share the item.  The first pair's map also adds up to the device's own hf_frame_ssim."""
    H, W, strides = RAGGED
    want = run_map_layout_case(ctx(hdr, H, W), dev, hdr, planar, H, W, strides, tile, seed=41 + 2 * hdr + planar)
    if tile == 16:
        assert want[0]["count"][0].tolist() == [[16, 16, 16, 16, 0], [16, 16, 16, 16, 0], [0, 0, 0, 0, 0]]
        assert want[0]["count"][1].tolist() == want[0]["count"][2].tolist() == [[4, 4, 4, 2, 0], [2, 2, 2, 1, 0], [0, 0, 0, 0, 0]]
    want = run_map_layout_case(ctx(hdr, 64, 128), dev, hdr, planar, 64, 128, ((128, 128),), tile, seed=43 + 2 * hdr + planar)
    # 32 x 16 luma blocks, 16 x 8 chroma blocks: the first luma tile, the last one, and the last chroma tile of the first row
    assert [int(want[0]["count"][i]) for i in ((0, 0, 0), (0, -1, -1), (1, 0, -1))] == {16: [16, 9, 2], 32: [64, 49, 12], 64: [240, 225, 49]}[tile]


@pytest.mark.parametrize("planar", [False, True], ids=["semi", "planar"])
@pytest.mark.parametrize("hdr", [False, True], ids=["sdr", "hdr"])
def test_the_smallest_planes(ctx, dev, hdr, planar):
    """4 x 4 has no window anywhere and one all-zero tile per plane; 8 x 8 one luma window and none in chroma; 16 x 16 nine and one."""
    for S, counts in ((4, [0, 0, 0]), (8, [1, 0, 0]), (16, [9, 1, 1])):
        for tile in TILES:
            want = run_map_layout_case(ctx(hdr, S, S), dev, hdr, planar, S, S, ((S, S), (S, 16), (16, 16)), tile, seed=S)
            assert want[0].shape == (3, 1, 1) and want[0]["count"].reshape(-1).tolist() == counts
            assert all((want[0]["sum_loss_q32"][p] > 0).all() == bool(n) for p, n in enumerate(counts))


@pytest.mark.parametrize("tile", [16, 64])
@pytest.mark.parametrize("planar", [False, True], ids=["semi", "planar"])
@pytest.mark.parametrize("hdr", [False, True], ids=["sdr", "hdr"])
def test_more_than_one_patch_each_way_with_a_ragged_last_one(ctx, dev, hdr, planar, tile):
    """A workgroup's patch is 16 block rows of windows (64 rows of elements) by 24 .. 29 sixteen-byte units: 1018 x 262 is five patches
    down with a ragged last one and two to five across in luma, three down in chroma.  A window dropped, counted twice or given to the
    wrong tile at a seam changes an entry.  Stride 1024: wide loads; stride 1018 on one side: element by element."""
    H, W = 262, 1018
    want = run_map_layout_case(ctx(hdr, H, W), dev, hdr, planar, H, W, ((1024, 1024), (1018, 1024)), tile, offsets=(0,), seed=3)
    assert [int(want[0]["count"][p].sum()) for p in range(3)] == [253 * 64, 126 * 31, 126 * 31]


@pytest.mark.parametrize("hdr", [False, True], ids=["sdr", "hdr"])
def test_more_patches_than_workgroups_per_pair(ctx, dev, hdr):
    """32 x 5488 at tile 16 is 86 patches down in luma and 43 in chroma; at 192 pairs a pair has a handful of workgroups (the launch is as
    many as the device holds at once), which stride over them and through the planes."""
    H, W, tile, n = 5488, 32, 16, 192
    c = ctx(hdr, H, W)
    rng = np.random.default_rng(7 + hdr)
    uniq = [random_frame(rng, hdr, H, W) for _ in range(4)]
    ptrs = [dev.put(f) for f in uniq]
    ia, ib = rng.integers(0, 4, size=n), rng.integers(0, 4, size=n)
    for planar in (False, True):
        got = maps(c, [ptrs[i] for i in ia], [ptrs[i] for i in ib], tile, planar=planar)
        model = {}
        for k, (i, j) in enumerate(zip(ia, ib)):
            if (i, j) not in model:
                model[(i, j)] = frame_ssim_map(uniq[i], uniq[j], H, W, tile, planar=planar)
            same(got[k], model[(i, j)], (planar, k))


@pytest.mark.parametrize("n", [1, 3, 192])
def test_pairs_per_launch(ctx, dev, n):
    """1, 3 and HF_MAX_ERROR_PAIRS pairs in one launch, distinct content per pair, every map in its place in the one buffer."""
    H, W, tile = 38, 70, 16
    c = ctx(False, H, W)
    rng = np.random.default_rng(100 + n)
    uniq = [random_frame(rng, False, H, W) for _ in range(8)]
    ptrs = [dev.put(f) for f in uniq]
    ia, ib = rng.integers(0, 8, size=n), rng.integers(0, 8, size=n)
    got = maps(c, [ptrs[i] for i in ia], [ptrs[i] for i in ib], tile)
    model = {}
    for k, (i, j) in enumerate(zip(ia, ib)):
        if (i, j) not in model:
            model[(i, j)] = frame_ssim_map(uniq[i], uniq[j], H, W, tile)
        same(got[k], model[(i, j)], k)


def test_magnitudes_at_16_bits(ctx, dev):
    """256 x 128 P010: 0 against 65535, every window 4294960585, so a full tile-64 luma entry is 256 times that; and the
    anti-checkerboard a = 65535 ((x + y) & 1) against 65535 - a, whose luma windows lose 8574741222 each, above 2^32, with max_loss_q32
    held.  An equal pair beside them: every entry written, zero losses."""
    H, W = 128, 256
    c = ctx(True, H, W)
    n = n_el(H, W)
    lo, hi = np.zeros(n, np.uint16), np.full(n, 65535, np.uint16)
    y, x = np.mgrid[0:H + H // 2, 0:W]
    a = (65535 * ((x + y) & 1)).astype(np.uint16).reshape(-1)
    pl, ph, pa, pn = dev.put(lo), dev.put(hi), dev.put(a), dev.put(65535 - a)
    for tile in TILES:
        got = maps(c, [pl, pa, pa], [ph, pn, pa], tile)
        same(got[0], frame_ssim_map(lo, hi, H, W, tile), tile)
        same(got[1], frame_ssim_map(a, 65535 - a, H, W, tile), tile)
        tb = tile // 4
        assert tuple(got[0][0, 0, 0]) == (tb * tb * FULL, FULL, tb * tb, 0) and tuple(got[0][1, 0, 0]) == (tb * tb // 4 * FULL, FULL, tb * tb // 4, 0)
        assert tuple(got[1][0, 0, 0]) == (tb * tb * 8574741222, 8574741222, tb * tb, 0) and 8574741222 > 1 << 32
        assert totals(got[1])["Y"] == {"sum_loss_q32": 63 * 31 * 8574741222, "max_loss_q32": 8574741222, "count": 63 * 31}
        assert not got[2]["sum_loss_q32"].any() and not got[2]["max_loss_q32"].any() and not got[2]["reserved"].any()
        assert np.array_equal(got[2]["count"], got[0]["count"])
    assert tuple(maps(c, [pl], [ph], 64)[0][0, 0, 0]) == (256 * FULL, FULL, 256, 0)


def test_peaks(ctx, dev):
    """peak = 0 on planar 16-bit frames is 1023 (LSB-aligned yuv420p10le) and an explicit 1023 is the same; an explicit 65535 there and
    an explicit 100 or 255 on 8 bit follow the model with those constants."""
    H, W, tile = 38, 70, 16
    rng = np.random.default_rng(21)
    a, b = random_frame(rng, True, H, W, 1023), random_frame(rng, True, H, W, 1023)
    c = ctx(True, H, W)
    pa, pb = dev.put(a), dev.put(b)
    want = frame_ssim_map(a, b, H, W, tile, planar=True, peak=1023)
    same(maps(c, [pa], [pb], tile, planar=True)[0], want, "peak 0, planar")
    same(maps(c, [pa], [pb], tile, planar=True, peak=1023)[0], want, "peak 1023, planar")
    other = frame_ssim_map(a, b, H, W, tile, planar=True, peak=65535)
    assert not np.array_equal(other, want)
    same(maps(c, [pa], [pb], tile, planar=True, peak=65535)[0], other, "peak 65535, planar")
    same(maps(c, [pa], [pb], tile, peak=1023)[0], frame_ssim_map(a, b, H, W, tile, peak=1023), "peak 1023, semi-planar")
    same(maps(c, [pa], [pb], tile)[0], frame_ssim_map(a, b, H, W, tile, peak=65535), "peak 0, semi-planar")
    a8, b8 = random_frame(rng, False, H, W, 100), random_frame(rng, False, H, W, 100)
    c8 = ctx(False, H, W)
    pa, pb = dev.put(a8), dev.put(b8)
    for peak in (100, 255):
        same(maps(c8, [pa], [pb], tile, peak=peak)[0], frame_ssim_map(a8, b8, H, W, tile, peak=peak), peak)
    same(maps(c8, [pa], [pb], tile)[0], frame_ssim_map(a8, b8, H, W, tile, peak=255), "peak 0, 8 bit")


def test_error_returns_enqueue_nothing(native_lib, dev):
    """Every refusal is HF_ERR_INVALID_ARGUMENT, names its call and leaves the prefilled buffer as it was."""
    from hopperrender_amd import capi
    from hopperrender_amd.calc import OpticalFlowCalcHDR, OpticalFlowCalcSDR
    H, W = 38, 70
    L = capi.load()
    rng = np.random.default_rng(9)
    pa, pb = dev.put(random_frame(rng, False, H, 80)), dev.put(random_frame(rng, False, H, 80))
    c, c16 = OpticalFlowCalcSDR(H, W, flags=capi.HF_FLAG_ASYNC), OpticalFlowCalcHDR(H, W, flags=capi.HF_FLAG_ASYNC)
    tw, th, nbytes = c.frameSsimMapShape(16)
    buf = prefilled(2 * nbytes)
    try:
        tab = lambda *ps: (C.c_void_p * len(ps))(*ps)
        A, B, hole = tab(pa, pa), tab(pb, pb), tab(pa, None)
        big = (C.c_void_p * 193)(*([pa] * 193))
        enq = lambda n, a, b, sa, sb, planar, tile, maps, peak=0, cc=c: L.hf_frame_ssim_map_enqueue(cc._ctx, n, a, b, sa, sb, planar, peak, tile, C.c_void_p(maps))
        bad = {f"tile {t}": enq(2, A, B, 80, 80, 0, t, buf.ptr) for t in (0, -16, 8, 17, 48, 128)}
        bad.update({
            "null maps": enq(2, A, B, 80, 80, 0, 16, None), "maps 8 bytes in": enq(2, A, B, 80, 80, 0, 16, buf.ptr + 8),
            "maps 4 bytes in": enq(2, A, B, 80, 80, 0, 16, buf.ptr + 4),
            "null a": enq(2, None, B, 80, 80, 0, 16, buf.ptr), "null b": enq(2, A, None, 80, 80, 0, 16, buf.ptr),
            "null entry a": enq(2, hole, B, 80, 80, 0, 16, buf.ptr), "null entry b": enq(2, A, hole, 80, 80, 0, 16, buf.ptr),
            "n = 0": enq(0, A, B, 80, 80, 0, 16, buf.ptr), "n < 0": enq(-1, A, B, 80, 80, 0, 16, buf.ptr), "n = 193": enq(193, big, big, 80, 80, 0, 16, buf.ptr),
            "stride a below W": enq(2, A, B, 69, 80, 0, 16, buf.ptr), "stride b below W": enq(2, A, B, 80, 68, 0, 16, buf.ptr),
            "odd planar stride a": enq(2, A, B, 71, 80, 1, 16, buf.ptr), "odd planar stride b": enq(2, A, B, 80, 79, 1, 16, buf.ptr),
            "peak < 0": enq(2, A, B, 80, 80, 0, 16, buf.ptr, -1), "peak 256 on 8 bit": enq(2, A, B, 80, 80, 0, 16, buf.ptr, 256),
            "peak 1023 on 8 bit": enq(2, A, B, 80, 80, 1, 16, buf.ptr, 1023),
        })
        assert b"hf_frame_ssim_map_enqueue" in L.hf_last_error(c._ctx) and b"peak" in L.hf_last_error(c._ctx)
        bad["peak 65536 on 16 bit"] = enq(2, A, B, 80, 80, 0, 16, buf.ptr, 65536, c16)
        assert b"hf_frame_ssim_map_enqueue" in L.hf_last_error(c16._ctx) and b"peak" in L.hf_last_error(c16._ctx)
        bad["tile 24, named"] = enq(2, A, B, 80, 80, 0, 24, buf.ptr)
        assert b"hf_frame_ssim_map_enqueue" in L.hf_last_error(c._ctx) and b"tile" in L.hf_last_error(c._ctx)
        bad.update({
            "null context": L.hf_frame_ssim_map_enqueue(None, 2, A, B, 80, 80, 0, 0, 16, C.c_void_p(buf.ptr)),
            "shape: tile 24": L.hf_frame_ssim_map_shape(c._ctx, 24, None, None, None),
            "shape: null context": L.hf_frame_ssim_map_shape(None, 16, None, None, None),
        })
        assert {k: v for k, v in bad.items() if v != INVALID} == {}
        assert L.hf_frame_ssim_map_shape(c._ctx, 16, None, None, None) == 0
        c.sync(); c16.sync()
        assert (buf.download(np.uint8) == 0xFF).all()
        with pytest.raises(capi.HopperFlowError) as e:
            c.frameSsimMapEnqueue([pa], [pb], 20, buf.ptr, 80, 80)
        assert e.value.code == INVALID
        with pytest.raises(capi.HopperFlowError):
            c.frameSsimMapShape(20)
        assert (buf.download(np.uint8) == 0xFF).all()
    finally:
        buf.free()
        c.close()
        c16.close()


def test_ssim_slots_and_error_slots_are_untouched(ctx, dev):
    """SSIM slots and error slots filled before the map launch read back unchanged after it."""
    H, W = 38, 70
    c = ctx(True, H, W)
    rng = np.random.default_rng(3)
    f = [random_frame(rng, True, H, W) for _ in range(4)]
    p = [dev.put(x) for x in f]
    c.frameSsimEnqueue([p[0], p[1]], [p[2], p[3]], 0)
    c.frameErrorEnqueue([p[1], p[0]], [p[2], p[3]], 0)
    ssim_before, err_before = c.frameSsimRead(0, 256), c.frameErrorRead(0, 2)
    assert [ints(g) for g in ssim_before[:2]] == [frame_ssim(f[0], f[2], H, W), frame_ssim(f[1], f[3], H, W)]
    assert err_before[:2] == [frame_error(f[1], f[2], H, W), frame_error(f[0], f[3], H, W)]
    for tile in TILES:
        got = maps(c, [p[3], p[2]], [p[0], p[1]], tile)
        same(got[0], frame_ssim_map(f[3], f[0], H, W, tile), tile)
    assert c.frameSsimRead(0, 256) == ssim_before and c.frameErrorRead(0, 2) == err_before


def test_batch_member_maps_its_periods_outputs_without_a_sync(native_lib, dev):
    """A FlowBatch of 3 members at 640 x 360: runPeriod with two outputs each, then the six maps against uploaded truths enqueued on a
    member straight away (the member issues on the batch's stream, behind the warps); equal to the model on the frames downloaded after."""
    from hopperrender_amd import capi, synth
    from hopperrender_amd.calc import DeviceBuffer, FlowBatch, OpticalFlowCalcSDR, frame_ssim_maps
    H, W, n, tile = 360, 640, 3, 32
    scenes = [synth.Scene(H, W, False, 40 + m) for m in range(n)]
    frames = [[sc.frame(k) for k in range(5)] for sc in scenes]
    calcs = [OpticalFlowCalcSDR(H, W, search_radius=8, flags=capi.HF_FLAG_ASYNC) for _ in range(n)]
    ptr = [[dev.put(frames[m][k]) for k in (0, 2, 4)] for m in range(n)]
    truth = [[frames[m][1], frames[m][3]] for m in range(n)]
    tptr = [[dev.put(t) for t in truth[m]] for m in range(n)]
    outs = [[DeviceBuffer(calcs[0].output_frame_bytes) for _ in range(2)] for _ in range(n)]
    tw, th, nbytes = calcs[1].frameSsimMapShape(tile)
    buf = prefilled(6 * nbytes)
    batch = FlowBatch(calcs)
    try:
        for k in range(2):
            batch.runPeriod(batch.preparePeriod([ptr[m][k] for m in range(n)], None, None))
        batch.runPeriod(batch.preparePeriod([ptr[m][2] for m in range(n)], [[0.25, 0.5]] * n, [[b.ptr for b in o] for o in outs]))
        calcs[1].frameSsimMapEnqueue([outs[m][i].ptr for m in range(n) for i in range(2)], [tptr[m][i] for m in range(n) for i in range(2)], tile, buf.ptr)
        batch.sync()
        raw = buf.download(np.uint8)
        assert (raw[6 * nbytes:] == 0xFF).all()
        got = frame_ssim_maps(raw, 6, tw, th)
        k = 0
        for m in range(n):
            for i in range(2):
                same(got[k], frame_ssim_map(outs[m][i].download(np.uint8), truth[m][i], H, W, tile), (m, i))
                assert got[k]["sum_loss_q32"][0].any() and int(got[k]["count"][0].sum()) == 159 * 89
                k += 1
    finally:
        batch.close()
        for c in calcs:
            c.close()
        for o in outs:
            for b in o:
                b.free()
        buf.free()


def test_dual_stream_context_warp_then_map(native_lib, dev):
    """HF_FLAG_DUAL_STREAM: the warps run on the context's second stream; the map is ordered behind them with no sync in between."""
    from hopperrender_amd import capi, synth
    from hopperrender_amd.calc import DeviceBuffer, OpticalFlowCalcHDR, frame_ssim_maps
    H, W, tile = 360, 640, 16
    sc = synth.Scene(H, W, True, 77)
    f = [sc.frame(k) for k in range(4)]
    c = OpticalFlowCalcHDR(H, W, search_radius=8, flags=capi.HF_FLAG_ASYNC | capi.HF_FLAG_DUAL_STREAM)
    out = DeviceBuffer(c.output_frame_bytes)
    tw, th, nbytes = c.frameSsimMapShape(tile)
    buf = prefilled(nbytes)
    try:
        p = [dev.put(x) for x in f]
        c.updateFrameDeviceRef(p[0]); c.updateFrameDeviceRef(p[1])
        c.interpolatePeriod(p[2], [0.5], [out.ptr])
        c.interpolatePeriod(p[3], [0.5], [out.ptr])   # (shows the pair (1, 2) with the flow of the period before)
        c.frameSsimMapEnqueue([out.ptr], [p[2]], tile, buf.ptr)
        c.sync()
        got = frame_ssim_maps(buf.download(np.uint8), 1, tw, th)[0]
        same(got, frame_ssim_map(out.download(np.uint16), f[2], H, W, tile), "map behind the period")
        assert got["sum_loss_q32"][0].any()
    finally:
        c.close()
        out.free()
        buf.free()


CHILD = r"""
import sys, ctypes as C
sys.path.insert(0, {root!r}); sys.path.insert(0, {root!r} + "/tests")
from hopperrender_amd import capi
from hopperrender_amd.calc import OpticalFlowCalcHDR, OpticalFlowCalcSDR
from frame_ssim_cases import RAGGED, Dev
from frame_ssim_map_cases import run_map_layout_case

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
        for tile in (16, 32, 64):
            run_map_layout_case(c, dev, hdr, planar, H, W, strides, tile, seed=41 + 2 * hdr + planar)
            assert violations(c)[0] == 0, (hdr, planar, tile, violations(c))
    c.close()
dev.free()
print("SSIM-MAP-DEBUG-BOUNDS-OK")
"""


def test_ragged_layouts_under_the_bounds_checking_build(native_lib):
    """The ragged 70 x 38 case with every stride pair and both base offsets, all four kernels and three tiles, in a fresh child process
    under libhopperflow_dbg.so (every load of the kernel checked against its frame's extent, every store against the map buffer's): the
    same results and zero violations."""
    from hopperrender_amd import build
    dbg = build.build_flow(debug_bounds=True)
    env = dict(os.environ, HF_LIB=dbg)
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT)], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0 and "SSIM-MAP-DEBUG-BOUNDS-OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
