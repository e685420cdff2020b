"""GPU: the device's per-tile error maps (hf_frame_error_map_shape / _enqueue, csrc/hf_metrics.hip) against the numpy model of
tests/frame_error_map_model.py.  Integer sums: every field of every tile of every plane must be EQUAL.  Frames are made on the host and
uploaded; every map buffer is prefilled with 0xFF bytes, so an entry the launch did not write shows."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_frame_error_gpu as feg  # noqa: E402
from frame_error_map_model import TILES, frame_error_map, map_shape  # noqa: E402
from frame_error_model import PLANES  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID = -1   # HF_ERR_INVALID_ARGUMENT
dev, ctx = feg.dev, feg.ctx   # the fixtures of the error sums' tests: uploaded frames, one context per geometry


def _prefilled(nbytes):
    from hopperrender_amd.calc import DeviceBuffer
    buf = DeviceBuffer(nbytes + 64)
    buf.upload(np.full(nbytes + 64, 0xFF, np.uint8))
    return buf


def _maps(c, pa, pb, tile, sa=0, sb=0, planar=False):
    """the maps of pairs (pa[i], pb[i]) from a prefilled buffer, [n][3][th][tw]"""
    from hopperrender_amd.calc import frame_error_maps
    tw, th, nbytes = c.frameErrorMapShape(tile)
    n = len(pa)
    buf = _prefilled(n * nbytes)
    try:
        c.frameErrorMapEnqueue(pa, pb, tile, buf.ptr, sa, sb, planar)
        c.sync()
        raw = buf.download(np.uint8)
    finally:
        buf.free()
    assert (raw[n * nbytes:] == 0xFF).all(), "bytes behind the last map were written"
    return frame_error_maps(raw, n, tw, th).copy()


def _same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.size} entries differ; first at [plane, ty, tx] = {i}: device {got[i]}, model {want[i]}")


def _sums(m):
    """a map's totals in the shape of the error sums"""
    return {p: {"sse": int(m["sse"][i].astype(object).sum()), "sad": int(m["sad"][i].astype(object).sum()), "max_abs": int(m["max_abs"][i].max())}
            for i, p in enumerate(PLANES)}


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("planar", [False, True], ids=["semi", "planar"])
@pytest.mark.parametrize("hdr", [False, True], ids=["sdr", "hdr"])
def test_layouts_strides_offsets_and_padding(ctx, dev, hdr, planar, tile):
    """70 x 38 (ragged row tail, ragged last tile both ways, H/2 odd) with strides 70 / 74 / 80 on either side, bases at the allocation
    and 2 elements into it, padding columns random and different on the two sides; 128 x 64: whole tiles, everything aligned.  Three
    pairs a launch.  Planar 8-bit frames at tile 16 are the case in which a work item holds two chroma tiles.  The first pair's map also
    adds up to the device's own error sums."""
    rng = np.random.default_rng(31 + 2 * hdr + planar)
    for (H, W, strides) in ((38, 70, ((70, 70), (74, 80), (80, 80), (80, 74), (80, 70))), (64, 128, ((128, 128),))):
        c = ctx(hdr, H, W)
        assert c.frameErrorMapShape(tile) == (map_shape(H, W, tile)[1], map_shape(H, W, tile)[0], 48 * map_shape(H, W, tile)[0] * map_shape(H, W, tile)[1])
        for sa, sb in strides:
            fa = [feg._random(rng, hdr, H, sa) for _ in range(3)]
            fb = [feg._random(rng, hdr, H, sb) for _ in range(3)]
            want = [frame_error_map(a, b, H, W, tile, sa, sb, planar) for a, b in zip(fa, fb)]
            for off in (0, 2):   # all bases aligned (wide accesses where the pitches allow them), then all 2 elements in (element by element)
                pa, pb = [dev.put(a, off) for a in fa], [dev.put(b, off) for b in fb]
                got = _maps(c, pa, pb, tile, sa, sb, planar)
                for i in range(3):
                    _same(got[i], want[i], (H, W, sa, sb, off, i))
                err = c.frameError(pa[0], pb[0], sa, sb, planar)
                assert _sums(got[0]) == {p: {k: err[p][k] for k in ("sse", "sad", "max_abs")} for p in PLANES}, (H, W, sa, sb, off)


@pytest.mark.parametrize("n", [1, 3, 192])
def test_pairs_per_launch(ctx, dev, n):
    """1, 3 and HF_MAX_ERROR_PAIRS pairs in one launch, distinct content per pair, every map in its place in the one buffer."""
    H, W, tile = 38, 70, 16
    c = ctx(False, H, W)
    rng = np.random.default_rng(100 + n)
    uniq = [feg._random(rng, False, H, W) for _ in range(8)]
    ptrs = [dev.put(f) for f in uniq]
    ia, ib = rng.integers(0, 8, size=n), rng.integers(0, 8, size=n)
    got = _maps(c, [ptrs[i] for i in ia], [ptrs[i] for i in ib], tile)
    model = {}
    for k, (i, j) in enumerate(zip(ia, ib)):
        if (i, j) not in model:
            model[(i, j)] = frame_error_map(uniq[i], uniq[j], H, W, tile)
        _same(got[k], model[(i, j)], k)


@pytest.mark.parametrize("hdr", [False, True], ids=["sdr", "hdr"])
def test_more_bands_than_workgroups_per_pair(ctx, dev, hdr):
    """32 x 5488 at tile 16 is 343 bands; at 192 pairs a pair has 341 workgroups (65536 in the launch), which stride over them."""
    H, W, tile, n = 5488, 32, 16, 192
    c = ctx(hdr, H, W)
    rng = np.random.default_rng(7 + hdr)
    uniq = [feg._random(rng, hdr, H, W) for _ in range(4)]
    ptrs = [dev.put(f) for f in uniq]
    ia, ib = rng.integers(0, 4, size=n), rng.integers(0, 4, size=n)
    got = _maps(c, [ptrs[i] for i in ia], [ptrs[i] for i in ib], tile)
    model = {}
    for k, (i, j) in enumerate(zip(ia, ib)):
        if (i, j) not in model:
            model[(i, j)] = frame_error_map(uniq[i], uniq[j], H, W, tile)
        _same(got[k], model[(i, j)], k)


@pytest.mark.parametrize("planar", [False, True], ids=["semi", "planar"])
@pytest.mark.parametrize("hdr", [False, True], ids=["sdr", "hdr"])
def test_rows_of_every_width_class(ctx, dev, hdr, planar):
    """How a workgroup reads a row depends on its work items (16 bytes each): up to 64 one wave and the rows dealt to four, up to 128 two
    waves side by side, beyond that four -- and beyond 256 a second sweep.  20 rows (a ragged second band) of 130 and of 259 items; the
    planar chroma rows have 65 and 130.  The smaller classes are those of the 70- and 128-wide frames above."""
    H = 20
    rng = np.random.default_rng(61 + 2 * hdr + planar)
    for items in (130, 259):
        W = (items * 16 - 12) // (2 if hdr else 1)   # the last item is ragged; the pitch is aligned, so the others are wide loads
        S = (W + 31) // 32 * 32
        c = ctx(hdr, H, W)
        assert W % 2 == 0 and (W * (2 if hdr else 1) + 15) // 16 == items
        fa, fb = feg._random(rng, hdr, H, S), feg._random(rng, hdr, H, S)
        pa, pb = dev.put(fa), dev.put(fb)
        for tile in (16, 64):
            _same(_maps(c, [pa], [pb], tile, S, S, planar)[0], frame_error_map(fa, fb, H, W, tile, S, S, planar), (W, tile))


@pytest.mark.parametrize("planar", [False, True], ids=["semi", "planar"])
@pytest.mark.parametrize("hdr", [False, True], ids=["sdr", "hdr"])
def test_one_difference_in_the_last_v_element_and_an_equal_pair(ctx, dev, hdr, planar):
    """Equal everywhere but the last column of the last chroma row, only in V: one entry of the map is not zero, tile (4, 2) of V at tile
    16 and (1, 0) at 64.  A pair equal everywhere: every entry is written, as zeros."""
    H, W, S = 38, 70, 80
    c = ctx(hdr, H, W)
    base = feg._random(np.random.default_rng(5), hdr, H, S)
    hc, sc = H // 2, S // 2
    f = base.copy()
    v_last = H * S + hc * sc + (hc - 1) * sc + (W // 2 - 1) if planar else H * S + (hc - 1) * S + (W - 1)
    top = 65535 if hdr else 255
    f[v_last] = top - f[v_last]
    d = abs(int(f[v_last]) - int(base[v_last]))
    pf, pb = dev.put(f), dev.put(base)
    for tile, (ti, tj) in ((16, (4, 2)), (32, (2, 1)), (64, (1, 0))):
        got = _maps(c, [pf, pb], [pb, pb], tile, S, S, planar)
        _same(got[0], frame_error_map(f, base, H, W, tile, S, S, planar), tile)
        assert np.count_nonzero(got[0]["sse"]) == 1 and tuple(got[0][2, tj, ti]) == (d * d, d, d)
        assert not got[1].view(np.uint8).any()


def test_a_saturated_tile_needs_more_than_32_bits(ctx, dev):
    """64 x 64 HDR, 0 against 65535: at tile 64 the one luma entry holds 4096 x 65535^2 = 1.76e13; at tile 16 every entry 256 x 65535^2."""
    H = W = 64
    c = ctx(True, H, W)
    n = feg._n_el(H, W)
    pa, pb = dev.put(np.zeros(n, np.uint16)), dev.put(np.full(n, 65535, np.uint16))
    for planar in (False, True):
        for tile in TILES:
            got = _maps(c, [pa], [pb], tile, planar=planar)[0]
            cnt = tile * tile
            assert got.shape == (3, 64 // tile, 64 // tile)
            assert (got["sse"][0] == cnt * 65535 ** 2).all() and (got["sad"][0] == cnt * 65535).all() and (got["max_abs"] == 65535).all()
            assert (got["sse"][1:] == cnt // 4 * 65535 ** 2).all() and (got["sad"][1:] == cnt // 4 * 65535).all()
    assert 4096 * 65535 ** 2 > 1 << 43


def test_error_returns_enqueue_nothing(ctx, dev):
    """Every refusal is HF_ERR_INVALID_ARGUMENT and leaves the prefilled buffer as it was."""
    from hopperrender_amd import capi
    H, W = 38, 70
    c = ctx(False, H, W)
    L = capi.load()
    rng = np.random.default_rng(9)
    pa, pb = dev.put(feg._random(rng, False, H, 80)), dev.put(feg._random(rng, False, H, 80))
    tw, th, nbytes = c.frameErrorMapShape(16)
    buf = _prefilled(2 * nbytes)
    try:
        tab = lambda *ps: (C.c_void_p * len(ps))(*ps)
        A, B, hole = tab(pa, pa), tab(pb, pb), tab(pa, None)
        big = (C.c_void_p * 193)(*([pa] * 193))
        enq = lambda n, a, b, sa, sb, planar, tile, maps: L.hf_frame_error_map_enqueue(c._ctx, n, a, b, sa, sb, planar, tile, C.c_void_p(maps))
        bad = {f"tile {t}": enq(2, A, B, 80, 80, 0, t, buf.ptr) for t in (0, -16, 8, 17, 48, 128)}
        bad.update({
            "null maps": enq(2, A, B, 80, 80, 0, 16, None), "maps 8 bytes in": enq(2, A, B, 80, 80, 0, 16, buf.ptr + 8),
            "maps 4 bytes in": enq(2, A, B, 80, 80, 0, 16, buf.ptr + 4),
            "null a": enq(2, None, B, 80, 80, 0, 16, buf.ptr), "null b": enq(2, A, None, 80, 80, 0, 16, buf.ptr),
            "null entry a": enq(2, hole, B, 80, 80, 0, 16, buf.ptr), "null entry b": enq(2, A, hole, 80, 80, 0, 16, buf.ptr),
            "n = 0": enq(0, A, B, 80, 80, 0, 16, buf.ptr), "n < 0": enq(-1, A, B, 80, 80, 0, 16, buf.ptr), "n = 193": enq(193, big, big, 80, 80, 0, 16, buf.ptr),
            "stride a below W": enq(2, A, B, 69, 80, 0, 16, buf.ptr), "stride b below W": enq(2, A, B, 80, 68, 0, 16, buf.ptr),
            "odd planar stride": enq(2, A, B, 71, 80, 1, 16, buf.ptr),
            "null context": L.hf_frame_error_map_enqueue(None, 2, A, B, 80, 80, 0, 16, C.c_void_p(buf.ptr)),
            "shape: tile 24": L.hf_frame_error_map_shape(c._ctx, 24, None, None, None),
            "shape: null context": L.hf_frame_error_map_shape(None, 16, None, None, None),
        })
        assert {k: v for k, v in bad.items() if v != INVALID} == {}
        assert b"hf_frame_error_map_enqueue" in L.hf_last_error(c._ctx)
        assert L.hf_frame_error_map_shape(c._ctx, 16, None, None, None) == 0
        c.sync()
        assert (buf.download(np.uint8) == 0xFF).all()
        with pytest.raises(capi.HopperFlowError) as e:
            c.frameErrorMapEnqueue([pa], [pb], 20, buf.ptr, 80, 80)
        assert e.value.code == INVALID
        with pytest.raises(capi.HopperFlowError):
            c.frameErrorMapShape(20)
    finally:
        buf.free()


@pytest.mark.parametrize("dual", [False, True], ids=["async", "dual-stream"])
def test_map_straight_behind_a_period_without_a_sync(native_lib, dev, dual):
    """interpolatePeriod on an asynchronous context (and on one whose warps run on a second stream), then the map of its output against
    the withheld frame enqueued at once: equal to the model on the output downloaded afterwards."""
    from hopperrender_amd import capi, synth
    from hopperrender_amd.calc import DeviceBuffer, OpticalFlowCalcHDR, frame_error_maps
    H, W, tile = 360, 640, 32
    sc = synth.Scene(H, W, True, 78)
    f = [sc.frame(k) for k in range(4)]
    c = OpticalFlowCalcHDR(H, W, search_radius=8, flags=capi.HF_FLAG_ASYNC | (capi.HF_FLAG_DUAL_STREAM if dual else 0))
    out = DeviceBuffer(c.output_frame_bytes)
    tw, th, nbytes = c.frameErrorMapShape(tile)
    buf = _prefilled(nbytes)
    try:
        p = [dev.put(x) for x in f]
        c.updateFrameDeviceRef(p[0]); c.updateFrameDeviceRef(p[1])
        c.interpolatePeriod(p[2], [0.5], [out.ptr])
        c.interpolatePeriod(p[3], [0.5], [out.ptr])   # (shows the pair (1, 2) with the flow of the period before)
        c.frameErrorMapEnqueue([out.ptr], [p[2]], tile, buf.ptr)
        c.sync()
        got = frame_error_maps(buf.download(np.uint8), 1, tw, th)[0]
        _same(got, frame_error_map(out.download(np.uint16), f[2], H, W, tile), "map behind the period")
        assert np.count_nonzero(got["sse"][0]) > 0
    finally:
        c.close()
        out.free()
        buf.free()
