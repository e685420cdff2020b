"""CPU: the model of the guarded blend (tests/guarded_blend_model.py) against the definition of hf_guarded_blend_enqueue in
include/hopperflow.h, calc.guard_weights against the model's weights, and the inputs the GPU tests use: in every geometry their weights
contain 0, 256 and values between, so no case there degenerates to a copy of one of the two frames."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded_blend_model as gbm  # noqa: E402
from frame_error_map_model import TILES, map_shape  # noqa: E402
from test_warp_disagreement_gpu import GEOMETRIES, T5, flows  # noqa: E402  (the geometries and flows of the launch this one runs first)
from warp_disagreement_model import warp_disagreement_maps  # noqa: E402

from hopperrender_amd.calc import ERROR_TILE_DTYPE, guard_weights  # noqa: E402


def _geom(hdr, H, W, res=270, si=0, so=0):
    from oracle import oracle
    return oracle.make_geom(int(hdr), H, W, si, so, res)


def _maps_of_sad(sad):
    """maps [n][3][th][tw] with the given luma sad [n][th][tw]; the chroma planes hold a sad that would change every weight if consulted"""
    sad = np.asarray(sad, np.int64)
    m = np.zeros((sad.shape[0], 3) + sad.shape[1:], ERROR_TILE_DTYPE)
    m["sad"][:, 0] = sad
    m["sad"][:, 1:] = 0xFFFFFFFF
    return m


def _both(maps, tile, lo, hi, H, W, hdr):
    """the model's weights, and calc.guard_weights held to them"""
    wt = gbm.tile_weights(maps, tile, lo, hi, H, W, hdr)
    w = gbm.luma_weights(wt, tile, H, W)
    cwt, cw = guard_weights(maps, tile, lo, hi, H, W, hdr)
    assert cwt.dtype == cw.dtype == np.int64 and np.array_equal(cwt, wt) and np.array_equal(cw, w)
    return wt, w


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("hdr", [False, True], ids=["sdr", "hdr"])
def test_weights_stay_within_0_and_256_and_reach_both(hdr, tile):
    H, W = 120, 200
    th, tw = map_shape(H, W, tile)
    rng = np.random.default_rng(tile + hdr)
    top = tile * tile * (65535 if hdr else 255)
    sad = rng.integers(0, top + 1, size=(3, th, tw))
    sad[0, 0, 0], sad[0, -1, -1] = 0, top           # (the corner tiles are partial: `top` is beyond what they can hold, still 256)
    wt, w = _both(_maps_of_sad(sad), tile, 700, 2900, H, W, hdr)
    for a in (wt, w):
        assert a.min() == 0 and a.max() == 256
    assert len(np.unique(w)) > 50
    # between equal neighbours the interpolation is the identity; between 0 and 256 it is monotonic and hits neither end early
    flat, _ = _both(_maps_of_sad(np.full((1, th, tw), top)), tile, 0, 1, H, W, hdr)
    assert (flat == 256).all() and (_both(_maps_of_sad(np.full((1, th, tw), top)), tile, 0, 1, H, W, hdr)[1] == 256).all()


@pytest.mark.parametrize("hdr", [False, True], ids=["sdr", "hdr"])
def test_the_interpolation_between_two_tile_centres(hdr):
    """tile 16, tiles 0 / 256 side by side: left of the first centre 0, then (fx 16 256 + 128) >> 8 = fx 16 rising to the second centre"""
    H, W, tile = 16, 32, 16
    unit = 256 if hdr else 1
    sad = np.array([[[0, 256 * 255 * unit]]])
    _, w = _both(_maps_of_sad(sad), tile, 0, 1, H, W, hdr)
    want = np.concatenate([np.zeros(8, np.int64), 16 * np.arange(16, dtype=np.int64), np.full(8, 256, np.int64)])
    assert (w[0] == want[None, :]).all()


@pytest.mark.parametrize("hdr", [False, True], ids=["sdr", "hdr"])
def test_guard_off_is_the_blend_and_a_saturated_guard_the_cross_fade(hdr):
    H, W = 50, 86
    g = _geom(hdr, H, W, 25, 0, 96)
    rng = np.random.default_rng(11 + hdr)
    f = gbm.guard_frames(rng, hdr, g)
    f[1] = rng.integers(0, 65536 if hdr else 256, size=f[1].shape, dtype=f[1].dtype)   # random everywhere
    flow = flows(g, rng)["random"]
    ts = [np.float32(t) for t in T5]
    for levels in ((0.0, 255.0), (16.0, 235.0)):
        off, _, w = gbm.guarded_blend(f[0], f[1], flow, g, ts, 16, *gbm.GUARD_OFF, *levels)
        all_on, maps, w1 = gbm.guarded_blend(f[0], f[1], flow, g, ts, 16, 0, 1, *levels)
        assert not w.any() and (w1.reshape(len(ts), -1, g.out_stride)[:, :, :W] == 256).all() and maps["sad"][:, 0].all()
        for k, t in enumerate(ts):
            M, Z = gbm.halves(f[0], f[1], flow, g, t, *levels)
            assert np.array_equal(off[k].reshape(-1), M) and np.array_equal(all_on[k].reshape(-1), Z)
            assert np.array_equal(M, Z) == (t in (0.0, 1.0))   # (at t = 0 and t = 1 one frame has weight 0 and the other is not displaced)


def test_a_one_tile_frame_has_one_weight():
    H, W, tile = 36, 40, 64
    for hdr in (False, True):
        unit = 256 if hdr else 1
        wt, w = _both(_maps_of_sad([[[H * W * 100 * unit]]]), tile, 800, 2400, H, W, hdr)   # m = 1600: half way
        assert wt.shape == (1, 1, 1) and wt[0, 0, 0] == 128 and (w == 128).all()


def test_partial_edge_tiles_use_their_true_count():
    """86 x 50 at tile 16: the last column of tiles is 6 wide, the last row 2 high.  The same MEAN difference in every tile gives the same
    weight in every tile; counted as full tiles the partial ones would fall below lo."""
    H, W, tile = 50, 86, 16
    th, tw = map_shape(H, W, tile)
    cnt = np.minimum(tile, H - tile * np.arange(th))[:, None] * np.minimum(tile, W - tile * np.arange(tw))[None, :]
    assert cnt[-1, -1] == 12 and cnt[0, -1] == 96 and cnt[-1, 0] == 32
    wt, w = _both(_maps_of_sad((cnt * 100)[None]), tile, 1000, 2200, H, W, False)
    assert (wt == 128).all() and (w == 128).all()
    wt, _ = _both(_maps_of_sad((cnt * 100 * 256)[None]), tile, 1000, 2200, H, W, True)
    assert (wt == 128).all()


def test_chroma_takes_the_weight_of_its_even_luma_position():
    H, W, tile, so = 50, 86, 16, 96
    th, tw = map_shape(H, W, tile)
    sad = np.random.default_rng(4).integers(0, 256 * 255, size=(2, th, tw))
    _, w = _both(_maps_of_sad(sad), tile, 500, 3500, H, W, False)
    e = gbm.element_weights(w, H, W, so)
    assert e.shape == (2, 75, so) and np.array_equal(e[:, :H, :W], w) and not e[:, :, W:].any()
    for k in range(2):
        for cy in (0, 3, 12, 24):
            for cx in (0, 1, 2, 7, 40, 41, 84, 85):
                assert e[k, H + cy, cx] == w[k, 2 * cy, cx & ~1]
    assert len(np.unique(e[:, H:, :W])) > 50


def test_one_ten_bit_code_is_four_q4_units():
    """P010: a 10-bit code is 64 of the 16-bit scale; a mean difference of c 10-bit codes is m = 4 c, as c 8-bit codes are m = 16 c"""
    H = W = tile = 16
    for c in (1, 3, 250):
        maps = _maps_of_sad([[[256 * 64 * c]]])
        assert gbm.q4_means(maps, tile, H, W, True)[0, 0, 0] == 4 * c
        assert gbm.tile_weights(maps, tile, 4 * c - 1, 4 * c, H, W, True)[0, 0, 0] == 256      # m >= hi
        assert gbm.tile_weights(maps, tile, 4 * c, 4 * c + 1, H, W, True)[0, 0, 0] == 0        # m <= lo
        assert gbm.q4_means(_maps_of_sad([[[256 * c]]]), tile, H, W, False)[0, 0, 0] == 16 * c


def test_saturated_hdr_at_tile_64_stays_within_64_bits():
    """The largest intermediates of steps 3 to 5 in Python integers: all far below 2^63, and numpy's int64 gives the same."""
    tile, cnt, sad = 64, 64 * 64, 64 * 64 * 65535
    assert sad < 1 << 32                                                   # the map's field holds it
    assert 16 * sad < 1 << 63 and (cnt << 8) < 1 << 63
    m = (16 * sad) // (cnt << 8)
    assert m == 4095
    assert (m - 0) * 256 < 1 << 63
    assert (tile * tile * 256 + tile * tile // 2) < 1 << 63               # step 4's sum at its largest
    assert 65535 * 256 + 128 < 1 << 63                                    # step 5's
    maps = _maps_of_sad([[[sad]]])
    wt, w = _both(maps, tile, 0, 65535, 64, 64, True)
    assert wt[0, 0, 0] == (4095 * 256) // 65535 == 15 and (w == 15).all()
    wt, w = _both(maps, tile, 4094, 4095, 64, 64, True)
    assert wt[0, 0, 0] == 256 and (w == 256).all()
    assert (gbm.mix(np.full(4, 65535, np.uint16), np.full(4, 65535, np.uint16), np.array([0, 1, 255, 256])) == 65535).all()
    assert (gbm.mix(np.array([0, 65535], np.uint16), np.array([65535, 0], np.uint16), np.array([256, 256])) == [65535, 0]).all()


def test_guard_weights_refuses_what_the_call_refuses():
    maps = _maps_of_sad(np.zeros((1, 4, 6)))
    for tile, lo, hi in ((8, 0, 1), (16, -1, 5), (16, 5, 5), (16, 6, 5), (16, 0, 65536)):
        with pytest.raises(ValueError):
            guard_weights(maps, tile, lo, hi, 50, 86, False)
    with pytest.raises(ValueError):
        guard_weights(maps, 32, 0, 1, 50, 86, False)     # maps of another tile's grid


@pytest.mark.parametrize("hdr", [False, True], ids=["sdr", "hdr"])
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_the_gpu_cases_inputs_cannot_degenerate(name, hdr):
    """The construction test_guarded_blend_gpu.py uses, per geometry, rs and tile: frames whose left third agrees, thresholds around the
    mean of the rest.  Over the flows of a case the weights contain 0, 256 and values strictly between."""
    H, W, res, si, so, _, tiles = GEOMETRIES[name]
    ts = [np.float32(t) for t in T5]
    for rs in range(4):
        g = _geom(hdr, H, W, res[rs], si, so)
        rng = np.random.default_rng(17 + rs + 4 * hdr)
        f = gbm.guard_frames(rng, hdr, g)
        fl = flows(g, rng)
        for tile in tiles:
            lo, hi = gbm.thresholds_around(warp_disagreement_maps(f[0], f[1], fl["random"], g, ts, tile), tile, H, W, hdr)
            assert 0 <= lo < hi <= 4095
            seen = set()
            for kind in ("zero", "random"):
                maps = warp_disagreement_maps(f[0], f[1], fl[kind], g, ts, tile)
                wt, w = _both(maps, tile, lo, hi, H, W, hdr)
                seen |= set(np.unique(wt).tolist()) | set(np.unique(w).tolist())
            assert 0 in seen and 256 in seen and any(0 < v < 256 for v in seen), (name, hdr, rs, tile, lo, hi, sorted(seen))
