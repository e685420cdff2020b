"""CPU: the numpy model of the per-tile error maps (tests/frame_error_map_model.py) against the frame error model it refines: per plane
the tile sums add up to the frame's sums, the largest tile maximum is the frame's, ragged last tiles hold the right element counts, and
a single difference lands in the one tile that covers it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frame_error_map_model as fmm  # noqa: E402
from frame_error_model import PLANES, frame_error  # noqa: E402


def _frame(rng, hdr, H, S, planar):
    n = H * S + (2 * (H // 2) * (S // 2) if planar else (H // 2) * S)
    return rng.integers(0, 65536 if hdr else 256, size=n, dtype=np.uint16 if hdr else np.uint8)


@pytest.mark.parametrize("tile", fmm.TILES)
@pytest.mark.parametrize("planar", [False, True], ids=["semi", "planar"])
@pytest.mark.parametrize("hdr", [False, True], ids=["sdr", "hdr"])
@pytest.mark.parametrize("H,W,sa,sb", [(38, 70, 74, 80), (64, 128, 128, 128)], ids=["70x38", "128x64"])
def test_tile_sums_add_up_to_the_frame_sums(H, W, sa, sb, hdr, planar, tile):
    rng = np.random.default_rng(H + 2 * hdr + planar)
    a, b = _frame(rng, hdr, H, sa, planar), _frame(rng, hdr, H, sb, planar)
    m, cnt = fmm.frame_error_map(a, b, H, W, tile, sa, sb, planar, counts=True)
    want = frame_error(a, b, H, W, sa, sb, planar)
    th, tw = fmm.map_shape(H, W, tile)
    assert m.shape == (3, th, tw) and m.dtype.itemsize == 16 and m.nbytes == 48 * th * tw
    for i, p in enumerate(PLANES):
        assert int(m["sse"][i].astype(object).sum()) == want[p]["sse"]
        assert int(m["sad"][i].astype(object).sum()) == want[p]["sad"]
        assert int(m["max_abs"][i].max()) == want[p]["max_abs"]
        assert int(cnt[i].sum()) == want[p]["count"]


def test_ragged_last_tiles_hold_the_right_element_counts():
    """70 x 38 at tile 16: 5 x 3 tiles; the last luma column of tiles is 6 wide and the last row 6 high; chroma is 35 x 19, so the last
    chroma tiles are 3 wide and 3 high.  At tile 64 the frame is two tiles across and one down."""
    H, W = 38, 70
    z = np.zeros(H * W * 3 // 2, np.uint8)
    _, cnt = fmm.frame_error_map(z, z, H, W, 16, counts=True)
    assert cnt.shape == (3, 3, 5)
    assert cnt[0].tolist() == [[256, 256, 256, 256, 96], [256, 256, 256, 256, 96], [96, 96, 96, 96, 36]]
    assert cnt[1].tolist() == cnt[2].tolist() == [[64, 64, 64, 64, 24], [64, 64, 64, 64, 24], [24, 24, 24, 24, 9]]
    _, cnt = fmm.frame_error_map(z, z, H, W, 64, counts=True)
    assert cnt[0].tolist() == [[64 * 38, 6 * 38]] and cnt[2].tolist() == [[32 * 19, 3 * 19]]


@pytest.mark.parametrize("planar", [False, True], ids=["semi", "planar"])
def test_one_difference_lands_in_the_tile_that_covers_it(planar):
    """V(18, 34), the last chroma element of 70 x 38, is in tile (4, 2) at tile 16 and (1, 0) at tile 64; Y(16, 15) in (0, 1) / (0, 0)."""
    H, W, S = 38, 70, 80
    rng = np.random.default_rng(4)
    base = _frame(rng, False, H, S, planar)
    v, y = base.copy(), base.copy()
    v_last = H * S + ((H // 2) * (S // 2) + (H // 2 - 1) * (S // 2) + W // 2 - 1 if planar else (H // 2 - 1) * S + W - 1)
    v[v_last] ^= 0x40
    y[16 * S + 15] ^= 0x03
    for tile, (vi, vj), (yi, yj) in ((16, (4, 2), (0, 1)), (64, (1, 0), (0, 0))):
        m = fmm.frame_error_map(v, base, H, W, tile, S, S, planar)
        assert np.count_nonzero(m["sse"]) == 1 and tuple(m[2, vj, vi]) == (0x40 ** 2, 0x40, 0x40)
        m = fmm.frame_error_map(y, base, H, W, tile, S, S, planar)
        assert np.count_nonzero(m["sse"]) == 1 and tuple(m[0, yj, yi]) == (9, 3, 3)


def test_worst_tiles_and_share_of_a_hand_made_map():
    m = np.zeros((2, 3), fmm.TILE_DTYPE)
    m["sse"] = [[5, 9, 0], [9, 1, 5]]
    m["max_abs"] = [[2, 3, 0], [3, 1, 2]]
    assert fmm.worst_tiles(m, 32, 4) == [{"x": 32, "y": 0, "sse": 9, "max_abs": 3}, {"x": 0, "y": 32, "sse": 9, "max_abs": 3},
                                        {"x": 0, "y": 0, "sse": 5, "max_abs": 2}, {"x": 64, "y": 32, "sse": 5, "max_abs": 2}]
    assert fmm.share_top1pct(m) == 9 / 29
    assert fmm.share_top1pct(np.zeros((2, 3), fmm.TILE_DTYPE)) is None
    big = np.zeros((10, 15), fmm.TILE_DTYPE)   # 150 tiles: the two worst
    big["sse"] = 1
    big["sse"][3, 4], big["sse"][9, 14] = 100, 50
    assert fmm.share_top1pct(big) == 150 / 298
