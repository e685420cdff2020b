"""CPU: the numpy model of the per-tile SSIM maps (tests/frame_ssim_map_model.py) against the definition in include/hopperflow.h --
its totals are frame_ssim_model.frame_ssim's, a window belongs to the tile of its first element, tiles past the last window are zeros --
and the Python view of a downloaded buffer (calc.frame_ssim_maps)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from frame_ssim_cases import n_el, random_frame  # noqa: E402
from frame_ssim_map_model import TILE_DTYPE, TILES, frame_ssim_map, map_shape, totals, window_losses  # noqa: E402
from frame_ssim_model import frame_ssim  # noqa: E402


@pytest.mark.parametrize("planar", [False, True], ids=["semi", "planar"])
@pytest.mark.parametrize("hdr", [False, True], ids=["sdr", "hdr"])
def test_the_tiles_add_up_to_the_frames_ssim(hdr, planar):
    """Per plane the sum of sum_loss_q32, the largest max_loss_q32 and the sum of count over the tiles are hf_frame_ssim's, at every
    tile size, with strides and random padding."""
    rng = np.random.default_rng(5 + 2 * hdr + planar)
    for H, W, sa, sb in ((38, 70, 74, 80), (64, 128, 128, 128), (8, 8, 8, 16), (16, 16, 16, 16), (4, 4, 4, 4), (70, 38, 38, 40)):
        a, b = random_frame(rng, hdr, H, sa), random_frame(rng, hdr, H, sb)
        want = frame_ssim(a, b, H, W, sa, sb, planar)
        for tile in TILES:
            m = frame_ssim_map(a, b, H, W, tile, sa, sb, planar)
            assert m.shape == (3,) + map_shape(H, W, tile) and m.dtype == TILE_DTYPE and TILE_DTYPE.itemsize == 24
            assert totals(m) == want, (H, W, tile)
            assert not m["reserved"].any()
            assert not m["sum_loss_q32"][m["count"] == 0].any() and not m["max_loss_q32"][m["count"] == 0].any()
        same = frame_ssim_map(a, a, H, W, 16, sa, sa, planar)
        assert not same["sum_loss_q32"].any() and not same["max_loss_q32"].any() and totals(same)["Y"]["count"] == want["Y"]["count"]


def test_window_counts_at_70_x_38():
    """70 x 38 at tile 16: 17 x 9 luma blocks are 16 x 8 windows, whose first blocks fill tiles 0 .. 3 across and 0 .. 1 down; the fifth
    tile column (6 elements) and the third row own none.  35 x 19 chroma: 8 x 4 blocks, 7 x 3 windows in tiles of 2 x 2 blocks."""
    rng = np.random.default_rng(1)
    for hdr in (False, True):
        a, b = random_frame(rng, hdr, 38, 70), random_frame(rng, hdr, 38, 70)
        for planar in (False, True):
            m = frame_ssim_map(a, b, 38, 70, 16, planar=planar)
            assert m["count"][0].tolist() == [[16, 16, 16, 16, 0], [16, 16, 16, 16, 0], [0, 0, 0, 0, 0]]
            assert m["count"][1].tolist() == m["count"][2].tolist() == [[4, 4, 4, 2, 0], [2, 2, 2, 1, 0], [0, 0, 0, 0, 0]]
            assert frame_ssim_map(a, b, 38, 70, 32, planar=planar)["count"][0].tolist() == [[64, 64, 0], [0, 0, 0]]
            assert frame_ssim_map(a, b, 38, 70, 64, planar=planar)["count"].reshape(3, -1).tolist() == [[128, 0], [21, 0], [21, 0]]


def test_a_window_is_scored_once_in_the_tile_of_its_first_element():
    """The ownership rule restated per window: each of the 16 x 8 luma windows of 70 x 38 is found, alone, in tile (4 i // 16, 4 j // 16)."""
    rng = np.random.default_rng(2)
    a, b = random_frame(rng, False, 38, 70), random_frame(rng, False, 38, 70)
    loss = window_losses(a[:38 * 70].reshape(38, 70), b[:38 * 70].reshape(38, 70), 255)
    assert loss.shape == (8, 16)
    m = frame_ssim_map(a, b, 38, 70, 16)[0]
    for ty in range(3):
        for tx in range(5):
            own = [int(loss[j, i]) for j in range(8) for i in range(16) if 4 * i // 16 == tx and 4 * j // 16 == ty]
            assert (int(m["sum_loss_q32"][ty, tx]), int(m["max_loss_q32"][ty, tx]), int(m["count"][ty, tx])) == (sum(own), max(own, default=0), len(own))


@pytest.mark.parametrize("hdr", [False, True], ids=["sdr", "hdr"])
def test_one_flipped_luma_element_changes_the_tiles_whose_windows_reach_it(hdr):
    """64 x 64 at tile 16.  Element (15, 15) lies in block (3, 3), the last of tile (0, 0): the windows that hold it start at blocks 2 .. 3
    each way, all of tile (0, 0).  Element (16, 16) lies in block (4, 4), the first of tile (1, 1): its windows start at blocks 3 .. 4
    each way, so the last windows of tiles (0, 0), (1, 0) and (0, 1) reach into it as well."""
    H = W = 64
    rng = np.random.default_rng(3)
    base = random_frame(rng, hdr, H, W)
    top = 65535 if hdr else 255
    zero = frame_ssim_map(base, base, H, W, 16)
    assert not zero["sum_loss_q32"].any()
    for (x, y), tiles in (((15, 15), {(0, 0)}), ((16, 16), {(0, 0), (1, 0), (0, 1), (1, 1)})):
        f = base.copy()
        f[y * W + x] = top - f[y * W + x]
        m = frame_ssim_map(f, base, H, W, 16)
        hit = {(int(i), int(j)) for j, i in np.argwhere(m["sum_loss_q32"][0] > 0)}
        assert hit == tiles, (x, y)
        assert not m["sum_loss_q32"][1:].any() and np.array_equal(m["count"], zero["count"])
        for planar in (False, True):
            assert totals(frame_ssim_map(f, base, H, W, 16, planar=planar)) == frame_ssim(f, base, H, W, planar=planar)


@pytest.mark.parametrize("planar", [False, True], ids=["semi", "planar"])
def test_padding_and_the_unused_remainder_change_nothing(planar):
    """70 x 38 at stride 80: differences confined to the padding columns and to the w & 3 columns / h & 3 rows no block uses."""
    H, W, S = 38, 70, 80
    base = random_frame(np.random.default_rng(5), False, H, S)
    hc, sc = H // 2, S // 2
    uw, uh, cw, ch = 68, 36, 32, 16    # used luma and chroma extents
    if planar:
        u_at = lambda y, x: H * S + y * sc + x
        v_at = lambda y, x: H * S + hc * sc + y * sc + x
        pad = [u_at(0, W // 2), v_at(3, W // 2 + 1)]
    else:
        u_at = lambda y, x: H * S + y * S + 2 * x
        v_at = lambda y, x: H * S + y * S + 2 * x + 1
        pad = [H * S + W, H * S + 5 * S + W + 1]
    unused = [(H - 1) * S + 3, uh * S + uw - 1, 5 * S + uw, 5 * S + W - 1, (H - 1) * S + W,
              u_at(ch, 0), u_at(hc - 1, cw - 1), u_at(2, cw), v_at(ch, 3), v_at(1, W // 2 - 1)] + pad
    f = base.copy()
    for i in unused:
        f[i] = 255 - f[i]
    for tile in TILES:
        m = frame_ssim_map(f, base, H, W, tile, S, S, planar)
        assert np.array_equal(m, frame_ssim_map(base, base, H, W, tile, S, S, planar)) and not m["sum_loss_q32"].any()
    f[(uh - 1) * S + uw - 1] ^= 0xFF    # ... while the last USED luma element shows, in the last tile that owns a window
    m = frame_ssim_map(f, base, H, W, 16, S, S, planar)
    assert [tuple(int(v) for v in t) for t in np.argwhere(m["sum_loss_q32"] > 0)] == [(0, 1, 3)]


def test_the_python_view_of_a_downloaded_buffer():
    """calc.frame_ssim_maps: n maps of 72 th tw bytes as [n][3][th][tw] with the fields of struct hf_ssim_tile; short buffers refused."""
    from hopperrender_amd import calc, capi
    assert calc.SSIM_TILE_DTYPE == TILE_DTYPE and C_sizeof(capi.HfSsimTile) == 24
    rng = np.random.default_rng(7)
    a, b = random_frame(rng, True, 38, 70), random_frame(rng, True, 38, 70)
    ms = [frame_ssim_map(a, b, 38, 70, 16), frame_ssim_map(b, b, 38, 70, 16)]
    raw = np.concatenate([m.reshape(-1).view(np.uint8) for m in ms] + [np.full(64, 0xFF, np.uint8)])
    for buf in (raw, raw.tobytes()):
        got = calc.frame_ssim_maps(buf, 2, 5, 3)
        assert got.shape == (2, 3, 3, 5) and np.array_equal(got[0], ms[0]) and np.array_equal(got[1], ms[1])
    with pytest.raises(ValueError):
        calc.frame_ssim_maps(raw[:2 * 72 * 15 - 1], 2, 5, 3)
    assert n_el(38, 70) == a.size
    assert {"hf_frame_ssim_map_shape", "hf_frame_ssim_map_enqueue"} <= set(capi.SIGNATURES)


def C_sizeof(t):
    import ctypes
    return ctypes.sizeof(t)
