"""CPU: the model of the warp disagreement maps (tests/warp_disagreement_model.py) against the two things it composes: the oracle's warped
halves and the frame error model.  Per plane the tile sums add up to the frame error of the two warps; equal frames with zero flow
disagree nowhere; a single differing element lands in exactly one tile of one plane."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import warp_disagreement_model as wdm  # noqa: E402
from frame_error_map_model import TILES, map_shape  # noqa: E402
from frame_error_model import PLANES, frame_error  # noqa: E402


def _geom(hdr, H, W, max_calc_res=270):
    from oracle import oracle
    return oracle.make_geom(int(hdr), H, W, 0, 0, max_calc_res)


def _frame(rng, hdr, g):
    from oracle import oracle
    return rng.integers(0, 65536 if hdr else 256, size=oracle.in_elems(g), dtype=oracle.frame_dtype(hdr))


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("hdr", [False, True], ids=["sdr", "hdr"])
def test_tile_sums_add_up_to_the_frame_error_of_the_two_warps(hdr, tile):
    H, W = 50, 86
    g = _geom(hdr, H, W, 25)   # rs = 1
    rng = np.random.default_rng(3 + hdr)
    f12, f21 = _frame(rng, hdr, g), _frame(rng, hdr, g)
    flow = rng.integers(-20, 21, size=(2, g.lh, g.lw)).astype(np.int16)
    for t in (0.0, 0.3996, 1.0):
        m = wdm.warp_disagreement_map(f12, f21, flow, g, t, tile)
        a, b = wdm.warped_halves(f12, f21, flow, g, t)
        want = frame_error(a, b, H, W, g.out_stride, g.out_stride)
        assert m.shape == (3,) + map_shape(H, W, tile)
        for i, p in enumerate(PLANES):
            assert int(m["sse"][i].astype(object).sum()) == want[p]["sse"] > 0
            assert int(m["sad"][i].astype(object).sum()) == want[p]["sad"]
            assert int(m["max_abs"][i].max()) == want[p]["max_abs"]


@pytest.mark.parametrize("hdr", [False, True], ids=["sdr", "hdr"])
def test_equal_frames_with_zero_flow_disagree_nowhere(hdr):
    g = _geom(hdr, 50, 86)
    f = _frame(np.random.default_rng(8), hdr, g)
    flow = np.zeros((2, g.lh, g.lw), np.int16)
    m = wdm.warp_disagreement_maps(f, f, flow, g, [0.0, 0.5, 1.0], 16)
    assert m.shape == (3, 3, 4, 6) and not m.view(np.uint8).any()


@pytest.mark.parametrize("plane,row,col,tile_at", [(0, 37, 70, (2, 4)), (1, 20, 33 * 2, (2, 4)), (2, 3, 5 * 2 + 1, (0, 0))],
                         ids=["Y", "U", "V"])
def test_a_single_differing_element_lands_in_one_tile_of_one_plane(plane, row, col, tile_at):
    """Zero flow: both halves are the source frames themselves but for the mirrored border (rows and columns 0 and last read their
    neighbours), so one interior element that differs between the frames is one difference of the halves."""
    H, W, tile = 50, 86, 16
    g = _geom(False, H, W)
    f12 = _frame(np.random.default_rng(2), False, g)
    f21 = f12.copy()
    at = (H * g.in_stride if plane else 0) + row * g.in_stride + col
    f21[at] = 255 - f21[at]
    d = abs(int(f21[at]) - int(f12[at]))
    m = wdm.warp_disagreement_map(f12, f21, np.zeros((2, g.lh, g.lw), np.int16), g, 0.5, tile)
    assert np.count_nonzero(m["sse"]) == 1
    assert tuple(m[plane][tile_at]) == (d * d, d, d)
