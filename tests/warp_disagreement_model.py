"""Model of the device's warp disagreement maps (hf_warp_disagreement_map_enqueue, include/hopperflow.h): for a blending scalar t the map
is the per-tile error map (tests/frame_error_map_model.py) of the two warped halves of the output, the oracle's warp_frames with output
modes 0 (frame N-2 pushed forward by t) and 1 (frame N-1 pulled back by 1 - t).  Two existing things composed, nothing restated.
Shared by the CPU and GPU tests; not a test module itself."""
import numpy as np

from frame_error_map_model import frame_error_map


def warped_halves(f12, f21, flow, g, t):
    """(mode-0 output, mode-1 output) of the oracle at t, each with g.out_stride"""
    from oracle import oracle
    return oracle.warp_frames(f12, f21, flow, g, t, 0), oracle.warp_frames(f12, f21, flow, g, t, 1)


def warp_disagreement_map(f12, f21, flow, g, t, tile):
    """[3][th][tw] of TILE_DTYPE: sse, sad, max_abs of |a - b| per tile, a / b the two warped halves at t"""
    a, b = warped_halves(f12, f21, flow, g, t)
    return frame_error_map(a, b, g.H, g.W, tile, g.out_stride, g.out_stride)


def warp_disagreement_maps(f12, f21, flow, g, ts, tile):
    """[len(ts)][3][th][tw]; a t that occurs twice is computed once"""
    done = {}
    for t in ts:
        if float(t) not in done:
            done[float(t)] = warp_disagreement_map(f12, f21, flow, g, t, tile)
    return np.stack([done[float(t)] for t in ts])
