"""numpy model of the device's per-tile SSIM maps (hf_frame_ssim_map*, include/hopperflow.h): the window losses of
tests/frame_ssim_model.py kept per tile of the error maps' grid.  Window (i, j) of a plane covers elements 4 i .. 4 i + 7 by
4 j .. 4 j + 7 and belongs to the ONE tile that holds its first element, tile (4 i // te, 4 j // te) with te = tile for Y and tile / 2
for U and V.  Returns a structured array [3][th][tw] of {sum_loss_q32, max_loss_q32, count, reserved} in the layout of struct
hf_ssim_tile, and what the evaluator derives from a plane's map.  Shared by the CPU and GPU tests; not a test module itself."""
from fractions import Fraction

import numpy as np

import frame_ssim_model as fsm
from frame_error_map_model import map_shape
from frame_error_model import split_planes

TILES = (16, 32, 64)
TILE_DTYPE = np.dtype([("sum_loss_q32", "<u8"), ("max_loss_q32", "<u8"), ("count", "<u4"), ("reserved", "<u4")])   # struct hf_ssim_tile, 24 bytes


def window_losses(a, b, peak):
    """int64 [bh - 1][bw - 1] losses of two planes of compared elements; None where the plane has no window"""
    t = fsm.window_terms(a, b, peak)
    if t is None:
        return None
    A, B, C, D = (x.astype(np.float64) for x in t)
    return fsm.ONE - np.rint((A * B) / (C * D) * 4294967296.0).astype(np.int64)


def plane_map(a, b, te, th, tw, peak):
    """[th][tw] of TILE_DTYPE of two planes of one shape, tile edge te in the plane's own elements"""
    out = np.zeros((th, tw), TILE_DTYPE)
    loss = window_losses(a, b, peak)
    if loss is None:
        return out
    ty, tx = np.meshgrid(4 * np.arange(loss.shape[0]) // te, 4 * np.arange(loss.shape[1]) // te, indexing="ij")   # the owner of window (i, j)
    total, worst, count = (np.zeros((th, tw), np.int64) for _ in range(3))
    np.add.at(total, (ty, tx), loss)
    np.maximum.at(worst, (ty, tx), loss)
    np.add.at(count, (ty, tx), 1)
    out["sum_loss_q32"], out["max_loss_q32"], out["count"] = total, worst, count
    return out


def frame_ssim_map(a, b, H, W, tile, stride_a=0, stride_b=0, planar=False, peak=None):
    """[3][th][tw] of TILE_DTYPE for frames a and b (plane 0 Y, 1 U, 2 V); peak None: the format's own, as frame_ssim_model.frame_ssim"""
    if not peak:
        peak = 255 if np.asarray(a).dtype.itemsize == 1 else 1023 if planar else 65535
    th, tw = map_shape(H, W, tile)
    pa, pb = split_planes(a, H, W, stride_a, planar), split_planes(b, H, W, stride_b, planar)
    out = np.zeros((3, th, tw), TILE_DTYPE)
    for p in range(3):
        out[p] = plane_map(pa[p], pb[p], tile if p == 0 else tile // 2, th, tw, peak)
    return out


def totals(m):
    """{'Y': {sum_loss_q32, max_loss_q32, count}, ...} of one map [3][th][tw]: what frame_ssim_model.frame_ssim gives for the frames"""
    return {p: {"sum_loss_q32": sum(int(v) for v in m[i]["sum_loss_q32"].flat), "max_loss_q32": max(int(v) for v in m[i]["max_loss_q32"].flat),
                "count": sum(int(v) for v in m[i]["count"].flat)} for i, p in enumerate(fsm.PLANES)}


def worst_tiles(m, tile, sse=None, k=5):
    """the k tiles of lowest mean SSIM of one plane's map [th][tw] -- largest sum_loss_q32 / count as an exact fraction, ties by lower y,
    then lower x, tiles without a window left out -- as the evaluator reports them; sse: [th][tw] squared errors to join, or None"""
    th, tw = m.shape
    order = sorted((-Fraction(int(m["sum_loss_q32"][j, i]), int(m["count"][j, i])), j, i) for j in range(th) for i in range(tw) if m["count"][j, i])[:k]
    out = []
    for _, j, i in order:
        d = {f: int(m[f][j, i]) for f in fsm.FIELDS}
        out.append(dict({"x": i * tile, "y": j * tile}, **fsm.derived(d), **d))
        if sse is not None:
            out[-1]["sse"] = int(sse[j, i])
    return out


def worst_window_tile(m, tile):
    """{x, y, max_loss_q32} of the tile that holds the plane's largest window loss, ties by lower y, then lower x; None without a window"""
    th, tw = m.shape
    order = sorted((-int(m["max_loss_q32"][j, i]), j, i) for j in range(th) for i in range(tw) if m["count"][j, i])
    return {"x": order[0][2] * tile, "y": order[0][1] * tile, "max_loss_q32": -order[0][0]} if order else None


def pgm_values(m):
    """the bytes of the evaluator's heat map of one plane's map: round(255 min(1, sum / count / 2^32)), 0 without a window"""
    return [0 if not c else int(round(255.0 * min(1.0, int(s) / int(c) / 4294967296.0))) for s, c in zip(m["sum_loss_q32"].flat, m["count"].flat)]
