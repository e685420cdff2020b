"""numpy model of the device's per-tile error maps (hf_frame_error_map*, include/hopperflow.h): the sums of tests/frame_error_model.py per
tile of `tile` x `tile` luma pixels -- Y tile (i, j) covers rows [j tile, (j + 1) tile) and columns [i tile, (i + 1) tile) clipped to the
frame, U and V tile (i, j) the chroma rows and columns of the same picture area (tile / 2 each way) -- as a structured array
[3][th][tw] of {sse, sad, max_abs} in the layout of struct hf_error_tile, and what the evaluator derives from a plane's map: the worst
tiles and the share of the error the worst hundredth of the tiles holds.  Shared by the CPU and GPU tests; not a test module itself."""
import numpy as np

from frame_error_model import split_planes

TILES = (16, 32, 64)
TILE_DTYPE = np.dtype([("sse", "<u8"), ("sad", "<u4"), ("max_abs", "<u4")])   # struct hf_error_tile, 16 bytes


def map_shape(H, W, tile):
    """(th, tw)"""
    return (H + tile - 1) // tile, (W + tile - 1) // tile


def _tiled(x, t, th, tw):
    """a plane padded with zeros to th x tw whole tiles of edge t, as [th][t][tw][t]"""
    full = np.zeros((th * t, tw * t), np.int64)
    full[:x.shape[0], :x.shape[1]] = x
    return full.reshape(th, t, tw, t)


def plane_map(a, b, t, th, tw):
    """([th][tw] of TILE_DTYPE, [th][tw] element counts) of two planes of one shape, tile edge t in the plane's own elements"""
    d = np.abs(a.astype(np.int64) - b.astype(np.int64))
    out = np.zeros((th, tw), TILE_DTYPE)
    out["sse"] = _tiled(d * d, t, th, tw).sum(axis=(1, 3))
    out["sad"] = _tiled(d, t, th, tw).sum(axis=(1, 3))
    out["max_abs"] = _tiled(d, t, th, tw).max(axis=(1, 3))
    return out, _tiled(np.ones_like(d), t, th, tw).sum(axis=(1, 3))


def frame_error_map(a, b, H, W, tile, stride_a=0, stride_b=0, planar=False, counts=False):
    """[3][th][tw] of TILE_DTYPE for frames a and b (plane 0 Y, 1 U, 2 V); counts=True: also the [3][th][tw] elements per tile."""
    th, tw = map_shape(H, W, tile)
    pa, pb = split_planes(a, H, W, stride_a, planar), split_planes(b, H, W, stride_b, planar)
    out, cnt = np.zeros((3, th, tw), TILE_DTYPE), np.zeros((3, th, tw), np.int64)
    for p in range(3):
        out[p], cnt[p] = plane_map(pa[p], pb[p], tile if p == 0 else tile // 2, th, tw)
    return (out, cnt) if counts else out


def worst_tiles(m, tile, k=5):
    """the k tiles of largest sse of one plane's map [th][tw]: [{x, y, sse, max_abs}], x and y the luma pixels of the tile's corner;
    ties by lower y, then lower x"""
    th, tw = m.shape
    order = sorted(((-int(m["sse"][j, i]), j, i) for j in range(th) for i in range(tw)))[:k]
    return [{"x": i * tile, "y": j * tile, "sse": -s, "max_abs": int(m["max_abs"][j, i])} for s, j, i in order]


def share_top1pct(m):
    """the share of the plane's sse that its ceil(tiles / 100) worst tiles hold; None where the sse is 0"""
    sse = sorted((int(v) for v in m["sse"].reshape(-1)), reverse=True)
    total = sum(sse)
    return None if total == 0 else sum(sse[:(len(sse) + 99) // 100]) / total
