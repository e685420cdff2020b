"""Model of the device's guarded blend (hf_guarded_blend_enqueue, include/hopperflow.h): the oracle's mode-2 frame with the flow as it is
(M) and with a zero flow (Z, the cross-fade), the model of the warp disagreement maps (tests/warp_disagreement_model.py), and the integer
weights of steps 3 to 5 of the definition in numpy int64, written element by element from the definition (calc.guard_weights is the
vectorised form a user calls; the tests hold the two to each other).  Nothing of the warp is restated.
Shared by the CPU and GPU tests; not a test module itself."""
import numpy as np

from warp_disagreement_model import warp_disagreement_maps

GUARD_OFF = (4080, 4081)


def tile_weights(maps, tile, lo_q4, hi_q4, H, W, hdr):
    """step 3: [n][th][tw] int64 from the luma sad of maps [n][3][th][tw]"""
    n, _, th, tw = maps.shape
    wt = np.zeros((n, th, tw), np.int64)
    for ty in range(th):
        for tx in range(tw):
            cnt = np.int64(min(tile, H - ty * tile) * min(tile, W - tx * tile))
            for k in range(n):
                m = (np.int64(16) * np.int64(maps["sad"][k, 0, ty, tx])) // (cnt << np.int64(8 if hdr else 0))
                wt[k, ty, tx] = 0 if m <= lo_q4 else 256 if m >= hi_q4 else ((m - lo_q4) * 256) // (hi_q4 - lo_q4)
    return wt


def _axis(n, tile, n_tiles):
    """step 4 along one axis: (index 0, index 1, fraction) per position"""
    lg = tile.bit_length() - 1
    u = np.arange(n, dtype=np.int64) - tile // 2
    t0 = u >> lg
    return np.clip(t0, 0, n_tiles - 1), np.clip(t0 + 1, 0, n_tiles - 1), u & (tile - 1)


def luma_weights(wt, tile, H, W):
    """step 4: [n][H][W] int64 from tile weights [n][th][tw]"""
    n, th, tw = wt.shape
    lg = tile.bit_length() - 1
    ty0, ty1, fy = _axis(H, tile, th)
    tx0, tx1, fx = _axis(W, tile, tw)
    w = np.empty((n, H, W), np.int64)
    for y in range(H):
        a, b = wt[:, ty0[y]], wt[:, ty1[y]]       # [n][tw]
        w[:, y] = ((tile - fx) * (tile - fy[y]) * a[:, tx0] + fx * (tile - fy[y]) * a[:, tx1] + (tile - fx) * fy[y] * b[:, tx0] + fx * fy[y] * b[:, tx1]
                   + tile * tile // 2) >> (2 * lg)
    return w


def element_weights(w_luma, H, W, stride):
    """the weight of every element of a frame [n][H + H/2][stride] (padding columns 0): luma its own, chroma (cx, cy) that of (cx & ~1, 2 cy)"""
    n = w_luma.shape[0]
    w = np.zeros((n, H + H // 2, stride), np.int64)
    w[:, :H, :W] = w_luma
    cx = np.arange(W) & ~1
    w[:, H:, :W] = w_luma[:, 0:2 * (H // 2):2][:, :, cx]
    return w


def mix(M, Z, w):
    """step 5 on arrays of one shape"""
    return (M.astype(np.int64) * (256 - w) + Z.astype(np.int64) * w + 128) >> 8


def halves(f12, f21, flow, g, t, black=0.0, white=255.0):
    """(M, Z): the oracle's mode-2 output at t with the flow and with a zero flow, each with g.out_stride"""
    from oracle import oracle
    return (oracle.warp_frames(f12, f21, flow, g, t, 2, black, white), oracle.warp_frames(f12, f21, np.zeros_like(flow), g, t, 2, black, white))


def guarded_blend(f12, f21, flow, g, ts, tile, lo_q4, hi_q4, black=0.0, white=255.0):
    """(frames [n][H + H/2][out_stride] of the frame dtype with the padding columns 0, maps [n][3][th][tw], element weights like frames)"""
    from oracle import oracle
    H, W = g.H, g.W
    maps = warp_disagreement_maps(f12, f21, flow, g, ts, tile)
    w = element_weights(luma_weights(tile_weights(maps, tile, lo_q4, hi_q4, H, W, g.hdr), tile, H, W), H, W, g.out_stride)
    out = np.zeros(w.shape, oracle.frame_dtype(g.hdr))
    done = {}
    for k, t in enumerate(ts):
        if float(t) not in done:
            done[float(t)] = [x.reshape(H + H // 2, g.out_stride) for x in halves(f12, f21, flow, g, t, black, white)]
        M, Z = done[float(t)]
        out[k] = mix(M, Z, w[k])
    return out, maps, w


# ---- the inputs the tests share: frames and thresholds under which a case cannot degenerate to a copy ----
def guard_frames(rng, hdr, g):
    """Frames N-2 / N-1 (and a third) of random samples; the left third of N-1 is that of N-2, so under a zero flow the halves agree there
    and disagree by the mean of random samples everywhere else."""
    from oracle import oracle
    f = [rng.integers(0, 65536 if hdr else 256, size=oracle.in_elems(g), dtype=oracle.frame_dtype(hdr)) for _ in range(3)]
    rows = lambda x: x.reshape(g.H + g.H // 2, g.in_stride)
    rows(f[1])[:, :(g.W // 3) & ~1] = rows(f[0])[:, :(g.W // 3) & ~1]
    return f


def q4_means(maps, tile, H, W, hdr):
    """m of step 3 per tile: [n][th][tw] int64"""
    _, _, th, tw = maps.shape
    cnt = np.minimum(tile, H - tile * np.arange(th, dtype=np.int64))[:, None] * np.minimum(tile, W - tile * np.arange(tw, dtype=np.int64))[None, :]
    return (16 * maps["sad"][:, 0].astype(np.int64)) // (cnt << (8 if hdr else 0))


def thresholds_around(maps, tile, H, W, hdr):
    """(lo_q4, hi_q4) inside the range of the maps' nonzero means: the lower and upper third of their distinct values, or with fewer than
    six of them (one tile) the least and the greatest, so that some tile is at or below lo, some at or above hi and some strictly between"""
    d = np.unique(q4_means(maps, tile, H, W, hdr))
    d = d[d > 0]
    assert len(d) >= 3, d
    lo, hi = (int(d[len(d) // 3]), int(d[2 * len(d) // 3])) if len(d) >= 6 else (int(d[0]), int(d[-1]))
    return lo, hi
