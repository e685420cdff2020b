"""numpy model of the device's frame error sums (hf_frame_error*, include/hopperflow.h): for each plane Y, U, V of two frames of one
geometry the sum of squared differences, the sum of absolute differences, the largest absolute difference, the number of differing
elements and the number of elements compared -- over columns [0, W) only (chroma: [0, W/2)), each side with its own stride in elements.
Plain Python ints, so a test compares for equality.  Shared by the CPU and GPU tests; not a test module itself."""
import numpy as np

PLANES = ("Y", "U", "V")
FIELDS = ("sse", "sad", "max_abs", "n_differ", "count")


def split_planes(frame, H, W, stride=0, planar=False):
    """(Y, U, V) views of the compared elements of a flat frame: H x W luma, H/2 x W/2 chroma; padding columns left out.
    Semi-planar (NV12 / P010): Y rows, then rows of interleaved U, V.  Planar: Y rows of `stride`, then U and V rows of stride / 2."""
    S = stride or W
    f = np.asarray(frame).reshape(-1)
    hc, wc = H // 2, W // 2
    y = f[:H * S].reshape(H, S)[:, :W]
    if planar:
        sc = S // 2
        u = f[H * S:H * S + hc * sc].reshape(hc, sc)[:, :wc]
        v = f[H * S + hc * sc:H * S + 2 * hc * sc].reshape(hc, sc)[:, :wc]
    else:
        uv = f[H * S:H * S + hc * S].reshape(hc, S)
        u, v = uv[:, 0:2 * wc:2], uv[:, 1:2 * wc:2]
    return y, u, v


def plane_error(a, b):
    d = np.abs(a.astype(np.int64) - b.astype(np.int64))
    return {"sse": int((d * d).sum()), "sad": int(d.sum()), "max_abs": int(d.max()) if d.size else 0,
            "n_differ": int(np.count_nonzero(d)), "count": int(d.size)}


def frame_error(a, b, H, W, stride_a=0, stride_b=0, planar=False):
    """{'Y': {sse, sad, max_abs, n_differ, count}, 'U': ..., 'V': ...} of frames a and b."""
    pa, pb = split_planes(a, H, W, stride_a, planar), split_planes(b, H, W, stride_b, planar)
    return {p: plane_error(x, y) for p, x, y in zip(PLANES, pa, pb)}


def psnr(sse, count, peak):
    """10 log10(peak^2 count / sse); None where the frames are equal."""
    import math
    return None if sse == 0 else 10.0 * math.log10(float(peak) ** 2 * count / sse)
