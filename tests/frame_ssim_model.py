"""numpy model of the device's windowed SSIM (hf_frame_ssim*, include/hopperflow.h has the six steps): per plane Y, U, V of two frames of
one geometry the summed and the largest window loss 2^32 - llrint(ssim 2^32) and the number of windows -- 4 x 4 integer block sums, 2 x 2
blocks per window, integer constants from the peak, two float64 multiplications and one division per window.  Plain Python ints, so a test
compares for equality.  Shared by the CPU and GPU tests; not a test module itself."""
import numpy as np

from frame_error_model import split_planes

PLANES = ("Y", "U", "V")
FIELDS = ("sum_loss_q32", "max_loss_q32", "count")
ONE = 1 << 32


def constants(peak):
    return (64 * peak * peak + 5000) // 10000, (9 * 64 * 63 * peak * peak + 5000) // 10000


def window_terms(a, b, peak):
    """(A, B, C, D) as int64 arrays [bh - 1][bw - 1] of two planes of compared elements; None where the plane has no window."""
    h, w = a.shape
    bw, bh = w >> 2, h >> 2
    if bw < 2 or bh < 2:
        return None
    a = a[:4 * bh, :4 * bw].astype(np.int64).reshape(bh, 4, bw, 4)
    b = b[:4 * bh, :4 * bw].astype(np.int64).reshape(bh, 4, bw, 4)
    win = lambda s: s[:-1, :-1] + s[:-1, 1:] + s[1:, :-1] + s[1:, 1:]
    S1, S2, SS, S12 = (win(x.sum(axis=(1, 3))) for x in (a, b, a * a + b * b, a * b))
    c1, c2 = constants(peak)
    var, covar = 64 * SS - S1 * S1 - S2 * S2, 64 * S12 - S1 * S2
    return 2 * S1 * S2 + c1, 2 * covar + c2, S1 * S1 + S2 * S2 + c1, var + c2


def plane_ssim(a, b, peak):
    t = window_terms(a, b, peak)
    if t is None:
        return {"sum_loss_q32": 0, "max_loss_q32": 0, "count": 0}
    A, B, C, D = (x.astype(np.float64) for x in t)
    ssim = (A * B) / (C * D)
    loss = ONE - np.rint(ssim * 4294967296.0).astype(np.int64)
    return {"sum_loss_q32": sum(int(x) for x in loss.sum(axis=1)), "max_loss_q32": int(loss.max()), "count": int(loss.size)}


def frame_ssim(a, b, H, W, stride_a=0, stride_b=0, planar=False, peak=None):
    """{'Y': {sum_loss_q32, max_loss_q32, count}, 'U': ..., 'V': ...} of frames a and b; peak None: the format's own (255; 16 bit: 65535
    semi-planar, 1023 planar)."""
    if not peak:
        peak = 255 if np.asarray(a).dtype.itemsize == 1 else 1023 if planar else 65535
    pa, pb = split_planes(a, H, W, stride_a, planar), split_planes(b, H, W, stride_b, planar)
    return {p: plane_ssim(x, y, peak) for p, x, y in zip(PLANES, pa, pb)}


def derived(d):
    """the floats the Python layer adds to a plane's integers: mean and worst-window SSIM, None where there is no window"""
    n = d["count"]
    return {"ssim": 1.0 - d["sum_loss_q32"] / 4294967296.0 / n if n else None, "min_ssim": 1.0 - d["max_loss_q32"] / 4294967296.0 if n else None}
