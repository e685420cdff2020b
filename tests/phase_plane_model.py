"""numpy model of the phase plane (csrc/hf_launch_plan.h make_phase_layout, csrc/hf_flow.hip prep_phase_kernel,
csrc/hf_phase_plane.h plane_fast_task), for the tests that hold the plane builders to the documented layout.

    PP[y][ph2][j], j in [-mx, lw + mx):  Y[y][x] | Y[y][x + 1] << 8 | U[y >> 1][x & ~1] << 16 | V[y >> 1][x & ~1] << 24    (top 8 bits each)
    x = (j << rs) + 2 ph2;  x and x + 1 each reflected once at the frame edge (calcDeltaSumsKernelSDR.h:86-95), then clamped; the chroma
    pair is that of the reflected x.  rs = 0: one luma phase, the second luma byte is 0.

layout() restates make_phase_layout; tests/test_chain_deep_rs_model.py holds it to the compiled header through tests/launch_plan_probe.cpp."""
import collections

import numpy as np

Layout = collections.namedtuple("Layout", "rs nph nph2 mx lwp bytes")


def max_iterations(lw, lh):
    """hf_context.hip: log2 of the chain's initial window, half the power of two that covers the grid (hf_oracle.c hfo_initial_window)."""
    return max((max(lw, lh) - 1).bit_length() - 1, 0)


def layout(H, rs, lw, lh):
    nph = 1 << rs
    nph2 = max(1, nph // 2)
    reach = (max_iterations(lw, lh) + 1) * 64 + 8
    mx = ((reach >> rs) + 2 + 3) // 4 * 4
    lwp = (lw + 2 * mx + 4 + 31) // 32 * 32
    return Layout(rs, nph, nph2, mx, lwp, H * nph2 * lwp * 4)


def mirror_clamp(p, dim):
    p = np.where(p >= dim, 2 * dim - p - 1, np.where(p < 0, -p - 1, p))
    return np.clip(p, 0, dim - 1)


def plane(frame, hdr, H, W, in_stride, L, lw):
    """uint32 [H][nph2][lw + 2 mx]: the columns in use (plane column j + mx) of the plane of one NV12 / P010 frame."""
    S = in_stride if in_stride > 0 else W
    f = np.asarray(frame).reshape(-1, S)
    top = (f >> 8 if hdr else f).astype(np.uint32)
    Y, C = top[:H, :W], top[H:H + H // 2, :]
    j = np.arange(-L.mx, lw + L.mx)
    out = np.empty((H, L.nph2, j.size), dtype=np.uint32)
    rows = np.arange(H) >> 1
    for ph2 in range(L.nph2):
        x = (j << L.rs) + 2 * ph2
        xa = mirror_clamp(x, W)
        xc = xa & ~1
        yb = Y[:, mirror_clamp(x + 1, W)] if L.nph > 1 else 0
        out[:, ph2, :] = Y[:, xa] | (yb << 8) | (C[rows][:, xc] << 16) | (C[rows][:, xc + 1] << 24)
    return out


def used(words, H, L, lw):
    """The same columns of a plane as hf_read_phase_plane returns it."""
    return np.asarray(words).reshape(H, L.nph2, L.lwp)[:, :, :lw + 2 * L.mx]
