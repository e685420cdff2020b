"""Reference for the planar 4:2:0 layout of HF_FLAG_PLANAR_IN / HF_FLAG_PLANAR_OUT (include/hopperflow.h), on the host, with strides:
a planar frame of H rows, stride S, width W holds Y at y S + x, U at H S + m (S/2) + k and V at H S + (H/2)(S/2) + m (S/2) + k; the
semi-planar twin (NV12 / P010) holds Y at y S + x and U / V at H S + m S + 2k (+1).  HDR planar values are LSB-aligned: << 6 in
(wrapping in 16 bits), >> 6 out -- the rules of hopperrender_amd/y4m.py, which these functions equal when S = W."""
import numpy as np


def _dt(hdr):
    return np.uint16 if hdr else np.uint8


def planar_planes(p, H, W, S):
    """(Y[H][W], U[H/2][W/2], V[H/2][W/2]) views of the valid columns of a planar frame."""
    p = np.asarray(p).reshape(-1)
    n_y, n_c = H * S, (H // 2) * (S // 2)
    y = p[:n_y].reshape(H, S)[:, :W]
    u = p[n_y:n_y + n_c].reshape(H // 2, S // 2)[:, :W // 2]
    v = p[n_y + n_c:n_y + 2 * n_c].reshape(H // 2, S // 2)[:, :W // 2]
    return y, u, v


def semiplanar_planes(f, H, W, S):
    """(Y, U, V) views of the valid columns of an NV12 / P010 frame, values as stored."""
    f = np.asarray(f).reshape(-1)
    y = f[:H * S].reshape(H, S)[:, :W]
    uv = f[H * S:H * S + (H // 2) * S].reshape(H // 2, S)[:, :W]
    return y, uv[:, 0::2], uv[:, 1::2]


def planar_to_semiplanar(p, H, W, S, hdr, pad=0):
    """The NV12 / P010 frame the device makes of planar frame p (padding columns set to `pad`)."""
    y, u, v = planar_planes(p, H, W, S)
    out = np.full(H * S * 3 // 2, pad, dtype=_dt(hdr))
    oy = out[:H * S].reshape(H, S)
    ouv = out[H * S:].reshape(H // 2, S)
    oy[:, :W] = y
    ouv[:, 0:W:2] = u
    ouv[:, 1:W:2] = v
    if hdr:
        oy[:, :W] <<= 6
        ouv[:, :W] <<= 6
    return out


def semiplanar_to_planar(f, H, W, S, hdr, pad=0):
    """The planar frame of NV12 / P010 frame f (HDR: >> 6; padding columns set to `pad`)."""
    y, u, v = semiplanar_planes(f, H, W, S)
    out = np.full(H * S * 3 // 2, pad, dtype=_dt(hdr))
    n_y, n_c = H * S, (H // 2) * (S // 2)
    oy = out[:n_y].reshape(H, S)
    ou = out[n_y:n_y + n_c].reshape(H // 2, S // 2)
    ov = out[n_y + n_c:].reshape(H // 2, S // 2)
    sh = 6 if hdr else 0
    oy[:, :W] = y >> sh
    ou[:, :W // 2] = u >> sh
    ov[:, :W // 2] = v >> sh
    return out


def valid_planes_of_output(frame, H, W, S, hdr, planar):
    """What a test compares: the valid columns of an output frame as planar (Y, U, V), HDR as 10-bit codes."""
    if planar:
        return tuple(np.ascontiguousarray(a) for a in planar_planes(frame, H, W, S))
    sh = 6 if hdr else 0
    return tuple(np.ascontiguousarray(a >> sh) for a in semiplanar_planes(frame, H, W, S))
