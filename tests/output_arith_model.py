"""CPU model of the arithmetic every kernel that writes an output frame ends in (csrc/hf_levels.h levels_y / levels_uv, csrc/hf_kernels.hip
warp_element / warp_finish_to / visualize_flow, copy_kernel, csrc/hf_scene.hip scene_copy_kernel), and the inputs that sweep its whole
domain instead of sampling it.  numpy only.

  blend        fma(a, 1 - t, b * t), truncated                                  (warpFrameKernel{SDR,HDR}.h:176-177 as compiled on gfx950)
  levels_y     ((v - black) * rcp(white - black)) * max, clamped, truncated     (:3-5)
  levels_uv    fma((v - mid) * rcp(white), max, mid), clamped, truncated        (:7-9)
  flow_view    mode 3, the HSV view of the flow (:23-113);  flow_magnitude: mode 4 (:161-164)

Every operation is a float32 numpy operation in the order of the device code; the fused multiply-adds are true ones (fma below: the exact
float64 product, the sum rounded to odd, one rounding to float32).  The reciprocal is a parameter (rcp = {y: value}; default 1 / y correctly
rounded): the device divides through v_rcp_f32, which is 1 ulp low for some spans (y = 46080, white 180 on 16-bit frames, is the known
one).  16-bit frames scale black and white by 256 (opticalFlowCalcHDR.cpp:173-174).

With zero flow and t in [0, 1] an output element is a pure function of ONE element of each source frame, so ramp frames drive every code
value through luma, U and V (ramp_frame: every value at an interior position, where mirror_warp leaves the read alone; the partner frame
of the blend holds the ramp reversed).  A 16-bit chroma plane of 128 x 512 has 126 x 255 = 32130 interior U positions, so 65536 code
values need THREE phases there (two cover 8-bit frames many times over): PHASES.

flow_view returns the SET of accepted values of a vector: the hue position u = wheel_pos * 255 (0 .. 1530, one unit = one step of the
rising / falling ramps) is computed in float64 and the model is evaluated at u - DELTA, u and u + DELTA (wrapping at 1530); everything after
u is float32 exactly as visualize_flow writes it.  Most vectors have one accepted value; one whose ramp value or sextant changes within
DELTA has two.  tests/test_output_arith_model.py asserts that at most 3 % of the flow domain has more than one.

`flaw=` selects a deliberately wrong variant; tests/test_output_arith_model.py proves that the committed inputs tell each from the model.
"""
import collections

import numpy as np

F = np.float32
H, W = 256, 512
PHASES = {0: 2, 1: 3}                      # per element type (hdr): see above
CONST = {0: 201, 1: 51457}                 # the constant code value of the flow views' frames (odd: the >> 1 of the luma mix drops a bit)

# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
T = (0.0, 1.0, 0.5, 0.1998, 0.7992, float(np.nextafter(F(1), F(0))))          # the blend scalars


def _levels():
    named = [(0.0, 255.0), (16.0, 235.0), (0.0, 180.0), (3.5, 200.25), (64.0, 192.0), (1.0, 254.0), (0.0, 100.0), (100.0, 255.0), (16.0, 240.0)]
    degenerate = [(200.0, 100.0), (-20.0, 300.0), (0.0, 1e-3)]                # the sane ones of ref_live_cases.LEVELS (white != black, white != 0)
    rng = np.random.default_rng(20240)
    seeded = [(float(b) * 0.25, 128.0 + float(w) * 0.25) for b, w in zip(rng.integers(0, 257, 24), rng.integers(0, 509, 24))]
    return named + degenerate + seeded


LEVELS = _levels()                         # (black, white)
SCENE_LEVELS = [(0.0, 180.0), (16.0, 235.0), (3.5, 200.25)]


def code_max(hdr):
    return 65535 if hdr else 255


def dtype(hdr):
    return np.uint16 if hdr else np.uint8


def interior_masks(h, w):
    """(luma [h][w], chroma [h / 2][w]): not in row or column 0 or dim - 1, where mirror_warp moves the read even at zero flow."""
    y = np.zeros((h, w), bool)
    y[1:h - 1, 1:w - 1] = True
    c = np.zeros((h // 2, w), bool)
    c[1:h // 2 - 1, 1:w - 1] = True
    return y, c


def ramp_frame(hdr, phase, h=H, w=W, stride=0):
    """One NV12 / P010 frame [h + h / 2][stride]: the interior positions of luma, of U and of V each walk through the code values (an odd
    multiplier: neighbours differ in every bit position), phase after phase where one does not hold them all; the rim continues the walk."""
    s = stride or w
    n = code_max(hdr) + 1
    mul = 40503 if hdr else 157
    ym, cm = interior_masks(h, w)
    out = np.zeros((h + h // 2, s), dtype(hdr))

    def fill(plane, mask, salt):
        k = int(mask.sum())
        walk = ((np.arange(plane.size, dtype=np.int64) + phase * k + salt) * mul) % n
        plane[mask] = walk[:k]
        plane[~mask] = walk[k:]

    y = np.zeros((h, w), np.int64)
    fill(y, ym, 0)
    out[:h, :w] = y
    for par, salt in ((0, 11), (1, 23)):
        c = np.zeros((h // 2, w // 2), np.int64)
        fill(c, cm[:, par::2], salt)
        out[h:, par:w:2] = c
    return out.reshape(-1)


def partner_frame(frame, hdr):
    """The second frame of the blend: the ramp reversed."""
    return (code_max(hdr) - frame.astype(np.int64)).astype(dtype(hdr))


def planes(frame, h=H, w=W, stride=0):
    """(luma [h][w], chroma [h / 2][w]) views of the valid columns."""
    s = stride or w
    a = frame.reshape(h + h // 2, s)
    return a[:h, :w], a[h:, :w]


# ------------------------------------------------------------------------------------------------
# levels and blend
# ------------------------------------------------------------------------------------------------
def fma(a, b, c):
    """fl32(a * b + c), ONE rounding: the float64 product of two float32 is exact; its sum with c is rounded to odd (Knuth's two-sum gives the
    error's sign), so that the final rounding to float32 sees what the exact sum would show it."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F).astype(np.float64), np.asarray(b, F).astype(np.float64), np.asarray(c, F).astype(np.float64))
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
    s = np.where((e != 0) & even, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(F)


def rcp_exact(y):
    return F(1) / F(y)


def rcp_one_low(y):
    """The neighbour below the correctly rounded 1 / y (in magnitude): what v_rcp_f32 gives for y = 46080."""
    r = rcp_exact(y)
    return np.nextafter(r, F(0))


def scaled(black, white, hdr):
    k = F(256) if hdr else F(1)
    return F(black) * k, F(white) * k


def rcp_inputs(black, white, hdr):
    """The two values the kernels take the reciprocal of."""
    bk, wh = scaled(black, white, hdr)
    return F(wh - bk), wh


def _rcp(y, rcp):
    if rcp and float(y) in rcp:
        return F(rcp[float(y)])
    return rcp_exact(y)


def _to_code(f, hdr, flaw):
    """fmax(fmin(f, max), 0), truncated to unsigned, & 0xFFFF, stored as the element type."""
    maxv = F(code_max(hdr))
    wrap = 65536
    if flaw == "negative_wraps":
        v = np.trunc(np.minimum(f, maxv)).astype(np.int64) % wrap
    elif flaw == "above_max_wraps":
        v = np.trunc(np.maximum(f, F(0))).astype(np.int64) % wrap
    else:
        f = np.maximum(np.minimum(f, maxv), F(0))
        v = (np.floor(f.astype(np.float64) + 0.5) if flaw == "round_to_nearest" else np.trunc(f)).astype(np.int64) & 0xFFFF
    return v & code_max(hdr)                                                   # the (E) of the store


def levels_y(v, black, white, hdr, rcp=None, flaw=None):
    bk, wh = scaled(black, white, hdr)
    f = ((np.asarray(v).astype(F) - bk) * _rcp(F(wh - bk), rcp)) * F(code_max(hdr))
    return _to_code(f, hdr, flaw)


def levels_uv(v, black, white, hdr, rcp=None, flaw=None):
    bk, wh = scaled(black, white, hdr)
    mid = F(32768 if hdr else 128)
    r = _rcp(F(wh - bk) if flaw == "chroma_by_span" else wh, rcp)
    f = fma((np.asarray(v).astype(F) - mid) * r, F(code_max(hdr)), mid)
    return _to_code(f, hdr, flaw)


def blend(a, b, t, flavour=1):
    """(unsigned)fma(a, 1 - t, b * t) & 0xFFFF for 0 <= t <= 1.  flavour 2: fma(b, t, a * (1 - t)); flavour 0: unfused (oracle flavours)."""
    s12 = F(t)
    s21 = F(1) - s12
    fa, fb = np.asarray(a).astype(F), np.asarray(b).astype(F)
    if flavour == 1:
        bl = fma(fa, s21, fb * s12)
    elif flavour == 2:
        bl = fma(fb, s12, fa * s21)
    else:
        bl = fa * s21 + fb * s12
    return np.trunc(bl).astype(np.int64) & 0xFFFF


def mirror_warp(pos, dim):
    pos = np.asarray(pos)
    res = np.where(pos >= dim - 1, pos - (pos - (dim - 2)) * 2, np.where(pos < 1, -pos + 1, pos))
    return np.clip(res, 1, dim - 2)


def _gather_zero_flow(plane, chroma):
    """What an output plane reads at zero flow: itself away from the rim."""
    h, w = plane.shape
    y = mirror_warp(np.arange(h), h)[:, None]
    x = mirror_warp(np.arange(w), w)[None, :]
    if chroma:
        x = (x & ~1) + (np.arange(w) & 1)[None, :]
    return plane[y, x]


def blend_zero_flow(f12, f21, t, flavour=1, h=H, w=W):
    """The blended planes (luma, chroma) of mode 2 at zero flow, before the output levels."""
    return tuple(blend(_gather_zero_flow(a, cz), _gather_zero_flow(b, cz), t, flavour)
                 for cz, (a, b) in enumerate(zip(planes(f12, h, w), planes(f21, h, w))))


def levels_frame(blended, hdr, black, white, rcp=None, flaw=None):
    """The output frame [h + h / 2][w] of the blended planes."""
    return np.concatenate([levels_y(blended[0], black, white, hdr, rcp, flaw),
                           levels_uv(blended[1], black, white, hdr, rcp, flaw)]).astype(dtype(hdr))


def warp_zero_flow(f12, f21, hdr, t, black, white, rcp=None, flaw=None, flavour=1, h=H, w=W):
    """Mode 2 at zero flow: the output frame [h + h / 2][w] (valid columns of unstrided frames)."""
    return levels_frame(blend_zero_flow(f12, f21, t, flavour, h, w), hdr, black, white, rcp, flaw)


def copy_frame(src, hdr, black, white, rcp=None, flaw=None, h=H, w=W, stride=0):
    y, c = planes(src, h, w, stride)
    return np.concatenate([levels_y(y, black, white, hdr, rcp, flaw), levels_uv(c, black, white, hdr, rcp, flaw)]).astype(dtype(hdr))


def levels_values(frame, hdr, black, white, cz, h=H, w=W):
    """The levels value BEFORE the clamp, in float32 as the kernels compute it: negative and above-maximum elements are where the packed
    16-bit path leans on the conversion instructions."""
    bk, wh = scaled(black, white, hdr)
    v = planes(frame, h, w)[cz].astype(F)
    if cz:
        mid = F(32768 if hdr else 128)
        return fma((v - mid) * rcp_exact(wh), F(code_max(hdr)), mid)
    return ((v - bk) * rcp_exact(F(wh - bk))) * F(code_max(hdr))


# ------------------------------------------------------------------------------------------------
# flow views
# ------------------------------------------------------------------------------------------------
# The float32 hue chain of visualize_flow (hue_u32, numpy float32 arctan2 and fmod) deviates from the float64 position by at most
# 1.8653e-04 units over the flow domain below (the same figure at rs 1 and rs 3: the worst vector lies in |v| <= 48; measured,
# tests/test_output_arith_model.py re-measures it).  DELTA is eight times that: the chain is a handful of roundings, a device atan2f may
# be a few ulp off a correctly rounded one.  At this DELTA 0.51 % (rs 1, gain 4) and 0.33 % (rs 3, gain 1) of the vectors have two
# accepted values in some channel of some element type.
DELTA = 8 * 1.8653e-4
U_WRAP = 1530.0


def hue_u(vx, vy):
    """u = wheel_pos * 255 in float64: 0 .. 1530 around the hue wheel, 255 per sextant."""
    ang = np.arctan2(np.asarray(vy, np.float64), np.asarray(vx, np.float64))
    ang = np.where(ang < 0, ang + 2 * np.pi, ang)
    return np.mod(ang / (2 * np.pi) * U_WRAP, U_WRAP)


def hue_u32(vx, vy):
    """The kernel's float32 chain on the CPU: (position behind `rising`, position behind `falling`), each evaluated exactly from the float32
    values the truncations see: sextant * 255 + frac * 255.0f and (sextant + 1) * 255 - (1.0f - frac) * 255.0f."""
    vx, vy = np.asarray(vx, F), np.asarray(vy, F)
    deg = np.arctan2(vy, vx) * (F(180.0) / F(3.14159274101257))
    deg = np.where(deg < 0, deg + F(360), deg).astype(F)
    deg = np.fmod(deg, F(360))
    deg = np.where(deg < 0, deg + F(360), deg).astype(F)
    wheel = deg / F(360) * F(6)
    sextant = np.trunc(wheel)
    frac = (wheel - sextant).astype(F)
    base = sextant.astype(np.float64) * 255.0
    return base + (frac * F(255)).astype(np.float64), base + 255.0 - ((F(1) - frac) * F(255)).astype(np.float64)


def hue_deviation(vx, vy):
    """max |u32 - u64| over the vectors (around the wheel), zero vectors apart."""
    vx, vy = np.asarray(vx), np.asarray(vy)
    nz = (vx != 0) | (vy != 0)
    u = hue_u(vx[nz], vy[nz])
    worst = 0.0
    for u32 in hue_u32(vx[nz], vy[nz]):
        d = np.abs(u32 - u)
        worst = max(worst, float(np.minimum(d, U_WRAP - d).max()))
    return worst


def _to_byte(v, flaw):
    if flaw == "to_byte_unclamped":
        return np.trunc(v).astype(np.int64) & 0xFF
    return np.trunc(np.maximum(np.minimum(v, F(255)), F(0))).astype(np.int64) & 0xFF


def _view_at(u, ax, ay, blended, channel, gain, hdr, flaw):
    """visualize_flow behind the hue position: float32, operation by operation."""
    u = np.mod(u, U_WRAP)
    sx = np.floor(u / 255.0)
    f = u - 255.0 * sx
    k = sx.astype(np.int64) % 6
    if flaw == "sextant_low_at_boundary":
        k = np.where(f == 0, (k + 5) % 6, k)
    rising = np.trunc(f).astype(np.int64) & 0xFF
    falling = np.trunc(255.0 - f).astype(np.int64) & 0xFF
    wheel = np.stack([np.full_like(k, 255), falling, np.zeros_like(k), np.zeros_like(k), rising, np.full_like(k, 255)])
    zero = (ax == 0) & (ay == 0)
    mag = (ax + ay).astype(F)
    scale = (mag, mag if flaw == "green_by_magnitude" else ay.astype(F) * F(2), mag)
    rgb = []
    for c, rot in enumerate((0, 4, 2)):
        h = np.take_along_axis(wheel, ((k + rot) % 6)[None], 0)[0]
        v = _to_byte(h.astype(F) / F(255) * scale[c] * F(gain), flaw)
        rgb.append(np.where(zero, 0, v).astype(F))
    fr, fg, fb = rgb
    if channel == 0:
        y = np.trunc(np.maximum(np.minimum(fr * F(0.299) + fg * F(0.587) + fb * F(0.114), F(255)), F(0))).astype(np.int64)
        b = np.asarray(blended, np.int64)
        if hdr:
            return (((y & 0xFFFF) << 7) + (b >> 1)) & 0xFFFF
        return (((y & 0xFF) >> 1) + ((b & 0xFF) >> 1)) & 0xFF
    if channel == 1:
        c = fr * F(-0.168736) + fg * F(-0.331264) + fb * F(0.5) + F(128)
    else:
        c = fr * F(0.5) + fg * F(-0.418688) + fb * F(-0.081312) + F(128)
    cb = np.trunc(np.maximum(np.minimum(c, F(255)), F(0))).astype(np.int64)
    return ((cb & 0xFFFF) << 8) & 0xFFFF if hdr else cb & 0xFF


def flow_view(vx, vy, blended, channel, gain, hdr, flaw=None, delta=None):
    """Mode 3 BEFORE the output levels: the accepted values [3][n] of the vectors (vx, vy) -- the flow as visualize_flow is handed it, the
    NEGATED blurred flow -- in `channel` (0 luma, 1 U, 2 V): the model at u - DELTA, u and u + DELTA."""
    vx, vy = np.asarray(vx, np.int64), np.asarray(vy, np.int64)
    d = DELTA if delta is None else delta
    ax, ay = np.abs(vx), np.abs(vy)
    u = hue_u(vx, vy)
    return np.stack([_view_at(u + s * d, ax, ay, blended, channel, gain, hdr, flaw) for s in (-1, 0, 1)])


def single_valued(acc):
    return (acc[0] == acc[1]) & (acc[1] == acc[2])


def flow_magnitude(vx, vy, channel, hdr):
    """Mode 4 (no output levels behind it): |x| + |y| scaled, saturating at 64; chroma is mid grey."""
    mag = np.abs(np.asarray(vx, np.int64)) + np.abs(np.asarray(vy, np.int64))
    if channel:
        return np.full_like(mag, 32768 if hdr else 128)
    return np.minimum(mag << 10, 65535) if hdr else np.minimum(mag << 2, 255)


def gain_of(rs):
    return 4 if rs <= 2 else 1


# ---- the flow domain and its fields ----
FlowGeom = collections.namedtuple("FlowGeom", "rs lw lh max_res")
FLOW_GEOMS = {1: FlowGeom(1, W >> 1, H >> 1, H >> 1), 3: FlowGeom(3, W >> 3, H >> 3, H >> 3)}
SMALL = 48
RINGS = (100, 300)


def chain_reach(g):
    """warp_variant_model.phase_layout's reach: what the flow chain can produce at this shape."""
    d = max(g.lw, g.lh)
    ws0 = d if d & (d - 1) == 0 else 1 << d.bit_length()
    return (ws0.bit_length() - 1 + 1) * 64 + 8


def flow_domain(rs):
    """[n][2] int16, unique: every (vx, vy) with |vx|, |vy| <= 48 (the disc |v| <= 48 and its corners), and rings of 360 directions at
    magnitudes 100, 300 and the chain's reach."""
    a = np.arange(-SMALL, SMALL + 1)
    small = np.stack(np.meshgrid(a, a, indexing="ij"), -1).reshape(-1, 2)
    deg = np.deg2rad(np.arange(360))
    rings = [np.stack([np.rint(m * np.cos(deg)), np.rint(m * np.sin(deg))], -1) for m in RINGS + (chain_reach(FLOW_GEOMS[rs]),)]
    v = np.concatenate([small] + rings).astype(np.int64)
    _, first = np.unique(v, axis=0, return_index=True)
    return v[np.sort(first)].astype(np.int16)


def flow_fields(rs):
    """The domain laid into low-resolution fields: [(field [2][lh][lw] int16, vector index per cell [lh][lw])].  Chroma reads only even grid
    columns and every second grid row (lx & ~1, ly << 1), so a vector fills a block of 2 x 2 cells: luma, U and V all see it.  The last field
    starts the domain over."""
    g = FLOW_GEOMS[rs]
    v = flow_domain(rs)
    by, bx = g.lh // 2, g.lw // 2
    per = by * bx
    out = []
    for f in range(-(-len(v) // per)):
        idx = ((np.arange(per) + f * per) % len(v)).reshape(by, bx)
        idx = np.repeat(np.repeat(idx, 2, 0), 2, 1)
        out.append((np.ascontiguousarray(np.moveaxis(v[idx], -1, 0)), idx))
    return out


def seen(rs, idx, h=H, w=W):
    """Per output element [h + h / 2][w]: (index of the vector its flow lookup returns, channel)."""
    g = FLOW_GEOMS[rs]
    assert idx.shape == (g.lh, g.lw)
    ly, lx = (np.arange(h) >> rs)[:, None], (np.arange(w) >> rs)[None, :]
    cy, cx = ((np.arange(h // 2) >> rs) << 1)[:, None], ((np.arange(w) >> rs) & ~1)[None, :]
    which = np.concatenate([idx[ly, lx], idx[cy, cx]])
    channel = np.concatenate([np.zeros((h, w), np.int64), np.broadcast_to(1 + (np.arange(w) & 1)[None, :], (h // 2, w))])
    return which, channel


def view_tables(rs, hdr, gain=None, flaw=None, rcp=None, levels=(0.0, 255.0)):
    """Per vector of the domain what an output element that sees it holds: (mode 3 accepted [3 values][3 channels][n] behind the output
    levels, mode 4 [3 channels][n]).  The kernels hand visualize_flow the negated flow; mode 4 takes the flow as it is."""
    v = flow_domain(rs).astype(np.int64)
    gain = gain_of(rs) if gain is None else gain
    m3, m4 = [], []
    for ch in range(3):
        acc = flow_view(-v[:, 0], -v[:, 1], CONST[hdr], ch, gain, hdr, flaw)
        m3.append((levels_uv if ch else levels_y)(acc, levels[0], levels[1], hdr, rcp))
        m4.append(flow_magnitude(v[:, 0], v[:, 1], ch, hdr))
    return np.stack(m3, 1), np.stack(m4)


def const_frame(hdr, h=H, w=W):
    return np.full((h + h // 2) * w, CONST[hdr], dtype(hdr))
