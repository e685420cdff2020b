"""Which device code builds a frame's phase plane, and the matrix of shapes that holds every builder to the layout model
(tests/phase_plane_model.py) at resolution scalars 0 to 3 -- and, for the planes a batch leaves to its warp launch, at 3 and 4.

Four pieces of device code write a plane (csrc/hf_flow.hip, csrc/hf_phase_plane.h, csrc/hf_kernels.hip):
  * prep_phase_kernel<E>                     "generic": any geometry, through LDS, reflection and clamp per element;
  * prep_phase_fast_kernel<E, RS, NT>        "fast": RS 0 .. 4, no LDS, margins from the tasks' own columns, reversed and luma-swapped; NT (non-
                                             temporal stores) for a launch over more than one frame, default stores for a lone context;
  * plane_fast_task<E, 3 | 4, 1> in warp_wg_kernel   the planes a batch defers: built by the NEXT period's staged warp launch;
  * prep_grid_kernel<E>                      the grid samples such a batch writes at once: phase pair 0, rows cy << rs, columns [0, lw).

builder() restates the decision of hf_flow.hip launch_prep_fast -- hf_launch_plan.h plane_fast_geometry plus the 16-byte alignment of every
frame of the launch; tests/test_plane_builders_model.py holds it to the compiled header over the matrix and over a sweep of widths, and
proves that the matrix reaches what it is for.  tests/test_plane_builders_gpu.py runs it."""
import collections

import numpy as np

import phase_plane_model as P

# offs: byte offsets of the three members' frames from their 256-byte aligned allocations (a lone context is member 0 and, where its
# offset is not 0, is shown its frames by reference: only a referenced frame reaches the builder where the caller put it).
Case = collections.namedtuple("Case", "name hdr H W max_res in_stride offs", defaults=(0, (0, 0, 0)))
# n: members of the batch, odd: the member whose frames sit at base + 8 bytes (its plane is the generic kernel's)
Deferred = collections.namedtuple("Deferred", "name hdr H W max_res in_stride n odd")
Builder = collections.namedtuple("Builder", "kind name reasons")

RAGGED, LW4, MARGIN, PITCH, BASE, DEEP, ODD_H = "ragged W", "lw % 4", "mx > lw", "pitch", "misaligned base", "rs > 4", "odd H"


def geometry(case):
    """(rs, lw, lh) of opticalFlowCalcSDR.cpp:217-222 and the plane layout of a case."""
    rs = 0
    while (case.H >> rs) > case.max_res:
        rs += 1
    lw, lh = -(-case.W >> rs), -(-case.H >> rs)
    return rs, lw, lh, P.layout(case.H, rs, lw, lh)


def stride(case):
    return case.in_stride if case.in_stride > 0 else case.W


def geometry_reasons(case):
    """Why plane_fast_geometry says no ([]: it says yes)."""
    rs, lw_ceil, lh, L = geometry(case)
    lw = case.W >> rs
    out = []
    if (lw << rs) != case.W or lw != lw_ceil:
        out.append(RAGGED)
    if lw & 3:
        out.append(LW4)
    if L.mx > lw:
        out.append(MARGIN)
    assert L.mx % 4 == 0 and L.lwp % 4 == 0          # (by construction of the layout: never a reason)
    if (stride(case) * (2 if case.hdr else 1)) % 16:
        out.append(PITCH)
    if rs > 4:
        out.append(DEEP)
    if case.H & 1:
        out.append(ODD_H)
    return out


def builder(case, batch, copied=False):
    """The kernel that builds the planes of one update: of the lone context (member 0) or of the batch of three.  One misaligned frame
    sends the whole launch to the generic kernel.  copied: the frame is copied into the context's own slot first, which is aligned."""
    rs = geometry(case)[0]
    offs = case.offs if batch else case.offs[:1]
    reasons = geometry_reasons(case) + ([BASE] if any(o % 16 for o in offs) and not copied else [])
    e = "u16" if case.hdr else "u8"
    if reasons:
        return Builder("generic", "generic.%s" % e, tuple(reasons))
    return Builder("fast", "fast.%s.rs%d.%s" % (e, rs, "nt" if batch else "st"), ())


FAST_INSTANTIATIONS = frozenset("fast.%s.rs%d.%s" % (e, rs, st) for e in ("u8", "u16") for rs in range(4) for st in ("st", "nt"))
DEFERRED_INSTANTIATIONS = frozenset(["warp.u16.rs3", "warp.u8.rs4"])


def _c(name, hdr, W, H, max_res, in_stride=0, offs=(0, 0, 0)):
    return Case(name, hdr, H, W, max_res, in_stride, offs)


CASES = [_c("fast-%s-rs%d" % ("u16" if hdr else "u8", rs), hdr, 1024, 64, 64 >> rs) for rs in range(4) for hdr in (0, 1)] + [
    # margins narrower than half the grid: interior tasks store into neither
    _c("fast-u8-rs3-w2048", 0, 2048, 64, 8), _c("fast-u16-rs3-w2048", 1, 2048, 64, 8),
    # mx == lw: every task stores into both margins, and its neighbour on the generic side (4 columns short)
    _c("edge-u8-rs1-mx-eq-lw", 0, 592, 64, 32), _c("edge-u16-rs1-mx-gt-lw", 1, 584, 64, 32),
    # the generic kernel, one reason each
    _c("ragged-u8-rs3", 0, 1028, 64, 8, 1040), _c("ragged-u16-rs2", 1, 1026, 64, 16, 1032),
    _c("lw4-u8-rs0", 0, 1026, 64, 64, 1040), _c("lw4-u16-rs1", 1, 1028, 64, 32, 1032),
    _c("pitch-u8-rs2", 0, 1024, 64, 16, 1026), _c("pitch-u16-rs0", 1, 1024, 64, 64, 1028),
    _c("base8-u16-rs2", 1, 1024, 64, 16, 0, (8, 0, 0)), _c("base8-u8-rs3", 0, 1024, 64, 8, 0, (8, 8, 8)),
    _c("middle8-u8-rs1", 0, 1024, 64, 32, 0, (0, 8, 0)), _c("middle8-u16-rs0", 1, 1024, 64, 64, 0, (0, 8, 0)),
    # fast, with 16 elements of garbage behind every row
    _c("padded-u8-rs3", 0, 1024, 64, 8, 1040), _c("padded-u16-rs1", 1, 1024, 64, 32, 1040),
    # an odd number of chroma rows
    _c("oddrows-u16-rs1", 1, 1024, 66, 33), _c("oddrows-u8-rs2", 0, 1024, 70, 17),
    # grids far narrower than a margin: nearly every margin element clamped
    _c("narrow-u8-rs0", 0, 16, 16, 16), _c("narrow-u16-rs1", 1, 32, 16, 8),
]

# The smallest batches that defer their planes (smallest_deferring below finds them again through the compiled plan).
DEFERRED_CASES = [Deferred("deferred-u16-rs3", 1, 3640, 672, 455, 0, 8, 5), Deferred("deferred-u8-rs4", 0, 3888, 576, 243, 0, 15, 11)]


def case(name):
    return next(c for c in CASES + DEFERRED_CASES if c.name == name)


def g_tuple(c):
    """The geometry as tests/launch_plan_probe.py takes it."""
    rs, lw, lh, _ = geometry(c)
    return (c.hdr, c.H, c.W, stride(c), c.W, rs, lw, lh)


def smallest_deferring(probe, hdr, rs, max_dim=4096):
    """(bytes of all members' frames, n, W, H): the batch of fewest frame bytes for which warp_period_can_build_planes says yes, over
    n <= 16 (a launch takes no more), W in whole 4-column tasks and H in whole grid rows; among equals the fewest members, then the lowest."""
    esz = 2 if hdr else 1
    best = None
    small = probe.constants["kSmallFrameBytes"]           # (a frame up to this size never defers: the scan of H starts above it)
    for n in range(1, 17):
        for W in range(4 << rs, max_dim + 1, 4 << rs):
            for H in range(max(2, small // (W * esz) >> rs) << rs, max_dim + 1, 1 << rs):
                cost = n * (H + H // 2) * W * esz
                if best is not None and (cost, n, H) >= (best[0], best[1], best[3]):
                    break
                c = Deferred("", hdr, H, W, H >> rs, 0, n, 0)
                assert geometry(c)[0] == rs
                if probe.can_build_planes(g_tuple(c), P.max_iterations(*geometry(c)[1:3]), n):
                    best = (cost, n, W, H)
                    break
    return best


# ------------------------------------------------------------------------------------------------
# content
# ------------------------------------------------------------------------------------------------
def noise_frame(c, seed):
    """Every code value everywhere, the padding columns included: P010 low bytes and padding must not show in a plane."""
    rng = np.random.default_rng(seed)
    n = (c.H + c.H // 2) * stride(c)
    return rng.integers(0, 65536, n, dtype=np.uint16) if c.hdr else rng.integers(0, 256, n, dtype=np.uint8)


def frames(c, member, count=3):
    k = (CASES + DEFERRED_CASES).index(c)
    return [noise_frame(c, 1000 * k + 10 * member + i) for i in range(count)]


# ------------------------------------------------------------------------------------------------
# wrong builders: what a case has to tell apart from the model
# ------------------------------------------------------------------------------------------------
NO_SWAP, SAME_ROW, CHROMA_UNREFLECTED, CLAMP, ROUNDED, SECOND_BYTE = "no-swap", "same-row", "chroma-unreflected", "clamp", "rounded", "second-byte"
MARGIN_VARIANTS = (NO_SWAP, SAME_ROW, CHROMA_UNREFLECTED, CLAMP)
VARIANTS = MARGIN_VARIANTS + (ROUNDED, SECOND_BYTE)


def applies(variant, c):
    """no-swap: one luma byte per element at rs 0; same-row: rs 0 and 1 have a single phase-pair row, which is its own mirror; rounded:
    P010 only; second-byte: rs 0 only."""
    rs = geometry(c)[0]
    return {NO_SWAP: rs >= 1, SAME_ROW: rs >= 2, ROUNDED: bool(c.hdr), SECOND_BYTE: rs == 0}.get(variant, True)


def wrong_plane(frame, c, variant):
    """The plane a builder with one flaw would write, in the layout of phase_plane_model.plane (variant None: no flaw -- the model, written
    out a second time).
      no-swap             the margin elements keep the luma byte order of the columns they mirror;
      same-row            the margin of phase-pair row ph2 holds what belongs into that of row nph2 - 1 - ph2;
      chroma-unreflected  the chroma pair of x itself (kept inside the frame) instead of that of the reflected x;
      clamp               no reflection: x and x + 1 clamped to the frame;
      rounded             the top 8 bits of P010 rounded to nearest;
      second-byte         rs 0: the second luma byte holds Y[x + 1] instead of 0."""
    rs, lw, lh, L = geometry(c)
    H, W = c.H, c.W
    f = np.asarray(frame).reshape(-1, stride(c)).astype(np.uint32)
    top = (np.minimum((f + 128) >> 8, 255) if variant == ROUNDED else f >> 8) if c.hdr else f
    Y, C = top[:H, :W], top[H:H + H // 2]
    j = np.arange(-L.mx, lw + L.mx)
    margin = (j < 0) | (j >= lw)
    rows = np.arange(H) >> 1
    out = np.empty((H, L.nph2, j.size), dtype=np.uint32)
    refl = (lambda p: np.clip(p, 0, W - 1)) if variant == CLAMP else (lambda p: P.mirror_clamp(p, W))
    for ph2 in range(L.nph2):
        x = (j << rs) + 2 * ph2
        xa, xb = refl(x), refl(x + 1)
        xc = (np.clip(x, 0, W - 1) if variant == CHROMA_UNREFLECTED else xa) & ~1
        yb = Y[:, xb] if (L.nph > 1 or variant == SECOND_BYTE) else 0
        out[:, ph2, :] = Y[:, xa] | (yb << 8) | (C[rows][:, xc] << 16) | (C[rows][:, xc + 1] << 24)
    if variant == NO_SWAP:
        m = out[:, :, margin]
        out[:, :, margin] = (m & 0xFFFF0000) | ((m & 0xFF) << 8) | ((m >> 8) & 0xFF)
    if variant == SAME_ROW:
        out[:, :, margin] = out[:, ::-1, :][:, :, margin]
    return out


