"""CPU model of which warp kernel a launch runs and which body every workgroup of the staged kernel takes (csrc/hf_launch_plan.h
plan_warp_periods, plan_warp_launch, warp_fast_shape, plan_warp_generic, plan_copy, warp_period_can_build_planes, plane_emission_geometry;
csrc/hf_kernels.hip launch_warp, launch_warp_periods, warp_wg_body).  numpy only.

The launchers choose by element type, resolution scalar, frame bytes, strides, pointer alignment, batch size, outputs per period and mode;
inside warp_wg_kernel every workgroup then stages a window (interior, or mirror-extended at a frame edge), takes the interior global path
or the generic body.  All three bodies give the same pixels, so only this model and the device counters can tell that the staged body ran.
The launch selection restated here is compared with the launchers' plan functions by tests/test_warp_variant_model.py (every shape of its
sweep, field by field), which pins the workgroup decision to the device code and proves that CASES -- the matrix
tests/test_warp_variants_gpu.py runs against the oracle -- reaches every label and every workgroup class the model knows.

Launch labels
  fast.<e>.vb<8|16>.g<G>.<dw|nodw>.<one|all>.w<4|16>   warp_fast_kernel<E, G, 2, MODE, VB, DW>; one / all outputs of the period per thread
                                                       (out_chunk 1 / kMaxWarpOutputs), waves per workgroup
  staged.<e>.rs<n>[.planes]                            warp_wg_kernel<E, MODE, 4, 2>; .planes: the launch carries plane-building workgroups
  generic.<e>.<aligned|unaligned>                      warp_kernel<E, 16 / sizeof(E), ALIGNED> (one output per launch)
  copy.<e>.<aligned|unaligned>                         copy_kernel<E, 16 / sizeof(E), ALIGNED>
  split                                                a batch of more than kMaxWarpBatch members: two launches
  plane.<e>.rs<3|4>                                    plane_fast_task<E, 3 | 4, 1> inside a staged launch;  plane.fallback: a member of such a
                                                       launch whose frame is not 16-byte aligned keeps its plane for the stand-alone kernel
<e> = u8 | u16.  The mode (0, 1, 2) is a template argument of the fast and the staged kernels: CASES must reach every label in each.

Workgroup classes of the staged kernel, per element type and plane (y / uv)
  staged.interior   staged.edge.left / .right / .top / .bottom (a corner window is two of them; right: luma only)
  global            every run interior, the window does not fit the LDS budget
  generic.partial   generic.beyond_extension   generic.chroma_right_zone   generic.edge_no_fit

The device counters (hopperflow_diag.h warp_workgroups) are the leader's, all members and launches together.  A single context's
one-output launch (launch_warp_t) passes no counters and never takes the staged kernel (it needs two outputs); nothing is added for it.
"""
import collections

import numpy as np

# constants of csrc/hf_launch_plan.h and hf_kernels.hip (compared with the launchers' plan functions by tests/test_warp_variant_model.py)
WARP_TX, WARP_TY = 16, 4                  # kWarpTX, kWarpTY
WAVES_SMALL, WAVES_LARGE = 4, 16          # kWarpWavesSmall, kWarpWavesLarge
WG_WAVES, WG_ROWS, WG_CHUNKS_PER_WAVE = 4, 2, 192
WG_MIN_WAVES = 4 * 8192                   # kWgMinWaves
ROUNDS = 4 * 8192                         # the literal of the out_chunk and wpb conditions
EXT_X, EXT_Y = 64, 64                     # kExtX, kExtY
WG_CELLS = 64                             # kWgCells
MAX_WARP_BATCH, MAX_WARP_OUTPUTS, MAX_FLOW_BATCH = 16, 6, 32
SMALL_FRAME_BYTES = 1920 * 1088           # warp_small_frame / warp_period_can_build_planes; launch_warp_fast's small_frame: twice that
NDW = 4                                   # dwords of a 16-byte run (a run spans NDW + 1 from the dword of its first byte)
FAST_ROWS = 2                             # rows per thread of warp_fast_kernel

Geom = collections.namedtuple("Geom", "hdr H W in_stride out_stride rs lw lh")
Case = collections.namedtuple(
    "Case", "name hdr H W in_stride out_stride max_res members outs modes src_align out_align levels flow ts path")
Member = collections.namedtuple("Member", "n_out ts src_off out_off flow")
Launch = collections.namedtuple("Launch", "label first count staged planes split", defaults=(False,))

PATHS = ("batch", "period", "single", "single1", "copy")
# batch:   FlowBatch.interpolatePeriod with injected flows       period: FlowBatch.runPeriod through the real chain
# single:  one context, interpolateOnly (fused when it has two outputs or more)
# single1: one context, warpFrames (launch_warp_t)               copy: one context, copyFrame


def ilog2(v):
    return 0 if v <= 1 else 1 + ilog2(v >> 1)


def geometry(case):
    """hf_context.hip / hf_oracle.c hfo_make_geom."""
    rs = 0
    while (case.H >> rs) > case.max_res:
        rs += 1
    c = 1 << rs
    return Geom(int(case.hdr), case.H, case.W, case.in_stride or case.W, case.out_stride or case.W, rs, -(-case.W // c), -(-case.H // c))


def esize(g):
    return 2 if g.hdr else 1


def ename(g):
    return "u16" if g.hdr else "u8"


def members(case):
    """Member i: outs[i % ..] outputs with the scalar pool rotated by i, alignments and flow kind cycled."""
    out = []
    for i in range(case.members):
        n = case.outs[i % len(case.outs)]
        pool = case.ts[i % len(case.ts):] + case.ts[:i % len(case.ts)]
        out.append(Member(n, tuple(pool[:n]), case.src_align[i % len(case.src_align)], case.out_align[i % len(case.out_align)],
                          case.flow[i % len(case.flow)]))
    return out


# ------------------------------------------------------------------------------------------------
# (a) launch selection
# ------------------------------------------------------------------------------------------------
def phase_layout(g):
    """hf_flow.hip make_phase_layout with hf_context.hip's max_iters = log2(initial window): (mx, lwp)."""
    d = max(g.lw, g.lh)
    ws0 = d if d & (d - 1) == 0 else 1 << d.bit_length()
    reach = (ilog2(ws0) + 1) * 64 + 8
    mx = (((reach >> g.rs) + 2 + 3) // 4) * 4
    return mx, ((g.lw + 2 * mx + 4 + 31) // 32) * 32


def plane_emission_geometry(g):
    mx, lwp = phase_layout(g)
    e, lw = esize(g), g.W >> g.rs
    return (3 <= g.rs <= 4 and (lw << g.rs) == g.W and lw == g.lw and (lw & 3) == 0 and mx <= lw and (mx & 3) == 0 and (lwp & 3) == 0 and
            (g.in_stride * e) % 16 == 0 and (g.H * g.in_stride * e) % 16 == 0 and (g.H & 1) == 0)


def tile_counts(g, vec):
    """(wave tiles per tile row, wave tiles of a frame) of kernels with 2 rows per thread."""
    y_groups, uv_groups = (g.H + 1) // 2, ((g.H >> 1) + 1) // 2
    wpr = -(-g.W // (WARP_TX * vec))
    return wpr, wpr * (-(-y_groups // WARP_TY) + -(-uv_groups // WARP_TY))


def defers_planes(g, n_members):
    """warp_period_can_build_planes (hf_batch_create: single-stream members without HF_FLAG_BATCH_EAGER_PLANES / HF_FLAG_NO_FUSED_WARP)."""
    e = esize(g)
    vec, cell = 16 // e, 1 << g.rs
    if cell < vec or g.W * g.H * e <= SMALL_FRAME_BYTES:
        return False
    _, n_tiles = tile_counts(g, vec)
    per_launch = min(n_members, MAX_WARP_BATCH)
    return n_tiles * per_launch >= WG_MIN_WAVES and g.H == (g.lh << g.rs) and plane_emission_geometry(g)


def wg_blocks_per_member(g, plane_blocks):
    vec, nw = 16 // esize(g), WG_WAVES * 2 // WG_ROWS
    wpr = -(-g.W // (WARP_TX * vec))
    y_tiles = -(-(-(-g.H // WG_ROWS)) // WARP_TY)
    uv_tiles = -(-(-(-(g.H >> 1) // WG_ROWS)) // WARP_TY)
    yb, ub = -(-y_tiles // nw), -(-uv_tiles // nw)
    return (wpr * 3 + plane_blocks) * max(ub, (yb + 1) // 2)


def plane_blocks(g):
    nw = WG_WAVES * 2 // WG_ROWS
    return ((g.lw >> 2) * (2 * nw * WARP_TY * WG_ROWS) + 64 * nw - 1) // (64 * nw)


def warp_fast_shape(g, vb, mode, ms, levels):
    """(fast, dw, group) for the members ms of one launch."""
    e = esize(g)
    vec, cell = vb // e, 1 << g.rs
    group = min(cell, vec)
    fast = (0 <= mode <= 2 and g.in_stride % 2 == 0 and g.out_stride % vec == 0 and g.W >= 2 * vec and group >= 2 and
            vec % group == 0 and vec // group <= 4)
    dw = (g.in_stride * e) % 4 == 0 and (g.W * e) % 4 == 0 and (g.H * g.in_stride * e) % 4 == 0
    black, white = levels
    sane = white != black and white != 0.0 and white == white and black == black
    for m in ms:
        fast = fast and (mode != 2 or sane) and 1 <= m.n_out <= MAX_WARP_OUTPUTS
        fast = fast and all(0.0 <= t <= 1.0 for t in m.ts) and m.out_off % vb == 0
        dw = dw and m.src_off % 4 == 0
    return fast, dw, group


def warp_small_frame(g):
    return g.W * g.H * esize(g) <= SMALL_FRAME_BYTES


def launch_warp_fast(g, vb, mode, ms, levels, pending=None):
    """One launch of launch_warp_fast<E, VB>: None (not this shape) or (label, staged, members whose plane the launch builds).
    pending: per member, does it ask for its frame21's plane (a deferring batch's launch ahead of the chain)?  None: no plane layout passed."""
    fast, dw, group = warp_fast_shape(g, vb, mode, ms, levels)
    if not fast:
        return None
    e, n = esize(g), len(ms)
    vec = vb // e
    _, n_tiles = tile_counts(g, vec)
    max_out = max(m.n_out for m in ms)
    small_frame = g.W * g.H * e <= SMALL_FRAME_BYTES * 2
    out_chunk = 1 if small_frame and n_tiles * n < ROUNDS else MAX_WARP_OUTPUTS
    n_chunks = -(-max_out // out_chunk)
    if vb == 16 and group == vec and dw and out_chunk > 1 and max_out >= 2 and n_tiles * n >= WG_MIN_WAVES:
        nb_max = wg_blocks_per_member(g, plane_blocks(g))
        if (nb_max * n + 8) * nb_max < (1 << 32):                              # fastdiv_exact
            built = ()
            if pending is not None and plane_emission_geometry(g):
                built = tuple(i for i, m in enumerate(ms) if pending[i] and m.src_off % 16 == 0)
            return f"staged.{ename(g)}.rs{g.rs}" + (".planes" if built else ""), True, built
    large = WAVES_LARGE if vb == 16 and group * e == 16 else WAVES_SMALL       # warp_max_waves
    wpb = large if out_chunk > 1 and n_tiles * n_chunks * n >= ROUNDS else WAVES_SMALL
    return (f"fast.{ename(g)}.vb{vb}.g{group}.{'dw' if dw else 'nodw'}.{'all' if out_chunk > 1 else 'one'}.w{wpb}"), False, ()


def launch_warp_fast_any(g, mode, ms, levels, pending=None):
    if warp_small_frame(g):
        r = launch_warp_fast(g, 8, mode, ms, levels)
        if r:
            return r
    return launch_warp_fast(g, 16, mode, ms, levels, pending)


def launch_warp_t(g, mode, m, levels):
    """A single output of one context (launch_warp): the fast kernel with one output, or warp_kernel."""
    one = Member(1, m.ts[:1], m.src_off, m.out_off, m.flow)
    r = launch_warp_fast_any(g, mode, [one], levels)
    if r:
        return r[0]
    vec = 16 // esize(g)
    return f"generic.{ename(g)}.{'aligned' if g.out_stride % vec == 0 and m.out_off % 16 == 0 else 'unaligned'}"


def launch_copy_t(g, m):
    vec = 16 // esize(g)
    aligned = g.in_stride % vec == 0 and g.out_stride % vec == 0 and m.src_off % 16 == 0 and m.out_off % 16 == 0
    return f"copy.{ename(g)}.{'aligned' if aligned else 'unaligned'}"


def launch_warp_periods(g, mode, ms, levels, pending=None):
    """The launches of a set of periods, or None: a member's shape does not qualify and nothing is launched."""
    if not 1 <= len(ms) <= MAX_FLOW_BATCH:
        return None
    parts = [(f, ms[f:f + MAX_WARP_BATCH]) for f in range(0, len(ms), MAX_WARP_BATCH)]
    for _, part in parts:
        if any(not 1 <= m.n_out <= MAX_WARP_OUTPUTS for m in part):
            return None
        if not ((warp_small_frame(g) and warp_fast_shape(g, 8, mode, part, levels)[0]) or warp_fast_shape(g, 16, mode, part, levels)[0]):
            return None
    out = []
    for f, part in parts:
        label, staged, built = launch_warp_fast_any(g, mode, part, levels, None if pending is None else pending[f:f + MAX_WARP_BATCH])
        out.append(Launch(label, f, len(part), staged, tuple(f + i for i in built), len(parts) > 1))
    return out


def interpolate_member(g, mode, m, levels):
    """hf_interpolate_period_ex of one context: a fused launch for two outputs or more, else (or where that does not qualify) one per output."""
    if m.n_out >= 2:
        r = launch_warp_periods(g, mode, [m], levels)
        if r:
            return r
    return [Launch(launch_warp_t(g, mode, m, levels), 0, 1, False, ())]


def launches(case, mode, ahead_of_chain=None):
    """The warp (or copy) launches of one call of the case's path in `mode`.  ahead_of_chain: a deferring batch's runPeriod issues the warps
    before the chain and asks them for the planes (default: the case's path is "period" and its batch defers)."""
    g, ms = geometry(case), members(case)
    if case.path == "copy":
        return [Launch(launch_copy_t(g, ms[0]), 0, 1, False, ())]
    if case.path == "single1":
        return [Launch(launch_warp_t(g, mode, ms[0], case.levels), 0, 1, False, ())]
    if case.path == "single":
        return interpolate_member(g, mode, ms[0], case.levels)
    if ahead_of_chain is None:
        ahead_of_chain = case.path == "period" and defers_planes(g, len(ms)) and 0 <= mode <= 2
    r = launch_warp_periods(g, mode, ms, case.levels, [True] * len(ms) if ahead_of_chain else None)
    if r is not None:
        return r
    out = []
    for i, m in enumerate(ms):                    # hf_batch.hip batch_interpolate: member by member
        out += [ln._replace(first=i) for ln in interpolate_member(g, mode, m, case.levels)]
    return out


def labels(case, mode):
    """Every label of the case in one mode: launches, split, plane emission."""
    g = geometry(case)
    lns = launches(case, mode)
    out = {ln.label for ln in lns}
    if any(ln.split for ln in lns):
        out.add("split")
    for ln in lns:
        if ln.label.endswith(".planes"):
            out.add(f"plane.{ename(g)}.rs{3 if g.hdr and g.rs == 3 else 4}")
            if len(ln.planes) < ln.count:
                out.add("plane.fallback")
    return out


def instantiation(label, mode):
    """The compiled kernel behind a launch label, as `nm -C` prints its template arguments (None: no kernel of its own)."""
    p = label.split(".")
    e = {"u8": "unsigned char", "u16": "unsigned short"}.get(p[1] if len(p) > 1 else "")
    if p[0] == "fast":
        return f"warp_fast_kernel<{e}, {p[3][1:]}, 2, {mode}, {p[2][2:]}, {'true' if p[4] == 'dw' else 'false'}>"
    if p[0] == "staged":
        return f"warp_wg_kernel<{e}, {mode}, {WG_WAVES * 2 // WG_ROWS}, {WG_ROWS}>"
    if p[0] in ("generic", "copy"):
        return f"{'warp' if p[0] == 'generic' else 'copy'}_kernel<{e}, {16 // (2 if p[1] == 'u16' else 1)}, {'true' if p[2] == 'aligned' else 'false'}>"
    return None


def _fast_labels():
    out = set()
    for e, name in ((1, "u8"), (2, "u16")):
        for vb in (8, 16):
            vec = vb // e
            for group in (vec, vec // 2, vec // 4):
                if group < 2:                 # warp_fast_shape: a chroma run is made of element pairs
                    continue
                for dw in ("dw", "nodw"):
                    waves = (4, 16) if vb == 16 and group * e == 16 else (4,)
                    out |= {f"fast.{name}.vb{vb}.g{group}.{dw}.one.w4"} | {f"fast.{name}.vb{vb}.g{group}.{dw}.all.w{w}" for w in waves}
    return out


# what a launch in modes 0 .. 2 can be (every entry is reached by the sweep of tests/test_warp_variant_model.py, nothing else is)
FAST_LABELS = frozenset(_fast_labels())
STAGED_LABELS = frozenset([f"staged.u16.rs{r}" for r in (3, 4, 5, 6)] + [f"staged.u8.rs{r}" for r in (4, 5, 6)] +
                          ["staged.u16.rs3.planes", "staged.u16.rs4.planes", "staged.u8.rs4.planes"])
GENERIC_LABELS = frozenset(f"generic.{e}.{a}" for e in ("u8", "u16") for a in ("aligned", "unaligned"))
COPY_LABELS = frozenset(f"copy.{e}.{a}" for e in ("u8", "u16") for a in ("aligned", "unaligned"))
EXTRA_LABELS = frozenset(["split", "plane.u16.rs3", "plane.u16.rs4", "plane.u8.rs4", "plane.fallback"])
MODE_LABELS = FAST_LABELS | STAGED_LABELS | GENERIC_LABELS | EXTRA_LABELS       # required in each of modes 0, 1, 2
# compiled, never launched: 8-byte threads of 16-bit frames hold 4 elements, GROUP 1 would be a resolution scalar of 0, and group >= 2 is required
UNREACHABLE = {f"warp_fast_kernel<unsigned short, 1, 2, {m}, 8, {d}>": "VB 8 with 16-bit elements and rs 0: group == 1, warp_fast_shape needs group >= 2"
               for m in (0, 1, 2) for d in ("true", "false")}


# ------------------------------------------------------------------------------------------------
# (b) the workgroups of warp_wg_kernel
# ------------------------------------------------------------------------------------------------
CLASSES = ("staged.interior", "staged.edge.left", "staged.edge.right", "staged.edge.top", "staged.edge.bottom", "global",
           "generic.partial", "generic.beyond_extension", "generic.chroma_right_zone", "generic.edge_no_fit")


def required_pairs():
    """(element type, plane, class): chroma never stages a window in the right mirror zone, luma has no chroma zone."""
    return {(e, p, c) for e in ("u8", "u16") for p in ("y", "uv") for c in CLASSES
            if not (p == "uv" and c == "staged.edge.right") and not (p == "y" and c == "generic.chroma_right_zone")}


def _roundf(v):
    """roundf of float32 values: halves away from zero."""
    v = np.asarray(v, np.float32).astype(np.float64)
    return np.where(v >= 0, np.floor(v + 0.5), np.ceil(v - 0.5)).astype(np.int64)


def wg_plane(g, cz, flow, ts, mode):
    """warp_wg_body's decision for every workgroup of one plane of one member.
    Returns (classes [block rows][tile columns] of frozensets, (staged, interior_global, generic), deepest staged reach into a mirror zone)."""
    e = esize(g)
    vec, rows, nw = 16 // e, WG_ROWS, WG_WAVES * 2 // WG_ROWS
    tw, th, chunks = WARP_TX * vec, nw * WARP_TY * rows, (nw * rows // 2) * WG_CHUNKS_PER_WAVE
    H, W, rs, lw, lh = g.H, g.W, g.rs, g.lw, g.lh
    dim_y = H >> 1 if cz else H
    groups = -(-dim_y // rows)
    tiles = -(-groups // WARP_TY)
    nb, wpr = -(-tiles // nw), -(-W // tw)
    need = {0: (True, False), 1: (False, True), 2: (True, True)}[mode]
    # waves: absent (no tile), full, or partial (a lane past the row's end or the plane's last row group)
    trow = np.arange(nb)[:, None] * nw + np.arange(nw)[None, :]
    present = trow < tiles
    full_rows = present & (trow * WARP_TY + WARP_TY - 1 < groups)
    full_cols = (np.arange(wpr) + 1) * tw <= W
    partial = (present[:, :, None] & ~(full_rows[:, :, None] & full_cols[None, None, :])).any(axis=1)          # [nb][wpr]
    # phase A per flow cell
    lcw = rs + cz
    lgx, lgy = max(0, ilog2(tw) - lcw), max(0, ilog2(th) - rs)
    it_ok0 = lgx + lgy <= ilog2(WG_CELLS)
    cw, ch = min(1 << lcw, tw), min(1 << rs, th)
    x0, y0 = np.arange(wpr << lgx) * cw, np.arange(nb << lgy) * ch
    inplane = (y0 < dim_y)[:, None] & (x0 < W)[None, :]
    ly = np.minimum(((y0 >> rs) << 1) if cz else (y0 >> rs), lh - 1)
    lx = np.minimum(((x0 >> rs) & ~1) if cz else (x0 >> rs), lw - 1)
    fx, fy = flow[0].astype(np.int64), flow[1].astype(np.int64)
    ox12, oy12 = fx[np.ix_(ly, lx)], fy[np.ix_(ly, lx)]
    py = np.clip(ly[:, None] - (oy12 >> rs), 0, lh - 1)
    px = np.clip(lx[None, :] - (ox12 >> rs), 0, lw - 1)
    ox21, oy21 = fx[py, px], fy[py, px]
    X0, Y0 = x0[None, :], y0[:, None]
    big = 1 << 30
    ok_all, bounds_all, in_all = (np.ones(inplane.shape, bool) for _ in range(3))
    edge = {k: np.zeros(inplane.shape, bool) for k in ("left", "right", "top", "bottom")}
    depth = np.zeros(inplane.shape, np.int64)
    win = [dict(bx_lo=np.full(inplane.shape, big), by_lo=np.full(inplane.shape, big), bx_hi=np.zeros(inplane.shape, np.int64),
                by_hi=np.zeros(inplane.shape, np.int64)) for _ in (0, 1)]
    half = np.float32(0.5)
    for t in ts:
        s12 = np.float32(t)
        s21 = np.float32(1.0) - s12
        for src in (0, 1):
            if not need[src]:
                continue
            ox, oy, s, sign = ((ox12, oy12, s12, 1), (ox21, oy21, s21, -1))[src]
            dx = sign * _roundf(ox.astype(np.float32) * s)
            dy = sign * _roundf(oy.astype(np.float32) * s * half if cz else oy.astype(np.float32) * s)
            dxe = (dx & ~1) if cz else dx
            x_lo = X0 + dxe
            x_hi = x_lo + cw - vec
            y_lo = Y0 + dy
            y_hi = y_lo + ch - rows
            bx_lo, bx_hi, by_lo, by_hi = (x_lo + EXT_X) * e, (x_hi + EXT_X) * e, y_lo + EXT_Y, y_hi + EXT_Y
            bounds = (bx_lo >= 0) & (bx_hi + 4 * NDW + 4 <= 0xFFFF) & (by_lo >= 0) & (by_hi + rows <= 0xFFFF)
            ok = bounds & (x_hi + vec <= W - 2) if cz else bounds
            ok_all &= ok | ~inplane
            bounds_all &= bounds | ~inplane
            left, right, top, bottom = x_lo < 1, x_hi + vec - 1 + cz > W - 2, y_lo < 1, y_hi + rows - 1 > dim_y - 2
            in_all &= ~(left | right | top | bottom) | ~inplane
            for k, v in (("left", left), ("right", right), ("top", top), ("bottom", bottom)):
                edge[k] |= v & inplane
            depth = np.maximum(depth, np.where(inplane, np.maximum.reduce([-x_lo, x_hi + vec - W, -y_lo, y_hi + rows - dim_y]), 0))
            use = ok & inplane                       # "only if ok": a run that is not stageable leaves the extremes alone
            w = win[src]
            w["bx_lo"] = np.where(use, np.minimum(w["bx_lo"], bx_lo), w["bx_lo"])
            w["by_lo"] = np.where(use, np.minimum(w["by_lo"], by_lo), w["by_lo"])
            w["bx_hi"] = np.where(use, np.maximum(w["bx_hi"], bx_hi), w["bx_hi"])
            w["by_hi"] = np.where(use, np.maximum(w["by_hi"], by_hi), w["by_hi"])

    def tile(a, red):
        return red(red(a.reshape(nb, 1 << lgy, wpr, 1 << lgx), axis=3), axis=1)

    ok_t, bounds_t, in_t = tile(ok_all, np.all) & it_ok0, tile(bounds_all, np.all) & it_ok0, tile(in_all, np.all)
    runs_ok = ok_t & ~partial
    fit = np.ones((nb, wpr), bool)
    for src in (0, 1):
        if not need[src]:
            continue                                 # (C = 1, R = 0: an unused source costs nothing)
        w = win[src]
        cmin, ymin = tile(w["bx_lo"], np.min) >> 4, tile(w["by_lo"], np.min)
        hx, hy = tile(w["bx_hi"], np.max), tile(w["by_hi"], np.max)
        C = (((hx & 0xFFFC) + 4 * NDW + 3) >> 4) - cmin + 1
        R = hy + rows - 1 - ymin + 1
        fit &= (((R * C + 63) & ~63) <= chunks) & (C <= 64)
    staged = runs_ok & fit
    glob = runs_ok & ~fit & in_t
    edges = {k: tile(v, np.any) for k, v in edge.items()}
    depth_t = tile(depth, np.max)
    classes = []
    for b in range(nb):
        row = []
        for c in range(wpr):
            if staged[b, c]:
                row.append(frozenset(["staged.interior"]) if in_t[b, c] else frozenset(f"staged.edge.{k}" for k in edges if edges[k][b, c]))
            elif glob[b, c]:
                row.append(frozenset(["global"]))
            elif partial[b, c]:
                row.append(frozenset(["generic.partial"]))
            elif not bounds_t[b, c]:
                row.append(frozenset(["generic.beyond_extension"]))
            elif not ok_t[b, c]:
                row.append(frozenset(["generic.chroma_right_zone"]))
            else:
                row.append(frozenset(["generic.edge_no_fit"]))
        classes.append(row)
    n_staged, n_glob = int(staged.sum()), int(glob.sum())
    deepest = int(depth_t[staged & ~in_t].max()) if (staged & ~in_t).any() else 0
    return classes, (n_staged, n_glob, nb * wpr - n_staged - n_glob), deepest


def wg_member(g, flow, ts, mode):
    """Both planes of one member: ({"y": classes, "uv": classes}, counts, deepest)."""
    y, cy, dy = wg_plane(g, 0, flow, ts, mode)
    uv, cu, du = wg_plane(g, 1, flow, ts, mode)
    return {"y": y, "uv": uv}, tuple(a + b for a, b in zip(cy, cu)), max(dy, du)


# ------------------------------------------------------------------------------------------------
# injected flow fields
# ------------------------------------------------------------------------------------------------
def flow_field(kind, g, seed=7):
    """uniform:<x>:<y> | half (left half (4, 2), right half (-300, 200)) | diverge | noise:<amplitude> | ramp (the vertical flow grows to the right)"""
    lw, lh = g.lw, g.lh
    f = np.zeros((2, lh, lw), np.int16)
    p = kind.split(":")
    if p[0] == "uniform":
        f[0], f[1] = int(p[1]), int(p[2])
    elif p[0] == "half":
        f[0, :, : lw // 2], f[1, :, : lw // 2] = 4, 2
        f[0, :, lw // 2:], f[1, :, lw // 2:] = -300, 200
    elif p[0] == "diverge":
        f[0] = np.linspace(-200, 200, lw).astype(np.int16)[None, :]
        f[1] = np.linspace(-90, 90, lh).astype(np.int16)[:, None]
    elif p[0] == "noise":
        a = int(p[1])
        f[:] = np.random.default_rng(seed).integers(-a, a + 1, size=f.shape)
    elif p[0] == "ramp":
        f[0] = 5
        f[1] = np.linspace(0, 160, lw).astype(np.int16)[None, :]
    else:
        raise ValueError(kind)
    return f


def case_counts(case, mode, flows=None):
    """(staged, interior_global, generic) of all staged launches of the case in `mode`, all their members together, plus the classes seen:
    (counts, {(element type, plane, class)}, deepest staged reach into a mirror zone).  flows: {kind: field} instead of the injected ones."""
    g, ms = geometry(case), members(case)
    tot, seen, deepest, cache = [0, 0, 0], set(), 0, {}
    for ln in launches(case, mode):
        if not ln.staged:
            continue
        for m in ms[ln.first:ln.first + ln.count]:
            k = (m.flow, m.ts)
            if k not in cache:
                cache[k] = wg_member(g, flows[m.flow] if flows else flow_field(m.flow, g), m.ts, mode)
            cl, cnt, d = cache[k]
            tot = [a + b for a, b in zip(tot, cnt)]
            deepest = max(deepest, d)
            for p in ("y", "uv"):
                seen |= {(ename(g), p, c) for row in cl[p] for cs in row for c in cs}
    return tuple(tot), seen, deepest


# ------------------------------------------------------------------------------------------------
# (c) the matrix (tests/test_warp_variants_gpu.py)
# ------------------------------------------------------------------------------------------------
T6 = (0.0, 0.1988, 0.5, 0.7992, 1.0, 0.3996)        # the blend scalars 0 and 1 exactly
T3 = (0.0, 0.7992, 1.0)
DEEP = (0.95, 1.0)                                  # with uniform:60:40 every edge window reaches 57 .. 60 elements into the mirror zone


def _c(name, hdr, H, W, max_res, n=1, outs=(3,), modes=(0, 1, 2), path="batch", si=0, so=0, src=(0,), out=(0,), levels=(0.0, 255.0),
       flow=("uniform:9:-5",), ts=T3):
    return Case(name, hdr, H, W, si, so, max_res, n, tuple(outs), tuple(modes), tuple(src), tuple(out), levels, tuple(flow), tuple(ts), path)


def _matrix():
    cs = []
    e = {0: "u8", 1: "u16"}
    far = ("uniform:230:-140", "half", "diverge", "noise:40")
    # --- one output per thread, 4-wave workgroups: single contexts and tiny batches.  180 x 320: 8-byte threads (both element types); 768 x 1408 HDR
    #     and 1088 x 2048 SDR: above warp_small_frame, 16-byte threads.  rs 1 / 2 / 3 / 4 from max_res; src 2: sources that are not dword aligned.
    k = 0
    for hdr, H, W, res in ((0, 180, 320, (135, 67, 30)), (1, 180, 320, (135, 67)), (1, 768, 1408, (500, 250, 120)), (0, 1088, 2048, (300, 200, 100))):
        for mr in res:
            for src in (0, 2):
                path, n, outs = (("single", 1, (3,)), ("single1", 1, (1,)), ("batch", 2, (1, 2)))[k % 3]
                cs.append(_c(f"one-{e[hdr]}-{H}-res{mr}-src{src}-{path}", hdr, H, W, mr, n, outs, path=path, src=(src,), flow=("noise:12",),
                             levels=(16.0, 235.0) if k % 4 == 3 else (0.0, 255.0)))
                k += 1
    # --- all outputs per thread, 4-wave workgroups.  Small frames only inside a batch with 4 x 8192 wave tiles: 1080p SDR x 11, 720p HDR x 13
    for mr in (540, 270, 135):
        for src in (0, 2):
            cs.append(_c(f"all-u8-1080-res{mr}-src{src}-n11", 0, 1080, 1920, mr, 11, (1, 2, 3), src=(src,), flow=("noise:12", "uniform:-31:17")))
    for mr in (360, 180):
        for src in (0, 2):
            cs.append(_c(f"all-u16-720-res{mr}-src{src}-n13", 1, 720, 1280, mr, 13, (3, 1, 2), src=(src,), flow=("uniform:-31:17", "noise:12")))
    # ... frames above twice the small-frame bound: every launch, here one context with its outputs fused (1 to 6 of them)
    for hdr, H, W, res in ((1, 1088, 2048, (544, 272, 136)), (0, 1536, 2816, (384, 192, 96))):
        for i, mr in enumerate(res):
            for src in (0, 2):
                cs.append(_c(f"all-{e[hdr]}-{H}-res{mr}-src{src}-single", hdr, H, W, mr, 1, (6, 2, 4)[i:i + 1], path="single", src=(src,),
                             flow=("diverge",), ts=T6))
    # --- 16-wave workgroups: one flow cell per 16-byte thread in a launch of 4 x 8192 tiles that cannot be staged (one output each, or sources
    #     that are not dword aligned)
    cs.append(_c("w16-u16-1088-dw-n14", 1, 1088, 1536, 136, 14, (1,), flow=far))
    cs.append(_c("w16-u16-1088-nodw-n14", 1, 1088, 1536, 136, 14, (1, 2, 3), src=(2,), flow=far))
    cs.append(_c("w16-u8-1088-dw-n15", 0, 1088, 2816, 68, 15, (1,), flow=far))
    cs.append(_c("w16-u8-1088-nodw-n15", 0, 1088, 2816, 68, 15, (3, 2, 1), src=(2,), flow=far))
    # --- the staged kernel: rs 3 .. 6 (cells smaller than, equal to and taller than the 32-row tile), flows for every workgroup class
    for hdr, W, n, res in ((1, 1536, 14, (136, 68, 34, 17)), (0, 2816, 15, (68, 34, 17))):
        for i, mr in enumerate(res):
            cs.append(_c(f"staged-{e[hdr]}-res{mr}-n{n}", hdr, 1088, W, mr, n, (2, 3, 1, 6, 4, 5), flow=("uniform:9:-5",) + far, ts=T6))
        cs.append(_c(f"staged-{e[hdr]}-res{res[0]}-deep-n{n}", hdr, 1088, W, res[0], n, (2,), flow=("uniform:60:40", "uniform:-60:-40", "uniform:60:-40"), ts=DEEP))
        cs.append(_c(f"staged-{e[hdr]}-res{res[1]}-deep-n{n}", hdr, 1088, W, res[1], n, (2,), flow=("uniform:-60:40", "uniform:60:40"), ts=DEEP))
    # ragged: the last tile column and the last row groups are partial waves; strided, levels 16 / 235
    cs.append(_c("staged-u16-1084x1608-ragged-n14", 1, 1084, 1608, 136, 14, (2, 3), so=1664, si=1616, levels=(16.0, 235.0), flow=("uniform:9:-5", "ramp")))
    cs.append(_c("staged-u8-1084x2832-ragged-n15", 0, 1084, 2832, 68, 15, (2, 3), so=2848, flow=("uniform:9:-5", "ramp")))
    # --- through the real chain (runPeriod): the deferring batches (their launches build the planes; one member's frames sit at base + 4 bytes and
    #     keep their planes for the plane kernel), a batch of the fast kernel, a batch in a diagnostic mode (member by member, generic kernel)
    cs.append(_c("period-u16-res136-n14", 1, 1088, 1536, 136, 14, (2, 3, 1), path="period", src=(0, 0, 0, 4, 0)))
    cs.append(_c("period-u16-res68-n14", 1, 1088, 1536, 68, 14, (2, 3, 1), path="period", src=(0, 0, 4)))
    cs.append(_c("period-u8-res68-n15", 0, 1088, 2816, 68, 15, (3, 2), path="period", src=(0, 4, 0, 0)))
    cs.append(_c("period-u8-360-n3", 0, 360, 640, 270, 3, (2, 3, 1), path="period"))
    cs.append(_c("period-u16-360-n3-diagnostic", 1, 360, 640, 270, 3, (1, 2), modes=(3, 4, 5, 6), path="period"))
    # --- more than kMaxWarpBatch members: two launches
    cs.append(_c("split-u8-180-n18", 0, 180, 320, 67, 18, (1, 2, 3), flow=("noise:12",)))
    cs.append(_c("split-u16-1088-n30", 1, 1088, 1536, 136, 30, (2, 1), flow=("uniform:9:-5", "half")))
    # --- the generic kernel (rs 0: a flow cell of one element; outputs that are not 16-byte aligned) in all seven modes, and the copy kernel
    for hdr in (0, 1):
        cs.append(_c(f"generic-{e[hdr]}-rs0", hdr, 180, 320, 270, 1, (1,), modes=range(7), path="single1", flow=("noise:12",)))
        cs.append(_c(f"generic-{e[hdr]}-out2", hdr, 182, 328, 67, 1, (1,), modes=range(7), path="single1", out=(2,), flow=("noise:12",), levels=(16.0, 235.0)))
        cs.append(_c(f"copy-{e[hdr]}", hdr, 180, 320, 270, 1, (1,), modes=(2,), path="copy"))
        cs.append(_c(f"copy-{e[hdr]}-src{2}", hdr, 182, 328, 270, 1, (1,), modes=(2,), path="copy", src=(2,), levels=(16.0, 235.0)))
    return cs


CASES = _matrix()


def case(name):
    return next(c for c in CASES if c.name == name)
