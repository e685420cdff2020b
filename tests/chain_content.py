"""Frames for the chain's GPU tests (test_sad_reuse_gpu.py, test_chain_variants_gpu.py, test_chain_saturation_gpu.py,
test_chain_deep_rs_gpu.py, test_chain_ties_gpu.py): the bench's content classes, noise patches inside a static frame, full-range noise, the
drift kinds (DRIFT_KINDS:
one noise field seen through a frame that moves by an odd number of pixels a frame, so that windows at a frame edge settle on offsets that
point out of the frame at a phase that is neither 0 nor even: drift_frames), the tie kinds (TIE_KINDS: flat frames whose marks make two
candidates of a window cost exactly the same: tie_sites), and the saturation kinds (SAT_KINDS) -- pairs whose SADs sit
at the top of their range, 765 per pixel, the value every width argument of hf_flow.hip is about:
  "saturated"   dark, bright, dark, bright, ..: every candidate of every window has the largest SAD there is (zero flow, every window reuses)
  "sat-y"       the same with only the luma plane alternating, the chroma plane mid-grey;   "sat-uv": only the chroma plane, luma mid-grey
  "specks"      a dark frame with bright cells and a bright frame alternate, fresh cells every time.  A cell is 2 x 2 luma pixels (one chroma
                sample) at every resolution scalar -- wider cells make neighbouring candidates see the same samples -- set independently
                per plane with a probability that depends on where it lies: 0 in a top-left corner of 32 x 32 grid samples (windows there
                reach the maximum), small in the rest of a strip on the left (sums near the maximum), a third right of it (the sums of
                windows of 32, 16 and 8 lie around a multiple of 2^16 or 2^15, so the winner depends on their high bits:
                tests/test_chain_saturation_model.py; SPECK_DEFAULT / SPECK_TUNED have the figures).
                Frames of at most SPECK_LATTICE_MAX luma pixels on their shorter side are no wider than the candidates reach (+-64), so
                any drift of a window samples beyond the single reflection, where the reference is undefined.  There the dark frame
                carries a LATTICE instead: luma bright exactly at the grid samples (every 2^rs-th pixel of every 2^rs-th row, rs >= 1),
                chroma dark.  Every window's true winner is d = 0 (zero flow, no sample beyond the reflection, every window reuses)
                with a SAD of 510 per pixel -- just below 8 x 2^16, 2 x 2^16 and 2^15 at windows of 32, 16 and 8 -- while every odd
                offset misses the lattice and scores the full 765: a sum that wraps, or is read as signed, elects one of those.
Codes: SDR 255 / 0; P010 bright 0xFFFF and 0xFF00 in turn from one bright frame to the next, dark 0x00FF -- top byte 0 under a low byte of all
ones, so a plane build that rounds instead of truncating, or lets low bits leak, shows as a difference that is not there."""
import numpy as np

SAT_KINDS = ("specks", "saturated", "sat-y", "sat-uv")
# "drift": one field of full-range noise seen through a frame that moves by DRIFT_STEP luma pixels per frame, one kind per direction
DRIFT_KINDS = ("drift-se", "drift-sw", "drift-ne", "drift-nw")
DRIFT_STEP = (75, 67)     # (|dx|, |dy|): odd, so no multiple of 2^rs at any rs >= 1, and beyond 2^6: an aligned grid's last column and row lie 2^rs short of the edge
DRIFT_CELLS = (256, 64, 16, 4)
# "tie": flat frames with luma marks that are mirror images about a window's centre, so that candidates -d and +d of that window cost
# exactly the same and beat d = 0 (tie_sites); one kind per (delta, nb) the marks' amplitudes are worked out for
TIE_KINDS = ("tie-d0", "tie-d3", "tie-d8")
TIE_SETTINGS = {"tie-d0": (0, 0), "tie-d3": (3, 2), "tie-d8": (8, 6)}
TIE_BASE = 16             # the flat luma level (top 8 bits); a mark is TIE_BASE + a
TIE_SITES = 4             # sites wanted per (window, axis): half of them in the odd frames, half in the even ones
TIE_TRIES = 400           # windows tried per site
KIND_ORDER = ("patches", "chaotic", "noise", "static", "bench", "cut", "pan64") + SAT_KINDS + DRIFT_KINDS + TIE_KINDS
SPECK_CLEAN = 32          # the clean corner, in grid samples per axis (at most half the grid)
SPECK_CELL = 2            # luma pixels per fine cell and axis
SPECK_COARSE_CELL = 4     # fine cells per coarse cell and axis
# (probability of a fine cell in the sparse strip, .. in the dense zone, probability of a coarse cell in the dense zone, the strip's share of
# the width).  Tuned on the CPU oracle against the floors of tests/test_chain_saturation_model.py.  A third of the samples bright puts the
# sums of the dense zone on the multiples of 2^16 / 2^15.  On two frame shapes the offset bias at delta 0 ties the candidates down too far
# for that (1388 wide: the chain carries the neighbour term before level 32); there part of the third comes as coarse cells, which spread
# the candidates' sums.
SPECK_DEFAULT = (0.02, 0.33, 0.0, 1 / 8)
SPECK_TUNED = {(568, 1388): (0.02, 0.12, 0.24, 1 / 16), (540, 960): (0.02, 0.12, 0.24, 1 / 16)}      # by (H, W) of the frame
SPECK_LATTICE_MAX = 128   # frames up to this many luma pixels on the shorter side carry the lattice


def kind_seed(kind):
    """The seed the matrices of test_chain_variants_gpu.py and test_chain_saturation_gpu.py (and the CPU proof of the latter's content) use."""
    return 9000 + 13 * KIND_ORDER.index(kind)


def patched(frame_a, H, S, hdr, seed, n=40):
    """frame_a with n rectangular patches (8 .. 96 px) of fresh noise: the rest of the frame is static."""
    rng = np.random.default_rng(seed)
    f = frame_a.copy()
    y = f[:H * S].reshape(H, S)
    uv = f[H * S:].reshape(H // 2, S)
    hi = 65536 if hdr else 256
    for _ in range(n):
        ph, pw = int(rng.integers(4, min(49, H // 4))) * 2, int(rng.integers(4, min(49, S // 4))) * 2
        y0, x0 = int(rng.integers(0, (H - ph) // 2)) * 2, int(rng.integers(0, (S - pw) // 2)) * 2
        y[y0:y0 + ph, x0:x0 + pw] = rng.integers(0, hi, size=(ph, pw))
        uv[y0 // 2:(y0 + ph) // 2, x0:x0 + pw] = rng.integers(0, hi, size=(ph // 2, pw))
    return f


def sat_codes(hdr, i):
    """(bright, dark, mid-grey) of frame i."""
    if not hdr:
        return 255, 0, 128
    return (0xFF00 if (i // 2) & 1 else 0xFFFF), 0x00FF, 0x8000


def _speck_mask(rng, H, W, rs):
    """[3][ceil(H / c)][ceil(W / c)] booleans, c = SPECK_CELL: the cells of Y, U and V that take the other code -- fine cells with the
    probability of their zone, and in the dense zone coarse cells of SPECK_COARSE_CELL x SPECK_COARSE_CELL fine ones on top."""
    c, cc = SPECK_CELL, SPECK_COARSE_CELL
    p_sparse, p_dense, p_coarse, share = SPECK_TUNED.get((H, W), SPECK_DEFAULT)
    ny, nx = -(-H // c), -(-W // c)
    p = np.full((ny, nx), p_dense)
    sparse = int(round(nx * share))
    p[:, :sparse] = p_sparse
    k = (SPECK_CLEAN << rs) // c
    ky, kx = min(k, ny // 2), min(k, nx // 2)
    p[:ky, :kx] = 0.0
    fine = rng.random((3, ny, nx)) < p
    coarse = rng.random((3, -(-ny // cc), -(-nx // cc))) < p_coarse
    coarse = np.repeat(np.repeat(coarse, cc, axis=1), cc, axis=2)[:, :ny, :nx]
    coarse[:, :, :sparse] = False
    coarse[:, :ky, :kx] = False
    return fine | coarse


def saturation_frame(kind, H, W, hdr, seed, i, in_stride=0, rs=0):
    """Frame i of a saturation kind (module docstring)."""
    assert kind in SAT_KINDS, kind
    S = in_stride if in_stride > 0 else W
    bright, dark, grey = sat_codes(hdr, i)
    base = bright if i & 1 else dark
    f = np.zeros((H + H // 2, S), dtype=np.uint16 if hdr else np.uint8)
    f[:H, :W] = grey if kind == "sat-uv" else base
    f[H:, :W] = grey if kind == "sat-y" else base
    if kind == "specks" and not i & 1:
        if min(H, W) <= SPECK_LATTICE_MAX:
            assert rs >= 1, "the lattice needs pixels between the grid samples"
            f[:H:1 << rs, :W:1 << rs] = bright
            return f.reshape(-1)
        c = SPECK_CELL
        m = _speck_mask(np.random.default_rng([seed, i]), H, W, rs)
        up = lambda a, k, h, w: np.repeat(np.repeat(a, k, axis=0), k, axis=1)[:h, :w]
        f[:H, :W][up(m[0], c, H, W)] = bright
        f[H:, 0:W:2][up(m[1], c // 2, H // 2, (W + 1) // 2)] = bright
        f[H:, 1:W:2][up(m[2], c // 2, H // 2, W // 2)] = bright
    return f.reshape(-1)


def _drift_field(rng, h, w, hdr):
    """[h][w] codes over the whole range of the element type: cells of DRIFT_CELLS pixels, each scale with its own random level, summed --
    the difference between the field and its shifted copy grows with the shift up to the largest cell, so the chain's coarse steps find the
    direction and its fine steps the pixel -- and stretched so that the smallest sum is code 0 and the largest the top code."""
    f = np.zeros((h, w), dtype=np.float32)
    for c in DRIFT_CELLS:
        f += np.repeat(np.repeat(rng.random((-(-h // c), -(-w // c)), dtype=np.float32), c, axis=0), c, axis=1)[:h, :w]
    f -= f.min()
    hi = 65535 if hdr else 255
    return np.minimum(f * ((hi + 1) / f.max()), hi).astype(np.uint16 if hdr else np.uint8)


def drift_frames(kind, H, W, hdr, seed, count=3, in_stride=0):
    """Frame k of a drift kind: the window [k dy, k dy + H) x [k dx, k dx + W) of one field (luma; U and V are fields of their own at half
    the resolution, moved by the whole chroma samples inside k dx and k dy), (dx, dy) = +-DRIFT_STEP by the kind's direction.  Windows at a
    frame edge the content drifts across settle on offsets that point out of the frame, by an odd number of pixels.  P010: all 16 bits of
    a code vary (the stretch leaves the low bits as they fall)."""
    assert kind in DRIFT_KINDS, kind
    S = in_stride if in_stride > 0 else W
    dx = DRIFT_STEP[0] * (1 if kind[-1] == "e" else -1)
    dy = DRIFT_STEP[1] * (1 if kind[-2] == "s" else -1)
    px, py = (DRIFT_STEP[0] * (count - 1) + 1) & ~1, (DRIFT_STEP[1] * (count - 1) + 1) & ~1
    rng = np.random.default_rng(seed)
    Y = _drift_field(rng, H + 2 * py, W + 2 * px, hdr)
    U, V = (_drift_field(rng, H // 2 + py, (W + 1) // 2 + px, hdr) for _ in range(2))
    out = []
    for k in range(count):
        y0, x0 = py + k * dy, px + k * dx
        f = np.zeros((H + H // 2, S), dtype=Y.dtype)
        f[:H, :W] = Y[y0:y0 + H, x0:x0 + W]
        cy, cx = y0 >> 1, x0 >> 1
        f[H:, 0:W:2] = U[cy:cy + H // 2, cx:cx + (W + 1) // 2]
        f[H:, 1:W:2] = V[cy:cy + H // 2, cx:cx + W // 2]
        out.append(f.reshape(-1))
    return out


def _first_window(lw, lh):
    """The chain's first window (opticalFlowCalcSDR.cpp:49-59): half the power of two at or above the longer side of the grid."""
    m = max(lw, lh)
    return (1 << (m - 1).bit_length()) // 2


def _tie_amplitude(ws, d, cols, thin, delta, bias, parent_pixels, parent_bias):
    """(bar length in samples, amplitude) of a site whose window leaves d = 0 while its parent keeps it, or None.
    One bar's SAD is E = cols x length x amplitude << delta.  At -d and +d the window's samples miss one bar and pay d x ws^2 x bias more
    than at 0: the window leaves 0 when E > d ws^2 bias, the parent (which loses the bar at its own border) stays while
    E < d x its pixels x its bias.  A thin bar at rs >= 1 lies on one sample column and candidates +-1 miss BOTH bars, here and in every
    ancestor: 2 E > ws^2 bias and 2 E < the parent's.  The target is 1.25 x the lower bound, under 0.8 x the upper."""
    lower = ws * ws * bias * (0.5 if thin else d)
    upper = None if parent_pixels is None else parent_pixels * parent_bias * (0.5 if thin else d)
    lengths = [n for n in (ws // 2, ws, ws // 4, ws // 8, ws // 16, 1) if n >= 1]
    for n in dict.fromkeys(lengths):
        unit = (cols * n) << delta
        a = int(1.25 * lower / unit) + 1
        if a <= 200 and (upper is None or a * unit < 0.8 * upper):
            return n, a
    return None


def tie_sites(kind, H, W, rs, seed):
    """The sites of a tie kind at one geometry: dicts (set: 0 = even frames, 1 = odd frames; ws, axis, d, wx, wy in grid samples; n, a: bar
    length in samples and amplitude; thin).  A site is one full window of level ws with two bars of luma marks, d pixels thick, at its first
    and its last sample along the searched axis -- mirror images about the window's centre, so with the window's offset still 0 the candidates
    -d and +d see the same samples mirrored and cost exactly the same, less than d = 0, which sees both bars.  At rs >= 1 half the sites
    are thin: one pixel on the sample line, which +-1 misses; at rs 0 the thickness goes through 1, 4 and 9.  Bars run across the searched axis over the middle half of the window where the
    amplitude allows, over pixels between the sample lines too, so the other axis' candidates see the same marks; the Y sites of windows 4 and 2 run
    on through both neighbours, or the window's own X step would leave them.  Sites keep clear of each other by the candidates' reach (and by
    two windows where the neighbour term counts, the chain's fifth level on: a neighbour that moved would bias -d and +d differently), of the frame's edge
    along the searched axis (the reflection is no mirror image), and lie inside their grandparent where the grid has room."""
    s = 1 << rs
    lw, lh = -(-W // s), -(-H // s)
    ws0 = _first_window(lw, lh)
    rng = np.random.default_rng(seed)
    placed = []
    for k in range(ws0.bit_length() - 1):
        ws = ws0 >> k
        if ws > 256:          # (the 1388-wide grid starts at 1024: no frame of the suite has two such windows, and their marks would leave no room)
            continue
        tile_w, tile_h = (64, 16) if ws > 32 else (32, 32)
        cand = [(ix, iy) for iy in range((lh // tile_h) * tile_h // ws) for ix in range((lw // tile_w) * tile_w // ws)]       # windows inside full tiles
        order = rng.permutation(len(cand))
        inner = lambda i: (i & 3) in (1, 2)
        cand = sorted((cand[i] for i in order), key=lambda c: not (inner(c[0]) and inner(c[1])))
        for index in range(TIE_SITES):
            for axis in (1, 0):          # Y and X sites in turn, each the first window that takes it (Y first: a wide grid has fewer rows to offer)
                any(_tie_place(placed, kind, ws, k, axis, index, ix, iy, H, W, rs) for ix, iy in cand[:TIE_TRIES])
    return placed


def _tie_place(placed, kind, ws, k, axis, index, ix, iy, H, W, rs):
    """Adds the index-th site of (ws, axis) at window (ix, iy) to `placed` if it can tie there and clashes with none (tie_sites)."""
    delta, nb = TIE_SETTINGS[kind]
    s = 1 << rs
    lw, lh = -(-W // s), -(-H // s)
    bias = 1 if k < 4 else 1 + (4 << nb)
    parent_bias = 1 if k - 1 < 4 else 1 + (4 << nb)
    thin = rs >= 1 and (index >> 1) & 1 == 0
    d = 1 if thin else ((1, 4, 9)[(index + k) % 3] if rs == 0 else 4 if s <= 4 else 9)
    cols = 1 if thin else -(-d // s)
    if 2 * cols > ws:
        d, cols, thin = 1, 1, rs >= 1
    i, dim = (ix, W) if axis == 0 else (iy, H)
    if i * ws * s < d or dim - 1 - (i * ws + ws - 1) * s < d:          # -d or +d would reach the reflection
        return False
    parent = None
    if k > 0:
        px, py = (ix // 2) * 2 * ws, (iy // 2) * 2 * ws
        parent = min(2 * ws, lw - px) * min(2 * ws, lh - py)
    along = axis == 1 and ws <= 4          # the bars run on through both neighbours
    amp = _tie_amplitude(ws, d, cols, thin, delta, bias, None if parent is None else parent // (2 if along else 1), parent_bias)
    if amp is None:
        return False
    x0, y0 = ix * ws, iy * ws
    marks = [x0, y0, x0 + ws, y0 + ws]
    if along:
        marks[0], marks[2] = x0 - ws, x0 + 2 * ws
        if marks[0] < 0 or marks[2] > lw:
            return False
    # what must stay free of other sites' marks: the samples this window's candidates see (+-16 pixels along the searched axis; farther ones
    # lose either way), and from the chain's fifth level on the windows whose offsets the neighbour term reads, two windows away on both axes
    m = [-(-16 // s) + 1, 0] if axis == 0 else [0, -(-16 // s) + 1]
    if k >= 4:
        m = [max(v, 3 * ws) for v in m]
    keep = [marks[0] - m[0], marks[1] - m[1], marks[2] + m[0], marks[3] + m[1]]
    clash = lambda r, q: r[0] < q[2] and q[0] < r[2] and r[1] < q[3] and q[1] < r[3]
    if any(clash(keep, p["marks"]) or clash(p["keep"], marks) for p in placed):
        return False
    placed.append(dict(set=index & 1, ws=ws, axis=axis, d=d, wx=x0, wy=y0, n=amp[0], a=amp[1], thin=thin, along=along, marks=marks, keep=keep))
    return True


def tie_frames(kind, H, W, hdr, seed, count=3, in_stride=0, rs=0):
    """Frame i of a tie kind: luma TIE_BASE, chroma mid-grey, and the marks of the sites of set i & 1 (tie_sites) -- frames N - 1 and N of a
    pair carry their marks in different windows; those of frame N add the same to every candidate of their window.
    P010: the flat level carries a low byte of all ones, the marks one of zero."""
    assert kind in TIE_KINDS, kind
    S = in_stride if in_stride > 0 else W
    s = 1 << rs
    sites = tie_sites(kind, H, W, rs, seed)
    code = (lambda v, low: (v << 8) | low) if hdr else (lambda v, low: v)
    out = []
    for i in range(count):
        f = np.zeros((H + H // 2, S), dtype=np.uint16 if hdr else np.uint8)
        f[:H, :W] = code(TIE_BASE, 0xFF)
        f[H:, :W] = code(128, 0xFF)
        for st in sites:
            if st["set"] != i & 1:
                continue
            ws, d = st["ws"], st["d"]
            u0, v0 = (st["wx"], st["wy"]) if st["axis"] == 0 else (st["wy"], st["wx"])       # u: the searched axis, v: across it
            first, last = u0 * s, (u0 + ws - 1) * s
            r0 = v0 + (ws - st["n"]) // 2
            across = (r0 * s - (s - 1), (r0 + st["n"] - 1) * s + s)
            if st["along"]:
                across = ((v0 - ws) * s, (v0 + 2 * ws) * s)
            across = (max(across[0], 0), min(across[1], W if st["axis"] == 1 else H))
            y = f[:H, :W] if st["axis"] == 0 else f[:H, :W].T
            for b0 in (first, last - d + 1):
                y[across[0]:across[1], b0:b0 + d] = code(TIE_BASE + st["a"], 0)
        out.append(f.reshape(-1))
    return out


def frames(kind, H, W, hdr, seed, count=3, in_stride=0, rs=0):
    """`count` consecutive frames of content `kind`: "patches", "noise" (every code value: for P010 the low six bits are set too), one of
    SAT_KINDS (rs: the resolution scalar of the geometry, which places the clean corner and the lattice of "specks"), one of DRIFT_KINDS or one
    of synth.SCENES.
    in_stride: row pitch in elements (0 = W)."""
    from hopperrender_amd import synth
    S = in_stride if in_stride > 0 else W
    if kind in SAT_KINDS:
        return [saturation_frame(kind, H, W, hdr, seed, i, in_stride, rs) for i in range(count)]
    if kind in DRIFT_KINDS:
        return drift_frames(kind, H, W, hdr, seed, count, in_stride)
    if kind in TIE_KINDS:
        return tie_frames(kind, H, W, hdr, seed, count, in_stride, rs)
    if kind == "patches":
        a = synth.Scene(H, W, hdr, seed=seed, in_stride=in_stride).frame(0)
        return [a, a] + [patched(a, H, S, hdr, seed + 1 + i) for i in range(count - 2)]
    if kind == "noise":
        return [synth.random_frame(H, W, hdr, seed=seed + i, in_stride=in_stride) for i in range(count)]
    sc = synth.ContentScene(kind, H, W, hdr, seed, in_stride=in_stride)
    return [sc.frame(i) for i in range(count)]
