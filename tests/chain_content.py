"""Frames for the chain's GPU tests (test_sad_reuse_gpu.py, test_chain_variants_gpu.py, test_chain_saturation_gpu.py,
test_chain_deep_rs_gpu.py): the bench's content classes, noise patches inside a static frame, full-range noise, the drift kinds (DRIFT_KINDS:
one noise field seen through a frame that moves by an odd number of pixels a frame, so that windows at a frame edge settle on offsets that
point out of the frame at a phase that is neither 0 nor even: drift_frames), and the saturation kinds (SAT_KINDS) -- pairs whose SADs sit
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
KIND_ORDER = ("patches", "chaotic", "noise", "static", "bench", "cut", "pan64") + SAT_KINDS + DRIFT_KINDS
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
    if kind == "patches":
        a = synth.Scene(H, W, hdr, seed=seed, in_stride=in_stride).frame(0)
        return [a, a] + [patched(a, H, S, hdr, seed + 1 + i) for i in range(count - 2)]
    if kind == "noise":
        return [synth.random_frame(H, W, hdr, seed=seed + i, in_stride=in_stride) for i in range(count)]
    sc = synth.ContentScene(kind, H, W, hdr, seed, in_stride=in_stride)
    return [sc.frame(i) for i in range(count)]
