"""Frames for the chain's GPU tests (test_sad_reuse_gpu.py, test_chain_variants_gpu.py): the bench's content classes, noise patches inside a
static frame, and full-range noise."""
import numpy as np


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


def frames(kind, H, W, hdr, seed, count=3, in_stride=0):
    """`count` consecutive frames of content `kind`: "patches", "noise" (every code value: for P010 the low six bits are set too) or one of
    synth.SCENES.  in_stride: row pitch in elements (0 = W)."""
    from hopperrender_amd import synth
    S = in_stride if in_stride > 0 else W
    if kind == "patches":
        a = synth.Scene(H, W, hdr, seed=seed, in_stride=in_stride).frame(0)
        return [a, a] + [patched(a, H, S, hdr, seed + 1 + i) for i in range(count - 2)]
    if kind == "noise":
        return [synth.random_frame(H, W, hdr, seed=seed + i, in_stride=in_stride) for i in range(count)]
    sc = synth.ContentScene(kind, H, W, hdr, seed, in_stride=in_stride)
    return [sc.frame(i) for i in range(count)]
