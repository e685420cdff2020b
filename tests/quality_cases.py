"""What quality.evaluate must report for a synth.Scene clip, from the CPU oracle: per evaluated pair the frame error model
(tests/frame_error_model.py) applied to the oracle's warp_frames / copy_frame / calculate_optical_flow.  Computed once per case and shared
by tests/test_quality.py (the sanity condition) and tests/test_quality_gpu.py (equality with the device).  Not a test module itself."""
import functools

from frame_error_model import frame_error

N_FRAMES = 9   # sources 0, 2, 4, 6, 8; withheld 1, 3, 5, 7; pair 0 is warm-up, pairs 1 .. 3 are scored


@functools.lru_cache(maxsize=None)
def clip(hdr, H, W, seed):
    from hopperrender_amd import synth
    sc = synth.Scene(H, W, hdr, seed)
    return tuple(sc.frame(k) for k in range(N_FRAMES))


@functools.lru_cache(maxsize=None)
def oracle_pairs(hdr, H, W, seed, R, n_frames=N_FRAMES):
    """[{pair, interpolated: model sums, repeat: model sums, oob}] for the pairs the evaluator scores: pair p = sources (2 p, 2 p + 2),
    withheld frame 2 p + 1, p >= 1; default knobs but the search radius; levels 0 .. 255 (HDR: the x 65535 / 65280 stretch)."""
    from oracle import oracle
    oracle.build()
    f = clip(hdr, H, W, seed)
    g = oracle.make_geom(int(hdr), H, W)
    out = []
    for p in range(1, (n_frames + 1) // 2 - 1):
        s0, s1, t = f[2 * p], f[2 * p + 2], f[2 * p + 1]
        _, blur, _, oob = oracle.calculate_optical_flow(s0, s1, g, R)
        truth = oracle.copy_frame(t, g)
        out.append({"pair": p, "oob": oob,
                    "interpolated": frame_error(oracle.warp_frames(s0, s1, blur, g, 0.5, 2), truth, H, W),
                    "repeat": frame_error(oracle.copy_frame(s0, g), truth, H, W)})
    return out
