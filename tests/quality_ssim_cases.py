"""What quality.evaluate(ssim=True) must report for a synth.Scene clip, from the CPU oracle: the frames tests/quality_cases.oracle_pairs
builds (the oracle's warp_frames / copy_frame / calculate_optical_flow on quality_cases.clip), scored with the SSIM model of
tests/frame_ssim_model.py.  Computed once per case and shared by tests/test_quality_ssim.py and tests/test_quality_ssim_gpu.py.  Not a
test module itself."""
import functools

import quality_cases
from frame_ssim_model import frame_ssim


@functools.lru_cache(maxsize=None)
def oracle_ssim_pairs(hdr, H, W, seed, R, n_frames=quality_cases.N_FRAMES):
    """[{pair, interpolated: model SSIM integers, repeat: the same, oob}] for pairs p >= 1: sources (2 p, 2 p + 2), withheld frame 2 p + 1."""
    from oracle import oracle
    oracle.build()
    f = quality_cases.clip(hdr, H, W, seed)
    g = oracle.make_geom(int(hdr), H, W)
    out = []
    for p in range(1, (n_frames + 1) // 2 - 1):
        s0, s1, t = f[2 * p], f[2 * p + 2], f[2 * p + 1]
        _, blur, _, oob = oracle.calculate_optical_flow(s0, s1, g, R)
        truth = oracle.copy_frame(t, g)
        out.append({"pair": p, "oob": oob,
                    "interpolated": frame_ssim(oracle.warp_frames(s0, s1, blur, g, 0.5, 2), truth, H, W),
                    "repeat": frame_ssim(oracle.copy_frame(s0, g), truth, H, W)})
    return out


def mean(d):
    return 1.0 - d["sum_loss_q32"] / 4294967296.0 / d["count"]
