"""What quality.evaluate(ssim_map=TILE, error_map=TILE) must report for a synth.Scene clip, from the CPU oracle: per evaluated pair the
SSIM map model (tests/frame_ssim_map_model.py) and the error map model applied to the oracle's warp_frames output against copy_frame of
the withheld frame -- the frames behind tests/quality_cases.py's sums.  Computed once per case.  Not a test module itself."""
import functools

import frame_error_map_model as fmm
import frame_ssim_map_model as smm
import quality_cases


@functools.lru_cache(maxsize=None)
def oracle_ssim_maps(hdr, H, W, seed, R, tile, n_frames=quality_cases.N_FRAMES):
    """[{pair, oob, ssim_map: the report's "ssim_map" entry with the "sse" join, luma: the Y plane of the SSIM map}] for the pairs the
    evaluator scores (pair p = sources (2 p, 2 p + 2), withheld 2 p + 1)"""
    from oracle import oracle
    oracle.build()
    f = quality_cases.clip(hdr, H, W, seed)
    g = oracle.make_geom(int(hdr), H, W)
    th, tw = fmm.map_shape(H, W, tile)
    out = []
    for p in range(1, (n_frames + 1) // 2 - 1):
        s0, s1, t = f[2 * p], f[2 * p + 2], f[2 * p + 1]
        _, blur, _, oob = oracle.calculate_optical_flow(s0, s1, g, R)
        shown, truth = oracle.warp_frames(s0, s1, blur, g, 0.5, 2), oracle.copy_frame(t, g)
        m, err = smm.frame_ssim_map(shown, truth, H, W, tile), fmm.frame_error_map(shown, truth, H, W, tile)
        out.append({"pair": p, "oob": oob, "luma": m[0],
                    "ssim_map": dict({"tile": tile, "shape": [th, tw]},
                                     **{pl: {"worst": smm.worst_tiles(m[i], tile, err[i]["sse"]), "worst_window_tile": smm.worst_window_tile(m[i], tile)}
                                        for i, pl in enumerate("YUV")})})
    return out
