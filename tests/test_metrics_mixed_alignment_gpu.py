"""GPU: mixed alignment inside ONE launch of the four frame metrics (csrc/hf_metrics.hip).  The launchers share one derivation of how a
frame lies in memory, and it takes one decision for the whole launch: a single frame whose base is not 16-byte aligned turns the wide
loads off for every pair.  Here every pitch allows wide loads and five of the six frames are aligned; all four calls must still equal
their numpy models, integer for integer."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_frame_error_map_gpu as femg  # noqa: E402
import test_frame_ssim_gpu as fsg  # noqa: E402
from frame_error_map_model import frame_error_map  # noqa: E402
from frame_error_model import PLANES, frame_error  # noqa: E402
from frame_ssim_cases import ints, random_frame  # noqa: E402
from frame_ssim_map_cases import maps, same  # noqa: E402
from frame_ssim_map_model import frame_ssim_map, totals  # noqa: E402
from frame_ssim_model import frame_ssim  # noqa: E402

pytestmark = pytest.mark.gpu
dev, ctx = fsg.dev, fsg.ctx   # the fixtures of the SSIM tests: uploaded frames, one context per geometry


@pytest.mark.parametrize("planar", [False, True], ids=["semi", "planar"])
@pytest.mark.parametrize("hdr", [False, True], ids=["sdr", "hdr"])
def test_one_unaligned_frame_among_three_pairs(ctx, dev, hdr, planar):
    """70 x 38 (ragged row tail, windowless edge tiles, an odd chroma row count) with strides 80 / 80 -- rows are 16-byte multiples at
    both element sizes -- three pairs a launch, every element random, the padding included.  Every frame starts at its allocation but
    frame b of pair 1, which lies 2 elements in.  Error sums, SSIM, error maps and SSIM maps (tile 16) of all three pairs equal their
    models, and every pair's maps add up to its slots."""
    H, W, S, tile = 38, 70, 80, 16
    c = ctx(hdr, H, W)
    rng = np.random.default_rng(71 + 2 * hdr + planar)
    fa, fb = [random_frame(rng, hdr, H, S) for _ in range(3)], [random_frame(rng, hdr, H, S) for _ in range(3)]
    pa, pb = [dev.put(a) for a in fa], [dev.put(b, 2 if i == 1 else 0) for i, b in enumerate(fb)]
    assert [p % 16 for p in pa + pb] == [0, 0, 0, 0, 4 if hdr else 2, 0]
    c.frameErrorEnqueue(pa, pb, 3, S, S, planar)
    c.frameSsimEnqueue(pa, pb, 3, S, S, planar)
    err, ssim = c.frameErrorRead(3, 3), [ints(g) for g in c.frameSsimRead(3, 3)]
    emap, smap = femg._maps(c, pa, pb, tile, S, S, planar), maps(c, pa, pb, tile, S, S, planar)
    for i, (a, b) in enumerate(zip(fa, fb)):
        assert err[i] == frame_error(a, b, H, W, S, S, planar), (hdr, planar, i)
        assert ssim[i] == frame_ssim(a, b, H, W, S, S, planar), (hdr, planar, i)
        femg._same(emap[i], frame_error_map(a, b, H, W, tile, S, S, planar), (hdr, planar, i))
        same(smap[i], frame_ssim_map(a, b, H, W, tile, S, S, planar), (hdr, planar, i))
        assert femg._sums(emap[i]) == {p: {k: err[i][p][k] for k in ("sse", "sad", "max_abs")} for p in PLANES}, (hdr, planar, i)
        assert totals(smap[i]) == ssim[i], (hdr, planar, i)
