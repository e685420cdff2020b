"""GPU: the evaluator's guard option end to end on a 6-frame synthetic scene at 320 x 180 -- with the guard off the guarded blocks are
the plain ones and the gain is 0; with every tile firing they are those of the cross-fade, computed here from a zero-flow warpFrames;
and the plain blocks of the report are those of a run without the option."""
import copy
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from frame_error_model import FIELDS, frame_error, psnr  # noqa: E402

pytestmark = pytest.mark.gpu

H, W, R = 180, 320, 8
CASES = [(False, 41), (True, 42)]


def _clip(hdr, seed):
    from hopperrender_amd import synth
    sc = synth.Scene(H, W, hdr, seed)
    return [sc.frame(k) for k in range(6)]


def _without_guard(report):
    rest = copy.deepcopy(report)
    del rest["guard"], rest["clip"]["guarded"], rest["clip"]["guard_gain_db"]
    rest["clip"].pop("guard_gain_ssim", None)
    for r in rest["pairs"]:
        del r["guarded"], r["guard_gain_db"]
        r.pop("guard_gain_ssim", None)
    return rest


@pytest.mark.parametrize("hdr,seed", CASES, ids=["sdr", "hdr"])
def test_guard_off_is_the_plain_run_and_the_plain_blocks_never_move(native_lib, hdr, seed):
    from hopperrender_amd import quality
    frames = _clip(hdr, seed)
    plain = quality.evaluate(frames, hdr, H, W, search_radius=R, ssim=True, error_map=16)
    report = quality.evaluate(frames, hdr, H, W, search_radius=R, ssim=True, error_map=16, guard=(16, 4080, 4081))
    assert [r["pair"] for r in report["pairs"]] == [1] and report["guard"] == {"tile": 16, "lo_q4": 4080, "hi_q4": 4081}
    for r in report["pairs"]:
        g = dict(r["guarded"])
        assert g.pop("mask") == {"tiles": 12 * 20, "tiles_firing": 0, "mean_weight": 0.0}
        assert g == {k: r["interpolated"][k] for k in ("Y", "U", "V", "map")}
        assert r["guard_gain_db"] == 0 and r["guard_gain_ssim"] == 0 and r["interpolated"]["Y"]["sse"] > 0
    c = report["clip"]
    assert {p: c["guarded"][p] for p in "YUV"} == c["interpolated"] and c["guard_gain_db"] == 0 and c["guard_gain_ssim"] == 0
    assert json.loads(json.dumps(report)) == report
    assert _without_guard(report) == plain


@pytest.mark.parametrize("hdr,seed", CASES, ids=["sdr", "hdr"])
def test_every_tile_firing_is_the_cross_fade(native_lib, hdr, seed, tmp_path):
    from hopperrender_amd import quality
    from hopperrender_amd.calc import OpticalFlowCalcHDR, OpticalFlowCalcSDR
    from oracle import oracle
    frames = _clip(hdr, seed)
    g = oracle.make_geom(int(hdr), H, W, 0, 0, 270)
    peak = 65535 if hdr else 255
    report = quality.evaluate(frames, hdr, H, W, search_radius=R, guard=(16, 0, 1), map_dir=str(tmp_path))
    plain = quality.evaluate(frames, hdr, H, W, search_radius=R)
    assert _without_guard(report) == plain and [r["pair"] for r in report["pairs"]] == [1]
    c = (OpticalFlowCalcHDR if hdr else OpticalFlowCalcSDR)(H, W, search_radius=R)
    try:
        total = {p: {"sse": 0, "count": 0} for p in "YUV"}
        for r in report["pairs"]:
            p = r["pair"]
            s0, s1, truth = frames[2 * p], frames[2 * p + 2], frames[2 * p + 1]
            for x in (s0, s1, s1):
                c.updateFrame(x)                     # the ring: s0, s1 | s1
            c.sync()
            c.writeBlurredFlow(0, np.zeros((2, c.m_opticalFlowFrameHeight, c.m_opticalFlowFrameWidth), np.int16))
            c.warpFrames(0.5, 2)
            fade = c.downloadFrame().copy()
            want = frame_error(fade, oracle.copy_frame(truth, g), H, W)   # (the truth goes through copyFrame at the same levels)
            for pl in "YUV":
                got = r["guarded"][pl]
                assert {k: got[k] for k in FIELDS} == want[pl] and got["psnr"] == psnr(want[pl]["sse"], want[pl]["count"], peak), (p, pl)
                total[pl]["sse"] += want[pl]["sse"]; total[pl]["count"] += want[pl]["count"]
            assert r["guarded"]["mask"] == {"tiles": 12 * 20, "tiles_firing": 12 * 20, "mean_weight": 1.0}
            assert r["guard_gain_db"] == r["guarded"]["Y"]["psnr"] - r["interpolated"]["Y"]["psnr"] != 0
        for pl in "YUV":
            assert report["clip"]["guarded"][pl]["sse"] == total[pl]["sse"] and report["clip"]["guarded"][pl]["psnr"] == psnr(total[pl]["sse"], total[pl]["count"], peak)
    finally:
        c.close()
    mask = open(tmp_path / "guard_pair0001.pgm", "rb").read()
    head = b"P5\n%d %d\n255\n" % (W, H)
    assert sorted(os.listdir(tmp_path)) == ["guard_pair0001.pgm"] and mask.startswith(head) and mask[len(head):] == b"\xff" * (H * W)
