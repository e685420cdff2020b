"""GPU: the leave-one-out evaluator (hopperrender_amd/quality.py) end to end -- one asynchronous context, hf_interpolate_period on device
frames, the truths and the repeat baseline through copyFrame of a second context, hf_frame_error_enqueue behind every period, one read.
Every integer of the report must equal the frame error model applied to the CPU oracle's frames for the same pairs."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quality_cases  # noqa: E402
from frame_error_model import FIELDS, PLANES, psnr  # noqa: E402

pytestmark = pytest.mark.gpu


def _check(report, hdr, H, W, seed, R):
    want = quality_cases.oracle_pairs(hdr, H, W, seed, R)
    peak = 65535 if hdr else 255
    assert report["geometry"] == {"width": W, "height": H, "hdr": hdr, "peak": peak, "frames": quality_cases.N_FRAMES}
    assert report["settings"]["search_radius"] == R and report["warmup_pairs"] == [0]
    assert [r["pair"] for r in report["pairs"]] == [w["pair"] for w in want] == [1, 2, 3]
    for r, w in zip(report["pairs"], want):
        assert w["oob"] == 0
        for kind in ("interpolated", "repeat"):
            for p in PLANES:
                got = r[kind][p]
                assert {k: got[k] for k in FIELDS} == w[kind][p], (r["pair"], kind, p)
                assert all(type(got[k]) is int for k in FIELDS)
                f = psnr(got["sse"], got["count"], peak)
                assert got["psnr"] == (None if f is None else pytest.approx(f, rel=1e-12))
        assert r["interpolated"]["Y"]["n_differ"] > 0 and r["gain_db_y"] == pytest.approx(r["interpolated"]["Y"]["psnr"] - r["repeat"]["Y"]["psnr"])
    for kind in ("interpolated", "repeat"):
        for p in PLANES:
            sse, cnt = sum(w[kind][p]["sse"] for w in want), sum(w[kind][p]["count"] for w in want)
            agg = report["clip"][kind][p]
            assert (agg["sse"], agg["count"]) == (sse, cnt) and agg["psnr"] == pytest.approx(psnr(sse, cnt, peak), rel=1e-12)
    ys = [r["interpolated"]["Y"]["psnr"] for r in report["pairs"]]
    assert report["clip"]["worst_pair"] == {"pair": report["pairs"][ys.index(min(ys))]["pair"], "psnr_y": min(ys)}
    assert json.loads(json.dumps(report)) == report


@pytest.mark.parametrize("hdr,H,W", [(False, 180, 320), (True, 360, 640)], ids=["sdr180", "hdr360"])
def test_evaluate_equals_the_model_on_the_oracles_frames(native_lib, hdr, H, W):
    from hopperrender_amd import quality
    frames = quality_cases.clip(hdr, H, W, 1234)
    report = quality.evaluate(frames, hdr, H, W, search_radius=16)
    _check(report, hdr, H, W, 1234, 16)
    assert report["scene_cuts"] is None
    assert report["clip"]["gain_db_y"] >= 2.0   # (tests/test_quality.py holds the oracle to this per pair)


def test_scene_cut_kinds_on_request(native_lib):
    """detect_scene_cuts reports the filter's decision per period and changes no sum.  Up to period 4 the filter has at most three deltas,
    the newest two equal to their own average: no cut whatever the content (hf_filter.cpp); the last period re-submits a frame."""
    from hopperrender_amd import quality
    H, W = 180, 320
    report = quality.evaluate(quality_cases.clip(False, H, W, 1234), False, H, W, search_radius=16, detect_scene_cuts=True)
    _check(report, False, H, W, 1234, 16)
    cuts = report["scene_cuts"]
    assert [(c["period"], c["pair"]) for c in cuts] == [(2, 0), (3, 1), (4, 2), (5, 3)]
    assert [c["kind"] for c in cuts[:3]] == ["warp"] * 3 and cuts[3]["kind"] in ("warp", "copy")
    assert all(c["total_frame_delta"] > 0 for c in cuts[:3])


def test_sweep_through_main(native_lib, tmp_path, capsys):
    """python -m hopperrender_amd.quality clip.nv12 --width 320 --height 180 --sweep radius=5,16 --report out.json"""
    from hopperrender_amd import quality
    H, W = 180, 320
    clip = tmp_path / "clip.nv12"
    with open(clip, "wb") as f:
        for fr in quality_cases.clip(False, H, W, 1234):
            f.write(np.ascontiguousarray(fr).tobytes())
    out = tmp_path / "out.json"
    reports = quality.main([str(clip), "--width", str(W), "--height", str(H), "--sweep", "radius=5,16", "--report", str(out)])
    assert [r["settings"]["search_radius"] for r in reports] == [5, 16]
    _check(reports[0], False, H, W, 1234, 5)
    _check(reports[1], False, H, W, 1234, 16)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("search_radius=")]
    assert len(lines) == 2 and lines[0].startswith("search_radius=5 ") and lines[1].startswith("search_radius=16 ")
    assert json.load(open(out))["reports"] == reports
