"""GPU: the evaluator's error-map option end to end -- hf_frame_error_map_enqueue behind every evaluated pair's error launch, one buffer,
one read.  Per pair the worst tiles and the share figure must be those the map model gives on the CPU oracle's frames, and the rest of
the report must be the report of a run without the option."""
import copy
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quality_cases  # noqa: E402
import quality_map_cases  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("hdr,H,W", [(False, 180, 320), (True, 360, 640)], ids=["sdr180", "hdr360"])
def test_evaluate_locates_the_error_where_the_model_does(native_lib, hdr, H, W, tmp_path):
    from hopperrender_amd import quality
    frames = quality_cases.clip(hdr, H, W, 1234)
    report = quality.evaluate(frames, hdr, H, W, search_radius=16, error_map=16, map_dir=str(tmp_path))
    want = quality_map_cases.oracle_maps(hdr, H, W, 1234, 16, 16)
    assert [r["pair"] for r in report["pairs"]] == [w["pair"] for w in want] == [1, 2, 3]
    for r, w in zip(report["pairs"], want):
        assert w["oob"] == 0
        got = r["interpolated"]["map"]
        assert got == w["map"], r["pair"]
        # the worst tile is a tile of the frame, and the map accounts for the whole error of the plane
        assert got["shape"] == [(H + 15) // 16, (W + 15) // 16] and 0 < got["Y"]["share_top1pct"] <= 1
        assert got["Y"]["worst"][0]["sse"] <= r["interpolated"]["Y"]["sse"] and got["Y"]["worst"][0]["max_abs"] <= r["interpolated"]["Y"]["max_abs"]
    tops = [(r["interpolated"]["map"]["Y"]["worst"][0], r["pair"]) for r in report["pairs"]]
    t, pair = max(tops, key=lambda x: x[0]["sse"])
    assert report["clip"]["worst_tile"] == {"pair": pair, "plane": "Y", "x": t["x"], "y": t["y"], "sse": t["sse"]}
    assert json.loads(json.dumps(report)) == report
    assert sorted(os.listdir(tmp_path)) == ["map_pair0001.pgm", "map_pair0002.pgm", "map_pair0003.pgm"]
    assert open(tmp_path / "map_pair0001.pgm", "rb").read().startswith(b"P5\n%d %d\n255\n" % ((W + 15) // 16, (H + 15) // 16))
    # the rest of the report: the run without the option
    plain = quality.evaluate(frames, hdr, H, W, search_radius=16)
    rest = copy.deepcopy(report)
    del rest["clip"]["worst_tile"]
    for r in rest["pairs"]:
        del r["interpolated"]["map"]
    assert rest == plain
