"""GPU: the evaluator's SSIM-map option end to end -- hf_frame_ssim_map_enqueue behind every evaluated pair's error launch beside the
error map of the same tile size, one buffer each, one read each.  Per pair the worst tiles with their squared error, the tile of the
worst window, the clip's worst tile and the heat map must be those the map models give on the CPU oracle's frames, and the rest of the
report must be the report of a run without the option."""
import copy
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frame_ssim_map_model as smm  # noqa: E402
import quality_cases  # noqa: E402
import quality_ssim_map_cases  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("hdr,H,W", [(False, 180, 320), (True, 360, 640)], ids=["sdr180", "hdr360"])
def test_evaluate_locates_the_structural_loss_where_the_model_does(native_lib, hdr, H, W, tmp_path):
    from hopperrender_amd import quality
    frames = quality_cases.clip(hdr, H, W, 1234)
    report = quality.evaluate(frames, hdr, H, W, search_radius=16, ssim=True, ssim_map=16, error_map=16, map_dir=str(tmp_path))
    want = quality_ssim_map_cases.oracle_ssim_maps(hdr, H, W, 1234, 16, 16)
    assert [r["pair"] for r in report["pairs"]] == [w["pair"] for w in want] == [1, 2, 3]
    th, tw = (H + 15) // 16, (W + 15) // 16
    for r, w in zip(report["pairs"], want):
        assert w["oob"] == 0
        got = r["interpolated"]["ssim_map"]
        assert got == w["ssim_map"], r["pair"]
        assert got["shape"] == [th, tw] and len(got["Y"]["worst"]) == 5 and got["Y"]["worst"][0]["sum_loss_q32"] > 0
        # the tile of the worst window holds the plane's max_loss_q32 of --ssim, the location that option alone cannot give
        for p in "YUV":
            assert got[p]["worst_window_tile"]["max_loss_q32"] == r["interpolated"][p]["max_loss_q32"]
            assert all(t["sum_loss_q32"] <= r["interpolated"][p]["sum_loss_q32"] and t["sse"] <= r["interpolated"][p]["sse"] for t in got[p]["worst"])
        # the join: the error map's own worst tile carries the same sse wherever it is also among the SSIM map's worst
        top = r["interpolated"]["map"]["Y"]["worst"][0]
        assert all(t["sse"] == top["sse"] for t in got["Y"]["worst"] if (t["x"], t["y"]) == (top["x"], top["y"]))
    # the clip's worst luma tile: the pairs' own worst tiles compared as fractions, the earlier pair of equals
    tops = [(r["interpolated"]["ssim_map"]["Y"]["worst"][0], r["pair"]) for r in report["pairs"]]
    t, pair = min(tops, key=lambda x: (-smm.Fraction(x[0]["sum_loss_q32"], x[0]["count"]), x[1]))
    assert report["clip"]["worst_tile_ssim"] == {"pair": pair, "plane": "Y", "x": t["x"], "y": t["y"], "ssim": t["ssim"]}
    assert json.loads(json.dumps(report)) == report
    assert sorted(os.listdir(tmp_path)) == [f"{kind}_pair000{k}.pgm" for kind in ("map", "ssim") for k in (1, 2, 3)]
    raw = open(tmp_path / "ssim_pair0002.pgm", "rb").read()
    head = b"P5\n%d %d\n255\n" % (tw, th)
    assert raw.startswith(head) and list(raw[len(head):]) == smm.pgm_values(want[1]["luma"]) and max(raw[len(head):]) > 0
    # the rest of the report: the run without the option
    plain = quality.evaluate(frames, hdr, H, W, search_radius=16, ssim=True, error_map=16)
    rest = copy.deepcopy(report)
    del rest["clip"]["worst_tile_ssim"]
    for r in rest["pairs"]:
        del r["interpolated"]["ssim_map"]
    assert rest == plain
