"""GPU: the evaluator's disagreement option and the confidence run end to end on a short synthetic clip at 96 x 64 -- the integers of
the reports must be those of the model (tests/warp_disagreement_model.py) on the CPU oracle's flows, the overlap figure must follow
from the two maps, and the rest of evaluate's report must be the report of a run without the option."""
import copy
import json
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frame_error_map_model as fmm  # noqa: E402
import quality_cases  # noqa: E402
import warp_disagreement_model as wdm  # noqa: E402

pytestmark = pytest.mark.gpu

H, W, TILE, R = 64, 96, 16, 8
S24, T60 = 417083, 166833
CASES = [(False, 270), (True, 32)]   # rs 0: every element through warp_element; rs 1: the run kernel


def _flow(f0, f1, g):
    from oracle import oracle
    _, blur, _, oob = oracle.calculate_optical_flow(f0, f1, g, R)
    assert oob == 0
    return blur


def _totals(m):
    return {"sse": int(m["sse"].astype(object).sum()), "sad": int(m["sad"].astype(object).sum()), "max_abs": int(m["max_abs"].max())}


@pytest.mark.parametrize("hdr,res", CASES, ids=["sdr-rs0", "hdr-rs1"])
def test_evaluate_reports_the_models_disagreement_beside_the_error_map(native_lib, hdr, res, tmp_path):
    from hopperrender_amd import quality
    from oracle import oracle
    frames = quality_cases.clip(hdr, H, W, 77)
    g = oracle.make_geom(int(hdr), H, W, 0, 0, res)
    report = quality.evaluate(frames, hdr, H, W, search_radius=R, max_calc_res=res, error_map=TILE, disagreement=TILE, map_dir=str(tmp_path))
    assert [r["pair"] for r in report["pairs"]] == [1, 2, 3]
    hits = {p: [0, 0] for p in "YUV"}
    for r in report["pairs"]:
        p = r["pair"]
        s0, s1, truth = frames[2 * p], frames[2 * p + 2], frames[2 * p + 1]
        flow = _flow(s0, s1, g)
        dis = wdm.warp_disagreement_map(s0, s1, flow, g, 0.5, TILE)
        err = fmm.frame_error_map(oracle.warp_frames(s0, s1, flow, g, 0.5, 2), oracle.copy_frame(truth, g), H, W, TILE)
        got = r["interpolated"]["disagreement"]
        assert got["tile"] == TILE and got["shape"] == [4, 6]
        for i, pl in enumerate("YUV"):
            k = 1   # 24 tiles
            want = dict({"worst": fmm.worst_tiles(dis[i], TILE), "share_top1pct": fmm.share_top1pct(dis[i])}, **_totals(dis[i]))
            both = int(err[i]["sse"].sum()) and want["sse"]
            top = lambda m: [(t["x"], t["y"]) for t in fmm.worst_tiles(m, TILE, k)]
            want["overlap_top1pct"] = len(set(top(err[i])) & set(top(dis[i]))) / k if both else None
            if both:
                hits[pl][0] += len(set(top(err[i])) & set(top(dis[i]))); hits[pl][1] += k
            assert got[pl] == want, (p, pl)
        assert got["Y"]["sse"] > 0
    for pl in "YUV":
        assert report["clip"]["disagreement"][pl] == {"sse": sum(r["interpolated"]["disagreement"][pl]["sse"] for r in report["pairs"]),
                                                      "overlap_top1pct": hits[pl][0] / hits[pl][1] if hits[pl][1] else None}
    assert json.loads(json.dumps(report)) == report
    assert sorted(os.listdir(tmp_path)) == [f"{k}_pair000{i}.pgm" for k in ("dis", "map") for i in (1, 2, 3)]
    plain = quality.evaluate(frames, hdr, H, W, search_radius=R, max_calc_res=res, error_map=TILE)
    rest = copy.deepcopy(report)
    del rest["clip"]["disagreement"], rest["clip"]["worst_tile_disagreement"]
    for r in rest["pairs"]:
        del r["interpolated"]["disagreement"]
    assert rest == plain


@pytest.mark.parametrize("hdr,res", CASES, ids=["sdr-rs0", "hdr-rs1"])
def test_confidence_reports_the_models_integers_at_the_real_schedule(native_lib, hdr, res):
    from hopperrender_amd import quality
    from oracle import oracle
    frames = quality_cases.clip(hdr, H, W, 77)[:6]
    g = oracle.make_geom(int(hdr), H, W, 0, 0, res)
    report = quality.confidence(frames, hdr, H, W, source_frame_time=S24, target_frame_time=T60, tile=TILE, search_radius=R, max_calc_res=res)
    sched = quality.confidence_schedule(6, S24, T60)
    assert report["warmup_pairs"] == [0] and [r["pair"] for r in report["periods"]] == [1, 2, 3, 4] and report["shape"] == [4, 6]
    worst = None
    for r, s in zip(report["periods"], sched[3:]):
        p = r["pair"]
        assert r["t"] == s["t"] and r["source_frames"] == [p, p + 1]
        flow = _flow(frames[p], frames[p + 1], g)
        maps = wdm.warp_disagreement_maps(frames[p], frames[p + 1], flow, g, [np.float32(t) for t in r["t"]], TILE)
        for o, m in zip(r["outputs"], maps):
            for i, (pl, cnt) in enumerate((("Y", H * W), ("U", H * W // 4), ("V", H * W // 4))):
                want = _totals(m[i])
                want.update(rms=math.sqrt(want["sse"] / cnt), worst=fmm.worst_tiles(m[i], TILE, 1)[0])
                assert o[pl] == want, (p, o["t"], pl)
            if worst is None or o["Y"]["sse"] > worst[1]:
                worst = ({"period": r["period"], "pair": p, "t": o["t"], "rms_y": o["Y"]["rms"]}, o["Y"]["sse"])
    assert report["clip"]["worst"] == worst[0] and worst[1] > 0
    assert report["clip"]["mean_rms_y"] == [r["mean_rms_y"] for r in report["periods"]]
    assert json.loads(json.dumps(report)) == report
