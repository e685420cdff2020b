"""GPU: the leave-one-out evaluator with its SSIM option (hopperrender_amd/quality.py, evaluate(ssim=True) / --ssim) end to end:
hf_frame_ssim_enqueue beside every hf_frame_error_enqueue, one read of each.  Every SSIM integer of the report must equal the model of
tests/frame_ssim_model.py applied to the CPU oracle's frames for the same pairs, and the error sums must still equal theirs."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quality_cases  # noqa: E402
import quality_ssim_cases as qsc  # noqa: E402
from frame_error_model import FIELDS, PLANES  # noqa: E402

pytestmark = pytest.mark.gpu
ONE = 4294967296.0
NEW_PLANE_KEYS = {"sum_loss_q32", "max_loss_q32", "ssim_count", "ssim", "min_ssim"}


def _floats(total, worst, count):
    return {"ssim": 1.0 - total / ONE / count if count else None, "min_ssim": 1.0 - worst / ONE if count else None}


def _check(report, hdr, H, W, seed, R):
    want, want_err = qsc.oracle_ssim_pairs(hdr, H, W, seed, R), quality_cases.oracle_pairs(hdr, H, W, seed, R)
    assert [r["pair"] for r in report["pairs"]] == [w["pair"] for w in want] == [1, 2, 3]
    for r, w, e in zip(report["pairs"], want, want_err):
        assert w["oob"] == 0
        for kind in ("interpolated", "repeat"):
            for p in PLANES:
                got = r[kind][p]
                assert {k: got[k] for k in FIELDS} == e[kind][p], (r["pair"], kind, p)          # the error sums are today's
                mine = {"sum_loss_q32": got["sum_loss_q32"], "max_loss_q32": got["max_loss_q32"], "count": got["ssim_count"]}
                assert mine == w[kind][p], (r["pair"], kind, p)
                assert all(type(v) is int for v in mine.values())
                assert {k: got[k] for k in ("ssim", "min_ssim")} == _floats(*mine.values())
        assert r["interpolated"]["Y"]["ssim_count"] == (W // 4 - 1) * (H // 4 - 1) and r["interpolated"]["U"]["ssim_count"] == (W // 8 - 1) * (H // 8 - 1)
        assert r["gain_ssim_y"] == r["interpolated"]["Y"]["ssim"] - r["repeat"]["Y"]["ssim"]
    for kind in ("interpolated", "repeat"):
        for p in PLANES:
            total, count = sum(w[kind][p]["sum_loss_q32"] for w in want), sum(w[kind][p]["count"] for w in want)
            worst = max(w[kind][p]["max_loss_q32"] for w in want)
            agg = report["clip"][kind][p]
            assert (agg["sum_loss_q32"], agg["max_loss_q32"], agg["ssim_count"]) == (total, worst, count)
            assert {k: agg[k] for k in ("ssim", "min_ssim")} == _floats(total, worst, count)
            assert agg["sse"] == sum(e[kind][p]["sse"] for e in want_err)
    clip = report["clip"]
    assert clip["gain_ssim_y"] == clip["interpolated"]["Y"]["ssim"] - clip["repeat"]["Y"]["ssim"]
    ys = [r["interpolated"]["Y"]["ssim"] for r in report["pairs"]]
    assert clip["worst_pair_ssim"] == {"pair": report["pairs"][ys.index(min(ys))]["pair"], "ssim_y": min(ys)}
    assert json.loads(json.dumps(report)) == report


@pytest.mark.parametrize("hdr,H,W", [(False, 180, 320), (True, 360, 640)], ids=["sdr180", "hdr360"])
def test_evaluate_with_ssim_equals_the_model_on_the_oracles_frames(native_lib, hdr, H, W):
    from hopperrender_amd import quality
    frames = quality_cases.clip(hdr, H, W, 1234)
    report = quality.evaluate(frames, hdr, H, W, search_radius=16, ssim=True)
    _check(report, hdr, H, W, 1234, 16)
    assert report["clip"]["gain_ssim_y"] >= 0.5   # (tests/test_quality_ssim.py holds the oracle to this per pair)
    # off: none of the new keys, and everything else equal to the report above
    plain = quality.evaluate(frames, hdr, H, W, search_radius=16)
    assert not {"gain_ssim_y", "worst_pair_ssim"} & set(plain["clip"]) and all("gain_ssim_y" not in r for r in plain["pairs"])
    for r, q in zip(plain["pairs"] + [plain["clip"]], report["pairs"] + [report["clip"]]):
        for kind in ("interpolated", "repeat"):
            for p in PLANES:
                assert not NEW_PLANE_KEYS & set(r[kind][p])
                assert r[kind][p] == {k: v for k, v in q[kind][p].items() if k not in NEW_PLANE_KEYS}
    assert plain["clip"]["worst_pair"] == report["clip"]["worst_pair"] and plain["settings"] == report["settings"]


def test_ssim_sweep_through_main(native_lib, tmp_path, capsys):
    """python -m hopperrender_amd.quality clip.nv12 --width 320 --height 180 --ssim --sweep radius=5,16 --report out.json"""
    from hopperrender_amd import quality
    H, W = 180, 320
    clip = tmp_path / "clip.nv12"
    with open(clip, "wb") as f:
        for fr in quality_cases.clip(False, H, W, 1234):
            f.write(np.ascontiguousarray(fr).tobytes())
    out = tmp_path / "out.json"
    reports = quality.main([str(clip), "--width", str(W), "--height", str(H), "--ssim", "--sweep", "radius=5,16", "--report", str(out)])
    assert [r["settings"]["search_radius"] for r in reports] == [5, 16]
    _check(reports[0], False, H, W, 1234, 5)
    _check(reports[1], False, H, W, 1234, 16)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("search_radius=")]
    assert len(lines) == 2 and lines[0].startswith("search_radius=5 ") and lines[1].startswith("search_radius=16 ")
    assert all("SSIM Y/U/V" in ln and "repeat Y" in ln and "worst window" in ln for ln in lines)
    assert json.load(open(out))["reports"] == reports
