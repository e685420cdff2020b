"""CPU: the evaluator's guard option without a GPU, against a recording fake device in the style of tests/test_quality_disagreement.py --
--guard TILE:LO:HI parsing and refusals, what is called on the clip's context and in which order, the result slots and buffer offsets,
what the report gains (and that it gains nothing and calls nothing when the option is off), and the mask's PGM."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frame_error_map_model as fmm  # noqa: E402
import test_quality as tq  # noqa: E402
import test_quality_disagreement as tqd  # noqa: E402
import test_quality_map as tqm  # noqa: E402

TW, TH, MAP_BYTES = tqm.TW, tqm.TH, tqm.MAP_BYTES
H, W = 32, 48          # 2 x 3 tiles of 16: the grid the fake context reports


def _fake_guard_map(k):
    """the disagreement map the k-th guarded call stores (from 1): luma sad of 16 x 16 tiles with mean difference 0, 2 and 6 codes"""
    m = np.zeros((3, TH, TW), fmm.TILE_DTYPE)
    m["sad"][0] = np.array([[0, 2, 6], [0, 0, 6 if k % 2 else 0]]) * 256
    return m


class _GuardCalc(tqd._DisCalc):
    def guardedBlendEnqueue(self, ts, tile, lo, hi, maps_ptr, outs):
        buf = self._buf_of(maps_ptr)
        off = maps_ptr - buf.ptr
        self._log("guard_enqueue", tile, lo, hi, tuple(ts), off)
        assert off % MAP_BYTES == 0 and off + len(ts) * MAP_BYTES <= buf.nbytes and len(outs) == len(ts) == 1
        self.w.guard_seen.append((self.ring[0][1], self.ring[1][1], self.prev_flow, ts[0]))
        buf.data[off:off + MAP_BYTES] = _fake_guard_map(len(self.w.guard_seen)).reshape(-1).view(np.uint8)
        self.w.mem[outs[0]] = ("guarded", self.ring[0][1], self.ring[1][1], self.prev_flow)


class _GuardWorld(tqd._DisWorld):
    def __init__(self):
        super().__init__()
        self.guard_seen = []

    def calc(self, hdr, H, W, black, white, settings):
        c = _GuardCalc(self, "main" if not self.calcs else "aux")
        c.settings = dict(settings)
        self.calcs.append(c)
        return c


def test_parse_guard_and_its_refusals():
    from hopperrender_amd import quality
    assert quality.parse_guard("16:32:96") == (16, 32, 96) and quality.parse_guard((64, 0, 65535)) == (64, 0, 65535)
    assert quality.parse_guard("32:4080:4081") == (32, 4080, 4081)
    for bad in ("", "16", "16:32", "16:32:96:1", "8:32:96", "48:32:96", "16:96:32", "16:32:32", "16:-1:5", "16:0:65536", "16:a:b", "16:3.5:9", "x:1:2",
                (16, 32), (16, 32, None), "16:32:"):
        with pytest.raises(ValueError):
            quality.parse_guard(bad)


def test_the_command_line_takes_and_refuses(capsys):
    from hopperrender_amd import quality
    a = quality.parse_args(["clip.y4m", "--guard", "16:32:96", "--map-dir", "d"])   # (the mask alone is a reason for --map-dir)
    assert a.guard == (16, 32, 96)
    assert quality.parse_args(["clip.y4m"]).guard is None                           # no default thresholds
    for argv in (["clip.y4m", "--guard", "8:32:96"], ["clip.y4m", "--guard", "16:96:32"], ["clip.y4m", "--guard", "16:32"], ["clip.y4m", "--guard", "16:0:70000"],
                 ["clip.y4m", "--guard"], ["clip.y4m", "--confidence", "--target-fps", "60", "--guard", "16:32:96"]):
        with pytest.raises(SystemExit) as e:
            quality.parse_args(argv)
        assert e.value.code == 2
    assert "--guard" in capsys.readouterr().err


def test_call_order_slots_offsets_and_what_the_report_gains():
    from hopperrender_amd import quality
    w = _GuardWorld()
    rep = quality.evaluate(tq._tagged_frames(9), False, H, W, device=w, guard=(16, 16, 80))
    main = [c[1:] for c in w.log if c[0] == "main"]
    per_pair = ["period", "enqueue", "guard_enqueue", "enqueue"]
    assert [c[0] for c in main] == ["map_shape", "update", "update", "period"] + per_pair * 3 + ["read", "read", "close"]
    gbase = 2 * (quality.PAIRS_PER_READ * 2 // 3)
    assert gbase + quality.PAIRS_PER_READ * 2 // 3 <= 256
    assert [c for c in main if c[0] == "guard_enqueue"] == [("guard_enqueue", 16, 16, 80, (0.5,), k * MAP_BYTES) for k in range(3)]
    assert [c for c in main if c[0] == "enqueue"] == [x for k in range(3) for x in (("enqueue", 2 * k, 2), ("enqueue", gbase + k, 1))]
    assert [c for c in main if c[0] == "read"] == [("read", 0, 6), ("read", gbase, 3)]
    # on the frames and the flow that period's warp used, against the same truth
    warps = [x[0] for x in w.compared[0:6:2]]
    assert [("warp",) + g[:3] for g in w.guard_seen] == warps and all(g[3] == 0.5 for g in w.guard_seen)
    assert [x[0] for x in w.compared[6:]] == [("guarded",) + g[:3] for g in w.guard_seen]
    assert [x[1] for x in w.compared[6:]] == [x[1] for x in w.compared[0:6:2]]
    assert sorted(w.freed) == sorted(b.ptr for b in w.bufs)
    assert rep["guard"] == {"tile": 16, "lo_q4": 16, "hi_q4": 80}
    for k, r in enumerate(rep["pairs"], 1):
        g = r["guarded"]
        assert set(g) == {"Y", "U", "V", "mask"} and set(g["Y"]) == set(r["interpolated"]["Y"])
        assert r["guard_gain_db"] == g["Y"]["psnr"] - r["interpolated"]["Y"]["psnr"]
        # m = 0, 32, 96: tile weights 0, 64, 256
        assert g["mask"]["tiles"] == 6 and g["mask"]["tiles_firing"] == (3 if k % 2 else 2) and 0 < g["mask"]["mean_weight"] < 1
    c = rep["clip"]
    assert set(c["guarded"]) == {"Y", "U", "V", "mask"} and c["guarded"]["mask"]["tiles"] == 18 and c["guarded"]["mask"]["tiles_firing"] == 8
    assert c["guarded"]["Y"]["sse"] == sum(r["guarded"]["Y"]["sse"] for r in rep["pairs"])
    assert c["guard_gain_db"] == c["guarded"]["Y"]["psnr"] - c["interpolated"]["Y"]["psnr"]
    assert json.loads(json.dumps(rep)) == rep
    # the plain blocks are those of a run without the option
    plain = quality.evaluate(tq._tagged_frames(9), False, H, W, device=_GuardWorld())
    del rep["guard"], c["guarded"], c["guard_gain_db"]
    for r in rep["pairs"]:
        del r["guarded"], r["guard_gain_db"]
    assert rep == plain


def test_the_guarded_frame_is_judged_by_every_metric_asked_for():
    from hopperrender_amd import quality
    w = _GuardWorld()
    rep = quality.evaluate(tq._tagged_frames(9), False, H, W, device=w, guard="16:16:80", ssim=True, error_map=16, disagreement=16)
    names = [c[1] for c in w.log if c[0] == "main"]
    first = names.index("guard_enqueue")
    assert names[first - 1] == "map_enqueue" and names[first:first + 4] == ["guard_enqueue", "enqueue", "ssim_enqueue", "map_enqueue"]
    assert names.count("guard_enqueue") == 3
    assert names.count("map_enqueue") == 6 and names.count("dis_enqueue") == 3
    for r in rep["pairs"]:
        g = r["guarded"]
        assert set(g) == {"Y", "U", "V", "mask", "map"} and set(g["Y"]) == set(r["interpolated"]["Y"]) and "ssim" in g["Y"]
        assert "disagreement" not in g and r["guard_gain_ssim"] == g["Y"]["ssim"] - r["interpolated"]["Y"]["ssim"]
    assert "guard_gain_ssim" in rep["clip"] and "ssim" in rep["clip"]["guarded"]["Y"]


def test_chunks_hold_two_thirds_of_the_pairs(monkeypatch):
    from hopperrender_amd import quality
    monkeypatch.setattr(quality, "PAIRS_PER_READ", 3)
    w = _GuardWorld()
    rep = quality.evaluate(tq._tagged_frames(21), False, H, W, device=w, guard=(16, 16, 80))
    reads = [c[2:] for c in w.log if c[:2] == ("main", "read")]
    assert reads == [(0, 4), (4, 2)] * 4 + [(0, 2), (4, 1)] and len(rep["pairs"]) == 9
    assert [c[6] for c in w.log if c[:2] == ("main", "guard_enqueue")] == [0, MAP_BYTES] * 4 + [0]


def test_without_the_option_nothing_new_is_called_and_the_report_is_todays():
    from hopperrender_amd import quality
    w, plain = _GuardWorld(), tq._FakeWorld()
    rep = quality.evaluate(tq._tagged_frames(9), False, 4, 4, device=w)
    assert rep == quality.evaluate(tq._tagged_frames(9), False, 4, 4, device=plain)   # (a calculator without the new method serves)
    assert w.log == plain.log and not w.map_bufs and not w.guard_seen
    assert "guard" not in rep and "guarded" not in rep["clip"] and all("guarded" not in r for r in rep["pairs"])
    for bad in ((8, 1, 2), (16, 5, 5), (16, 0, 65536), "16:1"):
        with pytest.raises(ValueError):
            quality.evaluate(tq._tagged_frames(9), False, H, W, device=_GuardWorld(), guard=bad)


def test_the_mask_is_written_per_pair_at_luma_resolution(tmp_path):
    from hopperrender_amd import quality
    from hopperrender_amd.calc import guard_weights
    quality.evaluate(tq._tagged_frames(9), False, H, W, device=_GuardWorld(), guard=(16, 16, 80), map_dir=str(tmp_path / "maps"))
    files = sorted(os.listdir(tmp_path / "maps"))
    assert files == ["guard_pair0001.pgm", "guard_pair0002.pgm", "guard_pair0003.pgm"]
    for k, name in enumerate(files, 1):
        raw = open(tmp_path / "maps" / name, "rb").read()
        head = b"P5\n%d %d\n255\n" % (W, H)
        assert raw.startswith(head) and len(raw) == len(head) + H * W
        _, w = guard_weights(_fake_guard_map(k)[None], 16, 16, 80, H, W, False)
        assert np.array_equal(np.frombuffer(raw[len(head):], np.uint8).reshape(H, W), np.minimum(w[0], 255))
        assert w.max() == 256 and w.min() == 0
