"""CPU: the evaluator's SSIM-map option without a GPU -- what it calls on the clip's context (a recording fake in the style of
tests/test_quality_map.py), that one map per evaluated pair goes out behind its error launch and the buffer is read once per chunk, what
the report gains, that it gains nothing and calls nothing when the option is off -- and the ranking of the worst tiles, the join with
the error map and the heat-map bytes on hand-made maps."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frame_ssim_map_model as smm  # noqa: E402
import test_quality as tq  # noqa: E402
import test_quality_map as tqm  # noqa: E402

TW, TH = tqm.TW, tqm.TH  # 3 x 2 tiles, what the fake context reports for any tile
SMAP_BYTES = 72 * TW * TH
ONE = 1 << 32


def _fake_smap(k):
    """the k-th SSIM map enqueued (from 1).  Y: four tiles of equal mean 3 s from different counts (6 / 2, 3 / 1, 3 / 1, 9 / 3), one
    without a window, and one whose mean loss, 1.25, is the same in every map and beyond the heat map's scale.  U: two equal tiles.
    V: no window at all."""
    s = k << 26
    m = np.zeros((3, TH, TW), smm.TILE_DTYPE)
    m["count"][0] = [[2, 1, 0], [1, 3, 4]]
    m["sum_loss_q32"][0] = [[6 * s, 3 * s, 0], [3 * s, 9 * s, 5 * ONE]]
    m["max_loss_q32"][0] = [[4 * s, 3 * s, 0], [3 * s, 4 * s, 2 * ONE]]
    m["count"][1] = [[1, 0, 1], [0, 0, 0]]
    m["sum_loss_q32"][1] = m["max_loss_q32"][1] = [[s, 0, s], [0, 0, 0]]
    return m


class _SmapCalc(tqm._MapCalc):
    def _buf_at(self, ptr):
        return max((b for b in self.w.map_bufs if b.ptr <= ptr), key=lambda b: b.ptr)

    def frameErrorMapEnqueue(self, a, b, tile, maps_ptr):   # (the fake of test_quality_map with the buffer found by its address)
        buf = self._buf_at(maps_ptr)
        off = maps_ptr - buf.ptr
        self._log("map_enqueue", tile, len(a), off)
        assert buf is self.w.map_bufs[0] and off + len(a) * tqm.MAP_BYTES <= buf.nbytes and off % tqm.MAP_BYTES == 0
        for x, y in zip(a, b):
            self.w.map_compared.append((self.w.mem[x], self.w.mem[y]))
            buf.data[off:off + tqm.MAP_BYTES] = tqm._fake_map(len(self.w.map_compared)).reshape(-1).view(np.uint8)
            off += tqm.MAP_BYTES

    def frameSsimMapShape(self, tile):
        self._log("smap_shape", tile)
        return TW, TH, SMAP_BYTES

    def frameSsimMapEnqueue(self, a, b, tile, maps_ptr):
        buf = self._buf_at(maps_ptr)
        off = maps_ptr - buf.ptr
        self._log("smap_enqueue", tile, len(a), off)
        assert buf is self.w.map_bufs[-1] and off + len(a) * SMAP_BYTES <= buf.nbytes and off % SMAP_BYTES == 0
        for x, y in zip(a, b):
            self.w.smap_compared.append((self.w.mem[x], self.w.mem[y]))
            buf.data[off:off + SMAP_BYTES] = _fake_smap(len(self.w.smap_compared)).reshape(-1).view(np.uint8)
            off += SMAP_BYTES


class _SmapWorld(tqm._MapWorld):
    def __init__(self):
        super().__init__()
        self.smap_compared = []

    def calc(self, hdr, H, W, black, white, settings):
        c = _SmapCalc(self, "main" if not self.calcs else "aux")
        c.settings = dict(settings)
        self.calcs.append(c)
        return c


def _entry(x, y, total, worst, count, **more):
    return dict({"x": x, "y": y, "ssim": 1.0 - total / 4294967296.0 / count, "min_ssim": 1.0 - worst / 4294967296.0,
                 "sum_loss_q32": total, "max_loss_q32": worst, "count": count}, **more)


def test_one_map_per_evaluated_pair_read_once_and_what_the_report_gains():
    from hopperrender_amd import quality
    w = _SmapWorld()
    rep = quality.evaluate(tq._tagged_frames(9), False, 4, 4, device=w, ssim_map=16)
    main = [c[1:] for c in w.log if c[0] == "main"]
    assert [c[0] for c in main] == ["smap_shape", "update", "update", "period", "period", "enqueue", "smap_enqueue", "period", "enqueue", "smap_enqueue",
                                    "period", "enqueue", "smap_enqueue", "read", "close"]
    # one map each, of the interpolation against the truth (the first comparison of each pair), side by side in ONE buffer
    assert [c for c in main if c[0] == "smap_enqueue"] == [("smap_enqueue", 16, 1, 0), ("smap_enqueue", 16, 1, SMAP_BYTES), ("smap_enqueue", 16, 1, 2 * SMAP_BYTES)]
    assert w.smap_compared == w.compared[0::2] and len(w.map_bufs) == 1 and w.map_bufs[0].nbytes == 3 * SMAP_BYTES
    # ... which is read once, behind the read of the sums that waits for the context
    assert [c for c in w.log if c[0] == "maps"] == [("maps", "download", 3 * SMAP_BYTES)]
    assert w.log.index(("maps", "download", 3 * SMAP_BYTES)) == w.log.index(("main", "read", 0, 6)) + 1
    assert sorted(w.freed) == sorted(b.ptr for b in w.bufs)
    for k, r in enumerate(rep["pairs"], 1):
        s = k << 26
        m = r["interpolated"]["ssim_map"]
        assert set(m) == {"tile", "shape", "Y", "U", "V"} and m["tile"] == 16 and m["shape"] == [TH, TW]
        assert all(set(m[p]) == {"worst", "worst_window_tile"} for p in "YUV")
        # the largest mean first; the four equal means in the order y, then x, whatever their counts; the tile without a window left out
        assert m["Y"]["worst"] == [_entry(32, 16, 5 * ONE, 2 * ONE, 4), _entry(0, 0, 6 * s, 4 * s, 2), _entry(16, 0, 3 * s, 3 * s, 1),
                                   _entry(0, 16, 3 * s, 3 * s, 1), _entry(16, 16, 9 * s, 4 * s, 3)]
        assert m["Y"]["worst"][0]["ssim"] == -0.25 and m["Y"]["worst"][0]["min_ssim"] == -1.0
        assert m["Y"]["worst_window_tile"] == {"x": 32, "y": 16, "max_loss_q32": 2 * ONE}
        assert m["U"]["worst"] == [_entry(0, 0, s, s, 1), _entry(32, 0, s, s, 1)] and m["U"]["worst_window_tile"] == {"x": 0, "y": 0, "max_loss_q32": s}
        assert m["V"] == {"worst": [], "worst_window_tile": None}
        for i, p in enumerate("YUV"):   # the model of the GPU tests reads the same maps the same way
            assert m[p] == {"worst": smm.worst_tiles(_fake_smap(k)[i], 16), "worst_window_tile": smm.worst_window_tile(_fake_smap(k)[i], 16)}
        assert all(type(v) is int for t in m["Y"]["worst"] for f, v in t.items() if f not in ("ssim", "min_ssim"))
        assert "ssim_map" not in r["repeat"] and "map" not in r["interpolated"]
    # every pair's worst luma tile has the same mean: the earlier pair is named
    assert rep["clip"]["worst_tile_ssim"] == {"pair": 1, "plane": "Y", "x": 32, "y": 16, "ssim": -0.25}
    assert json.loads(json.dumps(rep)) == rep
    # the rest of the report is the run without the option
    plain = quality.evaluate(tq._tagged_frames(9), False, 4, 4, device=tq._FakeWorld())
    del rep["clip"]["worst_tile_ssim"]
    for r in rep["pairs"]:
        del r["interpolated"]["ssim_map"]
    assert rep == plain


def test_maps_are_read_once_per_chunk_into_the_same_buffer(monkeypatch):
    """21 frames at two pairs a read: five chunks, the last of one pair."""
    from hopperrender_amd import quality
    monkeypatch.setattr(quality, "PAIRS_PER_READ", 2)
    w = _SmapWorld()
    rep = quality.evaluate(tq._tagged_frames(21), False, 4, 4, device=w, ssim_map=64)
    names = [c[1] for c in w.log if c[0] == "main"]
    assert names.count("enqueue") == names.count("smap_enqueue") == 9 and names.count("read") == 5
    assert all(names[i + 1] == "smap_enqueue" for i, n in enumerate(names) if n == "enqueue")
    assert [c[2] for c in w.log if c[0] == "maps"] == [2 * SMAP_BYTES] * 4 + [SMAP_BYTES]
    assert all(w.log[i + 1][0] == "maps" for i, c in enumerate(w.log) if c[:2] == ("main", "read"))
    assert [c[4] for c in w.log if c[:2] == ("main", "smap_enqueue")] == [0, SMAP_BYTES] * 4 + [0]
    assert len(w.map_bufs) == 1 and w.map_bufs[0].nbytes == 2 * SMAP_BYTES
    assert w.smap_compared == w.compared[0::2] and len(rep["pairs"]) == 9
    assert [r["interpolated"]["ssim_map"]["Y"]["worst"][1]["sum_loss_q32"] for r in rep["pairs"]] == [6 * (k << 26) for k in range(1, 10)]
    assert rep["clip"]["worst_tile_ssim"]["pair"] == 1 and rep["pairs"][0]["interpolated"]["ssim_map"]["tile"] == 64


def test_more_pairs_than_one_read_takes():
    """263 frames are 130 evaluated pairs: a chunk of 128 and one of 2, each read once from the one buffer of 128 maps."""
    from hopperrender_amd import quality
    w = _SmapWorld()
    rep = quality.evaluate([np.full(24, k, np.uint16) for k in range(263)], False, 4, 4, device=w, ssim_map=32)
    assert len(rep["pairs"]) == 130 and len(w.map_bufs) == 1 and w.map_bufs[0].nbytes == 128 * SMAP_BYTES
    assert [c[2] for c in w.log if c[0] == "maps"] == [128 * SMAP_BYTES, 2 * SMAP_BYTES]
    assert [c[4] for c in w.log if c[:2] == ("main", "smap_enqueue")] == [i * SMAP_BYTES for i in range(128)] + [0, SMAP_BYTES]
    assert [c for c in w.log if c[:2] == ("main", "read")] == [("main", "read", 0, 256), ("main", "read", 0, 4)]
    assert w.smap_compared == w.compared[0::2]
    assert [r["interpolated"]["ssim_map"]["U"]["worst"][0]["sum_loss_q32"] for r in rep["pairs"]] == [k << 26 for k in range(1, 131)]


def test_beside_the_error_map_the_worst_tiles_carry_their_squared_error():
    """error_map at the same tile size: every worst entry gains "sse", the same tile's entry of the error map; at another size none
    does.  Either way each map goes into its own buffer and is read once."""
    from hopperrender_amd import quality
    w = _SmapWorld()
    rep = quality.evaluate(tq._tagged_frames(9), False, 4, 4, device=w, ssim=True, error_map=16, ssim_map=16)
    names = [c[1] for c in w.log if c[0] == "main"]
    assert names[:2] == ["map_shape", "smap_shape"]
    assert names[names.index("enqueue"):][:4] == ["enqueue", "ssim_enqueue", "map_enqueue", "smap_enqueue"]
    assert names[-5:] == ["map_enqueue", "smap_enqueue", "read", "ssim_read", "close"]
    assert [c for c in w.log if c[0] == "maps"] == [("maps", "download", 3 * tqm.MAP_BYTES), ("maps", "download", 3 * SMAP_BYTES)]
    assert [b.nbytes for b in w.map_bufs] == [3 * tqm.MAP_BYTES, 3 * SMAP_BYTES]
    for k, r in enumerate(rep["pairs"], 1):
        err = tqm._fake_map(k)
        worst = r["interpolated"]["ssim_map"]["Y"]["worst"]
        assert [(t["x"], t["y"], t["sse"]) for t in worst] == [(32, 16, 5 * k), (0, 0, 5 * k), (16, 0, 9 * k), (0, 16, 9 * k), (16, 16, k)]
        assert [t["sse"] for t in r["interpolated"]["ssim_map"]["U"]["worst"]] == [0, 0]
        assert worst == smm.worst_tiles(_fake_smap(k)[0], 16, err[0]["sse"])
        assert r["interpolated"]["map"]["Y"]["worst"][0]["sse"] == 9 * k and "ssim" in r["interpolated"]["Y"]
    assert rep["clip"]["worst_tile"]["sse"] == 27 and rep["clip"]["worst_tile_ssim"]["pair"] == 1
    other = quality.evaluate(tq._tagged_frames(9), False, 4, 4, device=_SmapWorld(), error_map=32, ssim_map=16)
    assert all("sse" not in t for r in other["pairs"] for p in "YUV" for t in r["interpolated"]["ssim_map"][p]["worst"])
    assert other["pairs"][0]["interpolated"]["map"]["tile"] == 32 and other["pairs"][0]["interpolated"]["ssim_map"]["tile"] == 16
    del rep["clip"]["worst_tile_ssim"]
    for r in rep["pairs"]:
        del r["interpolated"]["ssim_map"]
    assert rep == quality.evaluate(tq._tagged_frames(9), False, 4, 4, device=tqm._MapWorld(), ssim=True, error_map=16)


def test_without_the_option_nothing_new_is_called_and_the_report_is_todays():
    from hopperrender_amd import quality
    w, plain = _SmapWorld(), tq._FakeWorld()
    rep = quality.evaluate(tq._tagged_frames(9), False, 4, 4, device=w)
    assert rep == quality.evaluate(tq._tagged_frames(9), False, 4, 4, device=plain)   # (a calculator without SSIM-map methods serves)
    assert rep == quality.evaluate(tq._tagged_frames(9), False, 4, 4, device=_SmapWorld(), ssim_map=0)
    assert w.log == plain.log and not w.map_bufs and not w.smap_compared
    assert "worst_tile_ssim" not in rep["clip"] and all("ssim_map" not in r["interpolated"] for r in rep["pairs"])
    both = quality.evaluate(tq._tagged_frames(9), False, 4, 4, device=tqm._MapWorld(), ssim=True, error_map=32)   # a fake without the new methods
    assert "worst_tile_ssim" not in both["clip"]
    for bad in (8, 48, 128, -16, True, 16.5, "16"):
        with pytest.raises(ValueError):
            quality.evaluate(tq._tagged_frames(9), False, 4, 4, device=_SmapWorld(), ssim_map=bad)
    with pytest.raises(ValueError):
        quality.evaluate(tq._tagged_frames(9), False, 4, 4, device=_SmapWorld(), map_dir="somewhere")
    a = quality.parse_args(["clip.y4m", "--ssim-map", "32", "--map-dir", "out"])
    assert a.ssim_map == 32 and a.map == 0 and a.map_dir == "out" and quality.parse_args(["clip.y4m"]).ssim_map == 0
    for argv in (["clip.y4m", "--ssim-map", "24"], ["clip.y4m", "--map-dir", "out"]):
        with pytest.raises(SystemExit):
            quality.parse_args(argv)


def test_ranking_on_hand_made_maps():
    """Largest sum / count first, compared as integers: (3 2^60 + 1) / 3 is above 2^60 / 1 by a third, which no double holds.  Ties go to
    the lower y, then the lower x; tiles without a window are left out; k tiles at the most."""
    from hopperrender_amd import quality
    m = np.zeros((3, 4), smm.TILE_DTYPE)
    big = 1 << 60
    m["sum_loss_q32"] = [[big, 8, 6, 0], [3, 9, 3 * big + 1, 12], [0, 6, 2 * big, 7]]
    m["count"] = [[1, 4, 2, 0], [1, 3, 3, 4], [5, 2, 2, 0]]
    m["max_loss_q32"] = [[5, 2, 9, 0], [3, 9, 4, 9], [0, 1, 2, 0]]
    assert float(3 * big + 1) / 3 == float(big) == float(2 * big) / 2
    got = quality._worst_ssim_tiles(m, 64, k=12)
    assert [(t["y"] // 64, t["x"] // 64) for t in got] == [(1, 2), (0, 0), (2, 2), (0, 2), (1, 0), (1, 1), (1, 3), (2, 1), (0, 1), (2, 0)]
    assert got == smm.worst_tiles(m, 64, k=12) and len(quality._worst_ssim_tiles(m, 64)) == 5
    assert got[3] == {"x": 128, "y": 0, "ssim": 1.0 - 3 / ONE, "min_ssim": 1.0 - 9 / ONE, "sum_loss_q32": 6, "max_loss_q32": 9, "count": 2}
    assert got[-1]["count"] == 5 and got[-1]["sum_loss_q32"] == 0 and got[-1]["ssim"] == 1.0
    # the worst window: the largest max_loss_q32 among tiles that own a window, the first of equals in the order y, then x
    assert quality._worst_window_tile(m, 64) == {"x": 128, "y": 0, "max_loss_q32": 9} == smm.worst_window_tile(m, 64)
    assert quality._worst_window_tile(np.zeros((2, 2), smm.TILE_DTYPE), 16) is None and quality._worst_ssim_tiles(np.zeros((2, 2), smm.TILE_DTYPE), 16) == []
    sse = np.arange(12).reshape(3, 4)
    joined = quality._worst_ssim_tiles(m, 64, {"sse": sse})
    assert [t["sse"] for t in joined] == [6, 0, 10, 2, 4] and joined == smm.worst_tiles(m, 64, sse)


def test_heat_maps_are_written_per_pair_on_an_absolute_scale(tmp_path):
    """One PGM per evaluated pair: TW x TH pixels, round(255 min(1, sum / count / 2^32)) of the Y tiles, 0 without a window; with both
    maps on, both kinds of file."""
    from hopperrender_amd import quality
    quality.evaluate(tq._tagged_frames(9), False, 40, 34, device=_SmapWorld(), ssim_map=16, map_dir=str(tmp_path / "maps"))
    files = sorted(os.listdir(tmp_path / "maps"))
    assert files == ["ssim_pair0001.pgm", "ssim_pair0002.pgm", "ssim_pair0003.pgm"]
    for k, name in enumerate(files, 1):
        raw = open(tmp_path / "maps" / name, "rb").read()
        assert raw.startswith(b"P5\n3 2\n255\n") and len(raw) == 11 + 6
        mean = [3 * k / 64, 3 * k / 64, None, 3 * k / 64, 3 * k / 64, 1.25]   # sum / count / 2^32 with s = k 2^26
        assert list(raw[11:]) == [0 if v is None else int(round(255.0 * min(1.0, v))) for v in mean] == smm.pgm_values(_fake_smap(k)[0])
        assert raw[11 + 2] == 0 and raw[-1] == 255
    assert list(open(tmp_path / "maps" / files[0], "rb").read()[11:]) == [12, 12, 0, 12, 12, 255]
    quality.evaluate(tq._tagged_frames(9), False, 40, 34, device=_SmapWorld(), ssim_map=16, error_map=16, map_dir=str(tmp_path / "both"))
    assert sorted(os.listdir(tmp_path / "both")) == [f"{kind}_pair000{k}.pgm" for kind in ("map", "ssim") for k in (1, 2, 3)]
