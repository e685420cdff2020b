"""CPU: the evaluator's error-map option without a GPU -- what it calls on the clip's context (a recording fake in the style of
tests/test_quality.py), that one map per evaluated pair goes out and the buffer is read once per chunk, what the report gains, that it
gains nothing and calls nothing when the option is off -- and the ordering of the worst tiles and the share figure on hand-made maps."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frame_error_map_model as fmm  # noqa: E402
import test_quality as tq  # noqa: E402
import test_quality_ssim as tqs  # noqa: E402

TW, TH = 3, 2            # what the fake context reports for any tile; 288 bytes a map
MAP_BYTES = 48 * TW * TH


def _fake_map(k):
    """the k-th map enqueued (from 1): Y has two pairs of equal tiles, U is equal everywhere, V differs in its last tile alone"""
    m = np.zeros((3, TH, TW), fmm.TILE_DTYPE)
    m["sse"][0] = np.array([[5, 9, 0], [9, 1, 5]]) * k
    m["max_abs"][0] = [[2, 3, 0], [3, 1, 2]]
    m["sad"][0] = m["sse"][0] // 2
    m[2, 1, 2] = (7, 7, 1)
    return m


class _MapBuf(tq._FakeBuf):
    def __init__(self, world, nbytes):
        super().__init__(world)
        self.nbytes, self.data = nbytes, np.full(nbytes, 0xFF, np.uint8)

    def download(self, dtype, count):
        assert np.dtype(dtype) == np.uint8 and count <= self.nbytes
        self.world.log.append(("maps", "download", count))
        return self.data[:count].copy()


class _MapCalc(tqs._SsimCalc):
    def frameErrorMapShape(self, tile):
        self._log("map_shape", tile)
        return TW, TH, MAP_BYTES

    def frameErrorMapEnqueue(self, a, b, tile, maps_ptr):
        buf = self.w.map_bufs[-1]
        off = maps_ptr - buf.ptr
        self._log("map_enqueue", tile, len(a), off)
        assert 0 <= off and off + len(a) * MAP_BYTES <= buf.nbytes and off % MAP_BYTES == 0
        for x, y in zip(a, b):
            self.w.map_compared.append((self.w.mem[x], self.w.mem[y]))
            buf.data[off:off + MAP_BYTES] = _fake_map(len(self.w.map_compared)).reshape(-1).view(np.uint8)
            off += MAP_BYTES


class _MapWorld(tqs._SsimWorld):
    def __init__(self):
        super().__init__()
        self.map_bufs, self.map_compared = [], []

    def calc(self, hdr, H, W, black, white, settings):
        c = _MapCalc(self, "main" if not self.calcs else "aux")
        c.settings = dict(settings)
        self.calcs.append(c)
        return c

    def buffer(self, nbytes):
        if nbytes == 24:
            return tq._FakeBuf(self)
        self.map_bufs.append(_MapBuf(self, nbytes))
        return self.map_bufs[-1]


def test_one_map_per_evaluated_pair_read_once_and_what_the_report_gains():
    from hopperrender_amd import quality
    w = _MapWorld()
    rep = quality.evaluate(tq._tagged_frames(9), False, 4, 4, device=w, error_map=16)
    main = [c[1:] for c in w.log if c[0] == "main"]
    assert [c[0] for c in main] == ["map_shape", "update", "update", "period", "period", "enqueue", "map_enqueue", "period", "enqueue", "map_enqueue",
                                    "period", "enqueue", "map_enqueue", "read", "close"]
    # one map each, of the interpolation against the truth (the first comparison of each pair), side by side in ONE buffer
    assert [c for c in main if c[0] == "map_enqueue"] == [("map_enqueue", 16, 1, 0), ("map_enqueue", 16, 1, MAP_BYTES), ("map_enqueue", 16, 1, 2 * MAP_BYTES)]
    assert w.map_compared == w.compared[0::2] and len(w.map_bufs) == 1 and w.map_bufs[0].nbytes == 3 * MAP_BYTES
    # ... which is read once, behind the read of the sums that waits for the context
    assert [c for c in w.log if c[0] == "maps"] == [("maps", "download", 3 * MAP_BYTES)]
    assert w.log.index(("maps", "download", 3 * MAP_BYTES)) == w.log.index(("main", "read", 0, 6)) + 1
    assert sorted(w.freed) == sorted(b.ptr for b in w.bufs)
    for k, r in enumerate(rep["pairs"], 1):
        m = r["interpolated"]["map"]
        assert set(m) == {"tile", "shape", "Y", "U", "V"} and m["tile"] == 16 and m["shape"] == [TH, TW]
        assert m["Y"]["worst"] == [{"x": 16, "y": 0, "sse": 9 * k, "max_abs": 3}, {"x": 0, "y": 16, "sse": 9 * k, "max_abs": 3},
                                   {"x": 0, "y": 0, "sse": 5 * k, "max_abs": 2}, {"x": 32, "y": 16, "sse": 5 * k, "max_abs": 2},
                                   {"x": 16, "y": 16, "sse": k, "max_abs": 1}]
        assert m["Y"]["share_top1pct"] == 9 / 29
        assert m["U"]["share_top1pct"] is None and [t["sse"] for t in m["U"]["worst"]] == [0] * 5
        assert [(t["x"], t["y"]) for t in m["U"]["worst"]] == [(0, 0), (16, 0), (32, 0), (0, 16), (16, 16)]
        assert m["V"]["worst"][0] == {"x": 32, "y": 16, "sse": 7, "max_abs": 1} and m["V"]["share_top1pct"] == 1.0
        for i, p in enumerate("YUV"):   # the model of the GPU tests reads the same maps the same way
            assert m[p] == {"worst": fmm.worst_tiles(_fake_map(k)[i], 16), "share_top1pct": fmm.share_top1pct(_fake_map(k)[i])}
        assert "map" not in r["repeat"]
    assert rep["clip"]["worst_tile"] == {"pair": 3, "plane": "Y", "x": 16, "y": 0, "sse": 27}
    assert json.loads(json.dumps(rep)) == rep
    # the rest of the report is the run without the option
    plain = quality.evaluate(tq._tagged_frames(9), False, 4, 4, device=tq._FakeWorld())
    del rep["clip"]["worst_tile"]
    for r in rep["pairs"]:
        del r["interpolated"]["map"]
    assert rep == plain


def test_maps_are_read_once_per_chunk_into_the_same_buffer(monkeypatch):
    from hopperrender_amd import quality
    monkeypatch.setattr(quality, "PAIRS_PER_READ", 2)
    w = _MapWorld()
    rep = quality.evaluate(tq._tagged_frames(21), False, 4, 4, device=w, error_map=64)
    names = [c[1] for c in w.log if c[0] == "main"]
    assert names.count("enqueue") == names.count("map_enqueue") == 9 and names.count("read") == 5
    assert [c[2] for c in w.log if c[0] == "maps"] == [2 * MAP_BYTES] * 4 + [MAP_BYTES]
    assert all(w.log[i + 1][0] == "maps" for i, c in enumerate(w.log) if c[:2] == ("main", "read"))
    assert [c[4] for c in w.log if c[:2] == ("main", "map_enqueue")] == [0, MAP_BYTES] * 4 + [0]
    assert len(w.map_bufs) == 1 and w.map_bufs[0].nbytes == 2 * MAP_BYTES
    assert w.map_compared == w.compared[0::2] and len(rep["pairs"]) == 9
    assert [r["interpolated"]["map"]["Y"]["worst"][0]["sse"] for r in rep["pairs"]] == [9 * k for k in range(1, 10)]
    assert rep["clip"]["worst_tile"]["pair"] == 9 and rep["clip"]["worst_tile"]["sse"] == 81


def test_beside_ssim_the_map_follows_both_judges():
    from hopperrender_amd import quality
    w = _MapWorld()
    rep = quality.evaluate(tq._tagged_frames(9), False, 4, 4, device=w, ssim=True, error_map=32)
    names = [c[1] for c in w.log if c[0] == "main"]
    assert names[names.index("enqueue"):][:3] == ["enqueue", "ssim_enqueue", "map_enqueue"]
    assert names[-4:] == ["map_enqueue", "read", "ssim_read", "close"]
    assert rep["pairs"][0]["interpolated"]["map"]["tile"] == 32 and "ssim" in rep["pairs"][0]["interpolated"]["Y"]
    assert rep["clip"]["worst_tile"]["x"] == 32   # (tile 1 across, at 32 luma pixels a tile)


def test_without_the_option_nothing_new_is_called_and_the_report_is_todays():
    from hopperrender_amd import quality
    w, plain = _MapWorld(), tq._FakeWorld()
    rep = quality.evaluate(tq._tagged_frames(9), False, 4, 4, device=w)
    assert rep == quality.evaluate(tq._tagged_frames(9), False, 4, 4, device=plain)   # (a calculator without map methods serves)
    assert rep == quality.evaluate(tq._tagged_frames(9), False, 4, 4, device=_MapWorld(), error_map=0)
    assert w.log == plain.log and not w.map_bufs and not w.map_compared
    assert "worst_tile" not in rep["clip"] and all("map" not in r["interpolated"] for r in rep["pairs"])
    for bad in (8, 48, 128, -16):
        with pytest.raises(ValueError):
            quality.evaluate(tq._tagged_frames(9), False, 4, 4, device=_MapWorld(), error_map=bad)
    with pytest.raises(ValueError):
        quality.evaluate(tq._tagged_frames(9), False, 4, 4, device=_MapWorld(), map_dir="somewhere")


def test_worst_ordering_and_share_on_hand_made_maps():
    """Ties go to the lower y, then the lower x; k tiles at the most; the share is that of the ceil(tiles / 100) worst tiles."""
    from hopperrender_amd import quality
    m = np.zeros((3, 4), fmm.TILE_DTYPE)
    m["sse"] = [[4, 8, 8, 0], [8, 2, 4, 1 << 43], [0, 0, 8, 4]]
    m["max_abs"] = np.arange(12).reshape(3, 4)
    got = quality._worst_tiles(m, 64)
    assert [(t["y"] // 64, t["x"] // 64, t["sse"]) for t in got] == [(1, 3, 1 << 43), (0, 1, 8), (0, 2, 8), (1, 0, 8), (2, 2, 8)]
    assert [t["max_abs"] for t in got] == [7, 1, 2, 4, 10] and all(type(v) is int for t in got for v in t.values())
    assert got == fmm.worst_tiles(m, 64)
    assert len(quality._worst_tiles(m[:1, :3], 16)) == 3
    assert quality._share_top1pct(m) == (1 << 43) / ((1 << 43) + 46) == fmm.share_top1pct(m)
    assert quality._share_top1pct(np.zeros((3, 4), fmm.TILE_DTYPE)) is None
    flat = np.zeros((10, 15), fmm.TILE_DTYPE)   # 150 tiles: the two worst of them
    flat["sse"] = 1
    assert quality._share_top1pct(flat) == 2 / 150
    flat["sse"][3, 4], flat["sse"][9, 14] = 100, 50
    assert quality._share_top1pct(flat) == 150 / 298 == fmm.share_top1pct(flat)
    flat["sse"] = 0
    flat["sse"][0, 0] = 3
    assert quality._share_top1pct(flat) == 1.0


def test_heat_maps_are_written_per_pair_scaled_to_the_clip(tmp_path):
    """One PGM per evaluated pair: TW x TH pixels, sqrt(sse / count) of the Y tiles with count the tile's elements inside the frame, the
    clip's largest value at 255."""
    from hopperrender_amd import quality
    quality.evaluate(tq._tagged_frames(9), False, 40, 34, device=_MapWorld(), error_map=16, map_dir=str(tmp_path / "maps"))
    files = sorted(os.listdir(tmp_path / "maps"))
    assert files == ["map_pair0001.pgm", "map_pair0002.pgm", "map_pair0003.pgm"]
    # 34 x 40: tile columns 16, 16, 2 wide and rows 16, 16, 8 high -- the fake reports 3 x 2 tiles whatever the geometry, rows 16, 16
    counts = np.outer([16, 16], [16, 16, 2]).astype(np.float64)
    rms = [np.sqrt(_fake_map(k)["sse"][0] / counts) for k in (1, 2, 3)]
    top = max(r.max() for r in rms)
    for k, name in enumerate(files):
        raw = open(tmp_path / "maps" / name, "rb").read()
        assert raw.startswith(b"P5\n3 2\n255\n") and len(raw) == 11 + 6
        assert list(raw[11:]) == np.rint(rms[k] * 255.0 / top).astype(np.uint8).reshape(-1).tolist()
    assert max(open(tmp_path / "maps" / files[2], "rb").read()[11:]) == 255
