"""CPU: the evaluator's disagreement option and the confidence run without a GPU, against a recording fake device in the style of
tests/test_quality_map.py -- what is called on the clip's context and in which order, the buffer offsets, what the report gains (and
that it gains nothing and calls nothing when the option is off), overlap_top1pct on hand-made maps, ties included, and the schedule,
gating and chunking of confidence()."""
import json
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frame_error_map_model as fmm  # noqa: E402
import test_quality as tq  # noqa: E402
import test_quality_map as tqm  # noqa: E402

TW, TH, MAP_BYTES = tqm.TW, tqm.TH, tqm.MAP_BYTES


def _fake_dis(k):
    """the k-th disagreement map enqueued (from 1).  Y: its worst tile is the error map's worst, (1, 0) in tiles x, y, for odd k and
    another one for even k; U disagrees a little where the error map is zero everywhere; V disagrees most in the error map's one tile"""
    m = np.zeros((3, TH, TW), fmm.TILE_DTYPE)
    m["sse"][0] = [[1, 8, 0], [8, 2, 3]] if k % 2 else [[1, 2, 0], [8, 2, 3]]
    m["sad"][0] = m["sse"][0]
    m["max_abs"][0] = [[1, 2, 0], [2, 1, 1]]
    m[1, 0, 0] = (4, 2, 2)
    m[2, 1, 2] = (5 * k, 5, 3)
    m[2, 0, 1] = (1, 1, 1)
    return m


class _DisCalc(tqm._MapCalc):
    prev_flow = None

    def _buf_of(self, ptr):
        return next(b for b in self.w.map_bufs if b.ptr <= ptr < b.ptr + b.nbytes)

    def interpolatePeriod(self, ptr, ts, outs, mode):
        self.prev_flow = self.flow
        if len(ts):
            return super().interpolatePeriod(ptr, ts, outs, mode)
        self._log("period", self.w.mem[ptr][1]); self._push(ptr)     # no outputs: update and flow only
        assert self.m_frameCount >= 3 and mode == 2 and not len(outs)
        self.flow = (self.ring[1][1], self.ring[2][1])

    def frameErrorMapEnqueue(self, a, b, tile, maps_ptr):             # (the buffer the pointer lies in, not the newest one)
        self.w.map_bufs.append(self.w.map_bufs.pop(self.w.map_bufs.index(self._buf_of(maps_ptr))))
        super().frameErrorMapEnqueue(a, b, tile, maps_ptr)

    def warpDisagreementMapEnqueue(self, ts, tile, maps_ptr):
        buf = self._buf_of(maps_ptr)
        off = maps_ptr - buf.ptr
        self._log("dis_enqueue", tile, tuple(ts), off)
        assert off % MAP_BYTES == 0 and off + len(ts) * MAP_BYTES <= buf.nbytes and 1 <= len(ts) <= 24
        for t in ts:   # what warpFrames would read now: frames N-2, N-1 and the PREVIOUS flow
            self.w.dis_seen.append((self.ring[0][1], self.ring[1][1], self.prev_flow, t))
            buf.data[off:off + MAP_BYTES] = _fake_dis(len(self.w.dis_seen)).reshape(-1).view(np.uint8)
            off += MAP_BYTES


class _DisWorld(tqm._MapWorld):
    def __init__(self):
        super().__init__()
        self.dis_seen = []

    def calc(self, hdr, H, W, black, white, settings):
        c = _DisCalc(self, "main" if not self.calcs else "aux")
        c.settings = dict(settings)
        self.calcs.append(c)
        return c


def test_call_order_offsets_and_what_the_report_gains():
    from hopperrender_amd import quality
    w = _DisWorld()
    rep = quality.evaluate(tq._tagged_frames(9), False, 4, 4, device=w, error_map=16, disagreement=16)
    main = [c[1:] for c in w.log if c[0] == "main"]
    # straight behind each evaluated pair's period, ahead of everything else of the pair and of the next period
    assert [c[0] for c in main] == ["map_shape", "map_shape", "update", "update", "period", "period", "dis_enqueue", "enqueue", "map_enqueue",
                                    "period", "dis_enqueue", "enqueue", "map_enqueue", "period", "dis_enqueue", "enqueue", "map_enqueue", "read", "close"]
    assert [c for c in main if c[0] == "dis_enqueue"] == [("dis_enqueue", 16, (0.5,), k * MAP_BYTES) for k in range(3)]
    # ... on the frames and the flow that period's warp used
    assert [(("warp",) + d[:3]) for d in w.dis_seen] == [x[0] for x in w.compared[0::2]] == [x[0] for x in w.map_compared] and all(d[3] == 0.5 for d in w.dis_seen)
    # a buffer of its own, read once, behind the read of the sums that waits for the context
    assert len(w.map_bufs) == 2 and [b.nbytes for b in w.map_bufs] == [3 * MAP_BYTES] * 2
    assert [c for c in w.log if c[0] == "maps"] == [("maps", "download", 3 * MAP_BYTES)] * 2
    assert w.log.index(("main", "read", 0, 6)) < w.log.index(("maps", "download", 3 * MAP_BYTES))
    assert sorted(w.freed) == sorted(b.ptr for b in w.bufs)
    for k, r in enumerate(rep["pairs"], 1):
        d = r["interpolated"]["disagreement"]
        assert set(d) == {"tile", "shape", "Y", "U", "V"} and d["tile"] == 16 and d["shape"] == [TH, TW]
        for i, p in enumerate("YUV"):
            m = _fake_dis(k)[i]
            assert set(d[p]) == {"worst", "share_top1pct", "sse", "sad", "max_abs", "overlap_top1pct"}
            assert d[p]["worst"] == fmm.worst_tiles(m, 16) and d[p]["share_top1pct"] == fmm.share_top1pct(m)
            assert (d[p]["sse"], d[p]["sad"], d[p]["max_abs"]) == (int(m["sse"].sum()), int(m["sad"].sum()), int(m["max_abs"].max()))
        # 6 tiles: k = 1.  Y: the error map's worst tile is (16, 0), first of two equals; U: the error map is zero; V: one tile in both
        assert d["Y"]["worst"][0] == ({"x": 16, "y": 0, "sse": 8, "max_abs": 2} if k % 2 else {"x": 0, "y": 16, "sse": 8, "max_abs": 2})
        assert (d["Y"]["overlap_top1pct"], d["U"]["overlap_top1pct"], d["V"]["overlap_top1pct"]) == (1.0 if k % 2 else 0.0, None, 1.0)
        assert "disagreement" not in r["repeat"]
    assert rep["clip"]["disagreement"] == {"Y": {"sse": 22 + 16 + 22, "overlap_top1pct": 2 / 3}, "U": {"sse": 12, "overlap_top1pct": None},
                                           "V": {"sse": 5 + 10 + 15 + 3, "overlap_top1pct": 1.0}}
    assert rep["clip"]["worst_tile_disagreement"] == {"pair": 1, "plane": "Y", "x": 16, "y": 0, "sse": 8}   # (the first of equals: the earlier pair)
    assert json.loads(json.dumps(rep)) == rep
    # the rest of the report is the run with the error map alone
    only_map = quality.evaluate(tq._tagged_frames(9), False, 4, 4, device=tqm._MapWorld(), error_map=16)
    del rep["clip"]["disagreement"], rep["clip"]["worst_tile_disagreement"]
    for r in rep["pairs"]:
        del r["interpolated"]["disagreement"]
    assert rep == only_map


def test_without_an_error_map_of_the_same_tile_there_is_no_overlap():
    from hopperrender_amd import quality
    for kw in ({"disagreement": 32}, {"disagreement": 32, "error_map": 16}):
        rep = quality.evaluate(tq._tagged_frames(9), False, 4, 4, device=_DisWorld(), **kw)
        d = rep["pairs"][0]["interpolated"]["disagreement"]
        assert d["tile"] == 32 and all("overlap_top1pct" not in d[p] for p in "YUV") and d["Y"]["worst"][0]["x"] == 32
        assert rep["clip"]["disagreement"] == {"Y": {"sse": 60}, "U": {"sse": 12}, "V": {"sse": 33}}


def test_read_once_per_chunk_into_the_same_buffer(monkeypatch):
    from hopperrender_amd import quality
    monkeypatch.setattr(quality, "PAIRS_PER_READ", 2)
    w = _DisWorld()
    rep = quality.evaluate(tq._tagged_frames(21), False, 4, 4, device=w, disagreement=64)
    names = [c[1] for c in w.log if c[0] == "main"]
    assert names.count("dis_enqueue") == 9 and names.count("read") == 5
    assert [c[4] for c in w.log if c[:2] == ("main", "dis_enqueue")] == [0, MAP_BYTES] * 4 + [0]
    assert [c[2] for c in w.log if c[0] == "maps"] == [2 * MAP_BYTES] * 4 + [MAP_BYTES]
    assert len(w.map_bufs) == 1 and w.map_bufs[0].nbytes == 2 * MAP_BYTES and len(rep["pairs"]) == 9
    assert [r["interpolated"]["disagreement"]["V"]["worst"][0]["sse"] for r in rep["pairs"]] == [5 * k for k in range(1, 10)]


def test_without_the_option_nothing_new_is_called_and_the_report_is_todays():
    from hopperrender_amd import quality
    w, plain = _DisWorld(), tq._FakeWorld()
    rep = quality.evaluate(tq._tagged_frames(9), False, 4, 4, device=w)
    assert rep == quality.evaluate(tq._tagged_frames(9), False, 4, 4, device=plain)   # (a calculator without the new method serves)
    assert rep == quality.evaluate(tq._tagged_frames(9), False, 4, 4, device=_DisWorld(), disagreement=0)
    assert w.log == plain.log and not w.map_bufs and not w.dis_seen
    assert "disagreement" not in rep["clip"] and "worst_tile_disagreement" not in rep["clip"]
    assert all("disagreement" not in r["interpolated"] for r in rep["pairs"])
    for bad in (8, 48, 128, -16):
        with pytest.raises(ValueError):
            quality.evaluate(tq._tagged_frames(9), False, 4, 4, device=_DisWorld(), disagreement=bad)


def test_overlap_on_hand_made_maps_ties_included():
    """150 tiles: k = 2.  The first k of either map in the order of `worst` (larger sse; ties by lower y, then lower x)."""
    from hopperrender_amd import quality
    err, dis = np.zeros((10, 15), fmm.TILE_DTYPE), np.zeros((10, 15), fmm.TILE_DTYPE)
    assert quality._overlap_top1pct(err, dis, 16) is None
    err["sse"][3, 4], err["sse"][9, 14] = 100, 50
    assert quality._overlap_top1pct(err, dis, 16) is None and quality._overlap_top1pct(dis, err, 16) is None
    dis["sse"][3, 4], dis["sse"][0, 0] = 7, 9
    assert quality._overlap_top1pct(err, dis, 16) == (1, 2)
    dis["sse"][9, 14] = 9          # ties with (0, 0), which is first: the top two are (0, 0) and (9, 14)
    assert quality._top1pct(dis, 16) == [(0, 0), (9, 14)] and quality._overlap_top1pct(err, dis, 16) == (1, 2)
    dis["sse"][3, 4] = 9           # three equals: (0, 0) and (3, 4) go first
    assert quality._top1pct(dis, 16) == [(0, 0), (3, 4)] and quality._overlap_top1pct(err, dis, 16) == (1, 2)
    dis["sse"][0, 0] = 0
    assert quality._overlap_top1pct(err, dis, 16) == (2, 2)
    err["sse"][:] = 5              # every tile equal: the first two in reading order
    assert quality._top1pct(err, 64) == [(0, 0), (0, 1)] and quality._overlap_top1pct(err, dis, 64) == (0, 2)
    one = np.zeros((2, 3), fmm.TILE_DTYPE)
    one["sse"][1, 2] = 1
    assert quality._overlap_top1pct(one, one, 32) == (1, 1)


def test_heat_maps_of_the_disagreement_are_scaled_to_their_own_clip_maximum(tmp_path):
    from hopperrender_amd import quality
    quality.evaluate(tq._tagged_frames(9), False, 32, 48, device=_DisWorld(), error_map=16, disagreement=16, map_dir=str(tmp_path / "m"))
    files = sorted(os.listdir(tmp_path / "m"))
    assert files == [f"{k}_pair000{i}.pgm" for k in ("dis", "map") for i in (1, 2, 3)]
    rms = [np.sqrt(_fake_dis(k)["sse"][0] / 256.0) for k in (1, 2, 3)]
    top = max(r.max() for r in rms)
    for k in range(3):
        raw = open(tmp_path / "m" / files[k], "rb").read()
        assert raw.startswith(b"P5\n3 2\n255\n") and list(raw[11:]) == np.rint(rms[k] * 255.0 / top).astype(np.uint8).reshape(-1).tolist()
        assert max(raw[11:]) == 255   # (every pair's largest Y tile is 8, the clip's own maximum -- not the error maps' 27)


# ---- confidence(): every frame a source, the real schedule, no output ----
S24, T60 = 417083, 166833


def test_confidence_schedule_and_gating():
    from hopperrender_amd import protocol, quality
    sched = quality.confidence_schedule(6, S24, T60)
    assert [(s["period"], s["source_frame"], s["flow"], s["pair"], s["evaluated"]) for s in sched] == [
        (0, 0, False, None, False), (1, 1, False, None, False), (2, 2, True, 0, False), (3, 3, True, 1, True), (4, 4, True, 2, True),
        (5, 5, True, 3, True), (6, 5, True, 4, True)]
    assert [s["t"] for s in sched] == protocol.BlendSchedule(S24, T60).plan(7)
    assert [len(s["t"]) for s in sched] == [3, 3, 2, 3, 2, 3, 2] and sched[2]["t"] == pytest.approx([0.4, 0.8], abs=1e-4)   # (166833 / 417083 is a little below 0.4)
    with pytest.raises(ValueError):
        quality.confidence_schedule(2, S24, T60)


def test_confidence_calls_report_and_no_output_frame():
    from hopperrender_amd import quality
    w = _DisWorld()
    rep = quality.confidence(tq._tagged_frames(6), False, 4, 6, device=w, source_frame_time=S24, target_frame_time=T60, tile=32, search_radius=9)
    sched = quality.confidence_schedule(6, S24, T60)
    main = [c[1:] for c in w.log if c[0] == "main"]
    assert [c[0] for c in main] == ["map_shape", "update", "update", "period", "period", "dis_enqueue", "period", "dis_enqueue", "period", "dis_enqueue",
                                    "period", "dis_enqueue", "sync", "close"]
    assert [c[1] for c in main if c[0] in ("update", "period")] == [0, 1, 2, 3, 4, 5, 5] and len(w.calcs) == 1
    # one launch per period with all its t's, the maps side by side in one buffer; nothing but sources and that buffer is allocated
    offs, at = [], 0
    for s in sched[3:]:
        offs.append(("dis_enqueue", 32, tuple(s["t"]), at))
        at += len(s["t"]) * MAP_BYTES
    assert [c for c in main if c[0] == "dis_enqueue"] == offs and at == 10 * MAP_BYTES
    assert len(w.map_bufs) == 1 and w.map_bufs[0].nbytes == 10 * MAP_BYTES and [c for c in w.log if c[0] == "maps"] == [("maps", "download", at)]
    assert len(w.bufs) == 7 + 1 and sorted(w.freed) == sorted(b.ptr for b in w.bufs)
    # frames N-2, N-1 and the flow calculated one period earlier
    assert [d[:3] for d in w.dis_seen] == [(1, 2, (1, 2))] * 3 + [(2, 3, (2, 3))] * 2 + [(3, 4, (3, 4))] * 3 + [(4, 5, (4, 5))] * 2
    assert rep["warmup_pairs"] == [0] and rep["tile"] == 32 and rep["shape"] == [TH, TW] and rep["settings"]["search_radius"] == 9
    assert [(r["period"], r["pair"], r["source_frames"], r["t"]) for r in rep["periods"]] == [(s["period"], s["pair"], [s["pair"], s["pair"] + 1], s["t"]) for s in sched[3:]]
    k = 0
    for r in rep["periods"]:
        assert [o["t"] for o in r["outputs"]] == r["t"]
        for o in r["outputs"]:
            k += 1
            m = _fake_dis(k)
            for i, (p, cnt) in enumerate((("Y", 24), ("U", 6), ("V", 6))):
                sse = int(m["sse"][i].sum())
                assert o[p] == {"sse": sse, "sad": int(m["sad"][i].sum()), "max_abs": int(m["max_abs"][i].max()), "rms": math.sqrt(sse / cnt),
                                "worst": fmm.worst_tiles(m[i], 32, 1)[0]}
        assert r["mean_rms_y"] == sum(o["Y"]["rms"] for o in r["outputs"]) / len(r["outputs"])
    assert k == 10
    y = [int(_fake_dis(k)["sse"][0].sum()) for k in range(1, 11)]
    assert rep["clip"]["Y"]["sse"] == sum(y) and rep["clip"]["Y"]["rms"] == math.sqrt(sum(y) / (24 * 10)) and rep["clip"]["V"]["max_abs"] == 3
    assert rep["clip"]["worst"] == {"period": 3, "pair": 1, "t": sched[3]["t"][0], "rms_y": math.sqrt(22 / 24)}   # (the first of equals)
    assert rep["clip"]["mean_rms_y"] == [r["mean_rms_y"] for r in rep["periods"]] and len(rep["clip"]["mean_rms_y"]) == 4
    assert json.loads(json.dumps(rep)) == rep


def test_confidence_chunks_by_map_bytes(monkeypatch):
    """A budget of 5 maps: periods of 3, 2 | 3, 2 outputs -- a chunk is whole periods; the buffer is the largest chunk's, read once per chunk;
    a budget below one period's maps still takes a period at a time."""
    from hopperrender_amd import quality
    monkeypatch.setattr(quality, "CONFIDENCE_MAP_BYTES", 5 * MAP_BYTES)
    w = _DisWorld()
    rep = quality.confidence(tq._tagged_frames(6), False, 4, 6, device=w, source_frame_time=S24, target_frame_time=T60)
    assert [c[2] for c in w.log if c[0] == "maps"] == [5 * MAP_BYTES] * 2 and w.map_bufs[0].nbytes == 5 * MAP_BYTES
    assert [c[4] for c in w.log if c[:2] == ("main", "dis_enqueue")] == [0, 3 * MAP_BYTES, 0, 3 * MAP_BYTES]
    assert [c[1] for c in w.log if c[0] == "main"].count("sync") == 2 and len(w.bufs) < 7 + 1   # (sources are used again across chunks)
    whole = quality.confidence(tq._tagged_frames(6), False, 4, 6, device=_DisWorld(), source_frame_time=S24, target_frame_time=T60)
    assert rep == whole
    monkeypatch.setattr(quality, "CONFIDENCE_MAP_BYTES", 1)
    w = _DisWorld()
    assert quality.confidence(tq._tagged_frames(6), False, 4, 6, device=w, source_frame_time=S24, target_frame_time=T60) == whole
    assert [c[2] for c in w.log if c[0] == "maps"] == [n * MAP_BYTES for n in (3, 2, 3, 2)] and w.map_bufs[0].nbytes == 3 * MAP_BYTES
    with pytest.raises(ValueError):
        quality.confidence(tq._tagged_frames(6), False, 4, 6, device=_DisWorld(), source_frame_time=S24, target_frame_time=T60, tile=20)


def test_confidence_chunks_by_source_bytes_too(monkeypatch):
    """Every source of a chunk is uploaded before the chunk is submitted, so a chunk is also bounded by its sources: three frames' worth
    here, whatever the maps take.  The report is that of the one-chunk run."""
    from hopperrender_amd import quality
    whole = quality.confidence(tq._tagged_frames(6), False, 4, 6, device=_DisWorld(), source_frame_time=S24, target_frame_time=T60)
    monkeypatch.setattr(quality, "CONFIDENCE_SOURCE_BYTES", 3 * 24)
    w = _DisWorld()
    assert quality.confidence(tq._tagged_frames(6), False, 4, 6, device=w, source_frame_time=S24, target_frame_time=T60) == whole
    main = [c[1] for c in w.log if c[0] == "main"]
    assert main == ["map_shape", "update", "update", "period", "sync", "period", "dis_enqueue", "period", "dis_enqueue", "period", "dis_enqueue", "sync",
                    "period", "dis_enqueue", "sync", "close"]
    assert [c[2] for c in w.log if c[0] == "maps"] == [8 * MAP_BYTES, 2 * MAP_BYTES] and w.map_bufs[0].nbytes == 8 * MAP_BYTES
    assert len(w.bufs) == 6 + 1   # three sources a chunk and the three the ring still references, used again


def test_the_command_line_refuses_what_a_confidence_run_cannot_honour(capsys):
    from hopperrender_amd import quality
    ok = quality.parse_args(["clip.y4m", "--confidence", "--target-fps", "59.94", "--disagreement", "32", "--radius", "8"])
    assert ok.confidence and ok.disagreement == 32 and ok.target_fps == 59.94
    for extra in (["--ssim"], ["--map", "16"], ["--ssim-map", "16"], ["--map-dir", "d", "--disagreement", "16"], ["--detect-cuts"],
                  ["--black", "16"], ["--white", "235"]):
        with pytest.raises(SystemExit):
            quality.parse_args(["clip.y4m", "--confidence", "--target-fps", "60"] + extra)
        assert extra[0] in capsys.readouterr().err
    for bad in (["--confidence"], ["--target-fps", "60"]):
        with pytest.raises(SystemExit):
            quality.parse_args(["clip.y4m"] + bad)
    capsys.readouterr()
