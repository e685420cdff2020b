"""CPU: the pieces of the leave-one-out quality evaluation that need no GPU -- the numpy model of the device's frame error sums, the PSNR
formula, the evaluator's schedule (against a fake calculator that records calls), and the condition under which the evaluation means
anything: on the synthetic scenes the oracle's interpolation is clearly closer to the withheld frame than repeating a frame is."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frame_error_model as fem  # noqa: E402


# ---- the model on hand-made frames ----
def test_model_semiplanar_hand_made():
    """4 x 4 NV12 with stride 6: two luma differences, one in U, two in V; padding differs everywhere and counts for nothing."""
    H, W, S = 4, 4, 6
    a = np.zeros((H + H // 2) * S, np.uint8)
    b = a.copy()
    a.reshape(-1, S)[:, W:] = 200                      # padding columns: garbage on one side only
    A, B = a.reshape(-1, S), b.reshape(-1, S)
    A[0, 0], B[0, 0] = 10, 13                          # Y: |d| = 3
    A[3, 3], B[3, 3] = 255, 0                          # Y: |d| = 255, last row and column
    A[4, 2], B[4, 2] = 7, 5                            # U(0, 1): 2
    A[4, 1], B[4, 1] = 0, 9                            # V(0, 0): 9
    A[5, 3], B[5, 3] = 100, 90                         # V(1, 1): 10
    e = fem.frame_error(a, b, H, W, S, S)
    assert e["Y"] == {"sse": 9 + 255 * 255, "sad": 258, "max_abs": 255, "n_differ": 2, "count": 16}
    assert e["U"] == {"sse": 4, "sad": 2, "max_abs": 2, "n_differ": 1, "count": 4}
    assert e["V"] == {"sse": 181, "sad": 19, "max_abs": 10, "n_differ": 2, "count": 4}


def test_model_planar_hand_made_and_its_semiplanar_twin():
    """The same content as planar Y, U, V planes (chroma rows of stride / 2) gives the same sums; each side has its own stride."""
    from hopperrender_amd.y4m import semiplanar_to_planar
    rng = np.random.default_rng(1)
    H, W = 6, 8
    a, b = rng.integers(0, 65536, (H + H // 2) * W, dtype=np.uint16), rng.integers(0, 65536, (H + H // 2) * W, dtype=np.uint16)
    want = fem.frame_error(a, b, H, W)

    def planar(f, S):   # Y rows of S, then U and V rows of S / 2, padding filled with noise
        y, u, v = fem.split_planes(f, H, W)
        out = rng.integers(0, 65536, H * S + 2 * (H // 2) * (S // 2), dtype=np.uint16)
        out[:H * S].reshape(H, S)[:, :W] = y
        out[H * S:H * S + (H // 2) * (S // 2)].reshape(H // 2, S // 2)[:, :W // 2] = u
        out[H * S + (H // 2) * (S // 2):].reshape(H // 2, S // 2)[:, :W // 2] = v
        return out
    assert fem.frame_error(planar(a, 8), planar(b, 12), H, W, 8, 12, planar=True) == want
    assert fem.frame_error(planar(a, 10), planar(b, 10), H, W, 10, 10, planar=True) == want
    assert want["Y"]["count"] == 48 and want["U"]["count"] == want["V"]["count"] == 12
    assert want["Y"]["sse"] == int(((a[:48].astype(np.int64) - b[:48].astype(np.int64)) ** 2).sum())
    own = np.concatenate([x.reshape(-1) for x in semiplanar_to_planar(a, H, W, False)])   # the library's own re-layout agrees on where U and V live
    assert all(v["n_differ"] == 0 for v in fem.frame_error(own, planar(a, 8), H, W, 8, 8, planar=True).values())


def test_psnr_formula():
    from hopperrender_amd import quality
    for f in (quality.psnr, fem.psnr):
        assert f(0, 100, 255) is None
        assert f(100, 100, 255) == pytest.approx(20 * math.log10(255))           # mse 1
        assert f(65025 * 50, 50, 255) == pytest.approx(0.0, abs=1e-12)            # every element off by the peak
        assert f(4 * 7, 7, 65535) == pytest.approx(10 * math.log10(65535 ** 2 / 4))
        big = 3840 * 2160 * 65535 ** 2                                            # past 2^53: plain ints in, a float out
        assert f(big, 3840 * 2160, 65535) == pytest.approx(0.0, abs=1e-9)


# ---- the evaluator's schedule, against a fake calculator ----
class _FakeBuf:
    def __init__(self, world):
        self.world, self.ptr = world, 0x1000 * (len(world.bufs) + 1)
        world.bufs.append(self)

    def upload(self, a):
        assert self.ptr not in self.world.referenced(), "a source the context's ring still references was overwritten"
        self.world.mem[self.ptr] = ("raw", int(a[0]))

    def free(self):
        self.world.freed.append(self.ptr)


class _FakeCalc:
    input_frame_bytes = output_frame_bytes = 24

    def __init__(self, world, name):
        self.w, self.name, self.ring, self.m_frameCount, self.target, self.flow, self.slots = world, name, [], 0, None, None, {}
        self.m_totalFrameDelta = 0

    def _log(self, *what):
        self.w.log.append((self.name,) + what)

    def _push(self, ptr):
        self.ring = (self.ring + [(ptr, self.w.mem[ptr][1])])[-3:]
        self.m_frameCount += 1

    def setOutputBuffer(self, ptr):
        self.target = ptr

    def updateFrameDevice(self, ptr):
        self._log("update", self.w.mem[ptr][1]); self._push(ptr)

    def updateFrameDeviceRef(self, ptr):
        self._log("update", self.w.mem[ptr][1]); self._push(ptr)

    def copyFrame(self):
        assert self.m_frameCount == 1, "copyFrame shows the frame just submitted only while m_frameCount is 1"
        self.w.mem[self.target] = ("copy", self.ring[-1][1])

    def interpolatePeriod(self, ptr, ts, outs, mode):
        self._log("period", self.w.mem[ptr][1]); self._push(ptr)
        assert self.m_frameCount >= 3 and list(ts) == [0.5] and mode == 2 and len(outs) == 1
        a, b, c = [x[1] for x in self.ring]
        self.w.mem[outs[0]] = ("warp", a, b, self.flow)   # frames N-2, N-1 with the PREVIOUS flow
        self.flow = (b, c)

    def frameErrorEnqueue(self, a, b, first_slot):
        self._log("enqueue", first_slot, len(a))
        for i, (x, y) in enumerate(zip(a, b)):
            self.slots[first_slot + i] = (self.w.mem[x], self.w.mem[y])

    def frameErrorRead(self, first, n):
        self._log("read", first, n)
        out = []
        for k in range(first, first + n):
            self.w.compared.append(self.slots[k])
            i = len(self.w.compared)
            out.append({p: {"sse": 0 if (i == 2 and p == "U") else 1000 * i + j, "sad": 10 * i, "max_abs": i, "n_differ": i, "count": 96 // (1 + 3 * (j > 0))}
                        for j, p in enumerate("YUV")})
        return out

    def sync(self):
        self._log("sync")

    def waitFlow(self):
        self._log("waitFlow")

    def close(self):
        self._log("close")


class _FakeWorld:
    def __init__(self):
        self.bufs, self.mem, self.freed, self.log, self.compared, self.calcs = [], {}, [], [], [], []

    def referenced(self):
        return [p for c in self.calcs if c.name == "main" for p, _ in c.ring]

    def calc(self, hdr, H, W, black, white, settings):
        c = _FakeCalc(self, "main" if not self.calcs else "aux")
        c.settings = dict(settings)
        self.calcs.append(c)
        return c

    def buffer(self, nbytes):
        assert nbytes == 24
        return _FakeBuf(self)


def _tagged_frames(n):
    return [np.full(24, k, np.uint8) for k in range(n)]


def test_schedule_which_period_is_compared_with_which_withheld_frame():
    """9 frames: sources 0, 2, 4, 6, 8.  The first flow is calculated when the third source arrives, so the period of source 4 shows
    (0, 2) without one: pair 0 is warm-up.  Pairs 1 .. 3 are compared with the withheld frames 3, 5, 7 through copyFrame, the repeat
    baseline is copyFrame of the pair's first source, the last source goes in once more so that (6, 8) is reached -- and nothing is read
    or waited for on the clip's context before the last comparison is enqueued."""
    from hopperrender_amd import quality
    w = _FakeWorld()
    rep = quality.evaluate(_tagged_frames(9), False, 4, 4, device=w, search_radius=7, blur_radius=32)
    assert [c for c in w.log if c[0] == "main" and c[1] in ("update", "period")] == [
        ("main", "update", 0), ("main", "update", 2), ("main", "period", 4), ("main", "period", 6), ("main", "period", 8), ("main", "period", 8)]
    assert w.compared == [
        (("warp", 2, 4, (2, 4)), ("copy", 3)), (("copy", 2), ("copy", 3)),
        (("warp", 4, 6, (4, 6)), ("copy", 5)), (("copy", 4), ("copy", 5)),
        (("warp", 6, 8, (6, 8)), ("copy", 7)), (("copy", 6), ("copy", 7))]
    main_calls = [c[1] for c in w.log if c[0] == "main"]
    assert main_calls.count("read") == 1 and main_calls.index("read") > max(i for i, c in enumerate(main_calls) if c == "enqueue")
    assert not {"sync", "waitFlow"} & set(main_calls)
    assert [c[1] for c in w.log if c[0] == "aux"].count("sync") == 1
    assert w.log.index(("aux", "sync")) < w.log.index(("main", "update", 0))
    assert rep["warmup_pairs"] == [0] and [r["pair"] for r in rep["pairs"]] == [1, 2, 3]
    assert [(r["source_frames"], r["withheld_frame"], r["period"]) for r in rep["pairs"]] == [([2, 4], 3, 3), ([4, 6], 5, 4), ([6, 8], 7, 5)]
    assert rep["settings"]["search_radius"] == 7 and rep["settings"]["blur_radius"] == 32 and rep["settings"]["delta_scalar"] == 8
    assert w.calcs[0].settings == w.calcs[1].settings
    # the sums are passed through, PSNR is the formula on them, sse == 0 gives None; aggregates are the PSNR of the summed sse
    r0 = rep["pairs"][0]
    assert r0["interpolated"]["Y"] == {"sse": 1000, "sad": 10, "max_abs": 1, "n_differ": 1, "count": 96, "psnr": quality.psnr(1000, 96, 255)}
    assert r0["repeat"]["U"]["sse"] == 0 and r0["repeat"]["U"]["psnr"] is None
    assert r0["gain_db_y"] == pytest.approx(quality.psnr(1000, 96, 255) - quality.psnr(2000, 96, 255))
    assert rep["clip"]["interpolated"]["Y"]["sse"] == 1000 + 3000 + 5000 and rep["clip"]["interpolated"]["Y"]["count"] == 3 * 96
    assert rep["clip"]["interpolated"]["Y"]["psnr"] == pytest.approx(quality.psnr(9000, 288, 255))
    assert rep["clip"]["repeat"]["V"]["sse"] == 2002 + 4002 + 6002 and rep["clip"]["repeat"]["V"]["count"] == 3 * 24
    assert rep["clip"]["worst_pair"] == {"pair": 3, "psnr_y": quality.psnr(5000, 96, 255)}
    assert rep["scene_cuts"] is None
    import json
    assert json.loads(json.dumps(rep)) == rep
    assert sorted(w.freed) == sorted(b.ptr for b in w.bufs) and "close" in main_calls


def test_schedule_even_frame_count_short_clips_and_unknown_settings():
    from hopperrender_amd import quality
    s = quality.schedule(10)   # the tenth frame would be a withheld frame without a right neighbour: not used
    assert [x["source_frame"] for x in s] == [0, 2, 4, 6, 8, 8] and [x["truth_frame"] for x in s if x["evaluated"]] == [3, 5, 7]
    assert [x["evaluated"] for x in quality.schedule(5)] == [False, False, False, True]
    for n in (0, 1, 4):
        with pytest.raises(ValueError):
            quality.schedule(n)
    with pytest.raises(TypeError):
        quality.evaluate(_tagged_frames(9), False, 4, 4, device=_FakeWorld(), radius=5)


def test_long_clips_are_read_in_chunks_and_ring_sources_survive(monkeypatch):
    """More pairs than result slots: one read per chunk, buffers are used again after it -- but never a source the ring still holds
    (the fake refuses such an upload) -- and the comparisons are the same as in one piece."""
    from hopperrender_amd import quality
    whole = _FakeWorld()
    quality.evaluate(_tagged_frames(21), False, 4, 4, device=whole)
    monkeypatch.setattr(quality, "PAIRS_PER_READ", 2)
    w = _FakeWorld()
    rep = quality.evaluate(_tagged_frames(21), False, 4, 4, device=w)
    assert [r["pair"] for r in rep["pairs"]] == list(range(1, 10))
    assert w.compared == whole.compared and len(w.compared) == 18
    assert [c[1] for c in w.log if c[0] == "main"].count("read") == 5
    assert len(w.bufs) < len(whole.bufs)


def test_sweep_parsing():
    from hopperrender_amd import quality
    assert quality.parse_sweeps(["radius=5,16", "blur=4,32"]) == [
        {"search_radius": 5, "blur_radius": 4}, {"search_radius": 5, "blur_radius": 32}, {"search_radius": 16, "blur_radius": 4}, {"search_radius": 16, "blur_radius": 32}]
    assert quality.parse_sweeps(None) == [{}]
    assert quality.parse_sweeps(["max-calc-res=135,270"]) == [{"max_calc_res": 135}, {"max_calc_res": 270}]
    for bad in ("radius", "speed=1,2", "radius="):
        with pytest.raises(ValueError):
            quality.parse_sweeps([bad])


# ---- the evaluation means something ----
@pytest.mark.parametrize("hdr,H,W,seed", [(False, 360, 640, 1234), (False, 360, 640, 7), (True, 360, 640, 1234), (False, 180, 320, 1234)],
                         ids=["sdr360-1234", "sdr360-7", "hdr360-1234", "sdr180-1234"])
def test_oracle_interpolation_beats_frame_repeat_by_2_db(hdr, H, W, seed):
    """Leave-one-out on synth.Scene at R = 16: on every pair the evaluator scores (sources (2 p, 2 p + 2), withheld 2 p + 1, p = 1 .. 3 of
    a 9-frame clip) the CPU oracle's blended frame at t = 0.5 is at least 2 dB of Y-PSNR closer to the withheld frame than the repeated
    first source, both against copyFrame(withheld) at the default levels.  Measured on these pairs (oob == 0 everywhere), Y-PSNR
    interpolation / repeat / gain in dB:
        360 x 640 SDR seed 1234   17.57 / 11.71 / 5.85    18.48 / 11.83 / 6.65    18.02 / 11.69 / 6.33
        360 x 640 SDR seed 7      18.78 / 12.04 / 6.74    19.20 / 11.72 / 7.48    19.02 / 11.80 / 7.22
        360 x 640 HDR seed 1234   18.92 / 13.04 / 5.88    19.82 / 13.15 / 6.66    19.36 / 13.02 / 6.35   (with the x 65535 / 65280 levels stretch)
        180 x 320 SDR seed 1234   16.52 / 11.72 / 4.79    16.40 / 11.72 / 4.68    16.56 / 11.72 / 4.84
    (R = 5 on the same pairs: gains of 2.2 to 8.2 dB.)"""
    import quality_cases
    rows = quality_cases.oracle_pairs(hdr, H, W, seed, 16)
    assert [r["pair"] for r in rows] == [1, 2, 3]
    peak = 65535 if hdr else 255
    for r in rows:
        assert r["oob"] == 0
        a = fem.psnr(r["interpolated"]["Y"]["sse"], r["interpolated"]["Y"]["count"], peak)
        b = fem.psnr(r["repeat"]["Y"]["sse"], r["repeat"]["Y"]["count"], peak)
        print(f"pair {r['pair']}: interpolation {a:.2f} dB, repeat {b:.2f} dB, gain {a - b:.2f} dB")
        assert a - b >= 2.0, (r["pair"], a, b)
