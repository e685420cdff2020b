"""CPU: the evaluator's SSIM option without a GPU -- what it calls on the clip's context (a recording fake in the style of
tests/test_quality.py), what the report gains and that it gains nothing when the option is off -- and the condition under which the number
means anything: on the synthetic scenes the oracle's interpolation has a far higher Y-SSIM than a repeated frame."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_quality as tq  # noqa: E402

NEW_PLANE_KEYS = {"sum_loss_q32", "max_loss_q32", "ssim_count", "ssim", "min_ssim"}


class _SsimCalc(tq._FakeCalc):
    def __init__(self, world, name):
        super().__init__(world, name)
        self.ssim_slots = {}

    def frameSsimEnqueue(self, a, b, first_slot):
        self._log("ssim_enqueue", first_slot, len(a))
        for i, (x, y) in enumerate(zip(a, b)):
            self.ssim_slots[first_slot + i] = (self.w.mem[x], self.w.mem[y])

    def frameSsimRead(self, first, n):
        self._log("ssim_read", first, n)
        out = []
        for k in range(first, first + n):
            self.w.ssim_compared.append(self.ssim_slots[k])
            i = len(self.w.ssim_compared)
            # slot i: Y loses i / 16 per window over 8 windows with a worst window of i / 8; U has no window; V is equal
            out.append({"Y": {"sum_loss_q32": (i << 28) * 8, "max_loss_q32": i << 29, "count": 8},
                        "U": {"sum_loss_q32": 0, "max_loss_q32": 0, "count": 0}, "V": {"sum_loss_q32": 0, "max_loss_q32": 0, "count": 2}})
        return out


class _SsimWorld(tq._FakeWorld):
    def __init__(self):
        super().__init__()
        self.ssim_compared = []

    def calc(self, hdr, H, W, black, white, settings):
        c = _SsimCalc(self, "main" if not self.calcs else "aux")
        c.settings = dict(settings)
        self.calcs.append(c)
        return c


def test_ssim_goes_out_beside_every_error_enqueue_and_is_read_once():
    """The SSIM enqueues carry the slots and pairs of the error enqueues, each straight behind its twin; one read of each kind after the
    last enqueue; nothing else is called on the clip's context."""
    from hopperrender_amd import quality
    w = _SsimWorld()
    rep = quality.evaluate(tq._tagged_frames(9), False, 4, 4, device=w, ssim=True)
    main = [c[1:] for c in w.log if c[0] == "main"]
    assert [c for c in main if c[0] in ("enqueue", "ssim_enqueue")] == [
        ("enqueue", 0, 2), ("ssim_enqueue", 0, 2), ("enqueue", 2, 2), ("ssim_enqueue", 2, 2), ("enqueue", 4, 2), ("ssim_enqueue", 4, 2)]
    assert w.ssim_compared == w.compared and len(w.compared) == 6
    names = [c[0] for c in main]
    assert names == ["update", "update", "period", "period", "enqueue", "ssim_enqueue", "period", "enqueue", "ssim_enqueue",
                     "period", "enqueue", "ssim_enqueue", "read", "ssim_read", "close"]
    assert [c for c in main if c[0] in ("read", "ssim_read")] == [("read", 0, 6), ("ssim_read", 0, 6)]
    # the integers are passed through beside the error sums (whose count keeps its meaning), the floats derive from them
    r0 = rep["pairs"][0]
    y = r0["interpolated"]["Y"]
    assert (y["sum_loss_q32"], y["max_loss_q32"], y["ssim_count"], y["count"], y["sse"]) == (8 << 28, 1 << 29, 8, 96, 1000)
    assert y["ssim"] == 1 - 1 / 16 and y["min_ssim"] == 1 - 1 / 8
    assert r0["repeat"]["Y"]["ssim"] == 1 - 2 / 16 and r0["gain_ssim_y"] == pytest.approx(1 / 16)
    assert r0["interpolated"]["U"]["ssim"] is None and r0["interpolated"]["U"]["min_ssim"] is None and r0["interpolated"]["U"]["ssim_count"] == 0
    assert r0["interpolated"]["V"]["ssim"] == 1.0 and r0["interpolated"]["V"]["min_ssim"] == 1.0
    # aggregates: summed loss over summed count, the largest loss; slots 1, 3, 5 are the interpolations, 2, 4, 6 the repeats
    agg = rep["clip"]["interpolated"]["Y"]
    assert (agg["sum_loss_q32"], agg["ssim_count"], agg["max_loss_q32"]) == ((1 + 3 + 5) * 8 << 28, 24, 5 << 29)
    assert agg["ssim"] == pytest.approx(1 - 9 / 48) and agg["min_ssim"] == 1 - 5 / 8
    assert rep["clip"]["repeat"]["Y"]["ssim"] == pytest.approx(1 - 12 / 48) and rep["clip"]["gain_ssim_y"] == pytest.approx(3 / 48)
    assert rep["clip"]["interpolated"]["U"]["ssim"] is None
    assert rep["clip"]["worst_pair_ssim"] == {"pair": 3, "ssim_y": 1 - 5 / 16}
    assert rep["clip"]["worst_pair"] == {"pair": 3, "psnr_y": quality.psnr(5000, 96, 255)}   # (the error side is what it was)
    assert json.loads(json.dumps(rep)) == rep


def test_ssim_is_read_once_per_chunk(monkeypatch):
    from hopperrender_amd import quality
    monkeypatch.setattr(quality, "PAIRS_PER_READ", 2)
    w = _SsimWorld()
    rep = quality.evaluate(tq._tagged_frames(21), False, 4, 4, device=w, ssim=True)
    names = [c[1] for c in w.log if c[0] == "main"]
    assert names.count("read") == names.count("ssim_read") == 5 and names.count("enqueue") == names.count("ssim_enqueue") == 9
    assert all(names[i + 1] == "ssim_read" for i, n in enumerate(names) if n == "read")
    assert w.ssim_compared == w.compared and len(rep["pairs"]) == 9


def test_without_the_option_no_ssim_method_is_touched_and_the_report_is_todays():
    from hopperrender_amd import quality
    w, plain = _SsimWorld(), tq._FakeWorld()
    rep = quality.evaluate(tq._tagged_frames(9), False, 4, 4, device=w)
    assert rep == quality.evaluate(tq._tagged_frames(9), False, 4, 4, device=plain)   # (a calculator without SSIM methods serves)
    assert rep == quality.evaluate(tq._tagged_frames(9), False, 4, 4, device=_SsimWorld(), ssim=False)
    assert not [c for c in w.log if c[1].startswith("ssim")] and w.log == plain.log
    assert not {"gain_ssim_y", "worst_pair_ssim"} & set(rep["clip"]) and "gain_ssim_y" not in rep["pairs"][0]
    for r in rep["pairs"] + [rep["clip"]]:
        for kind in ("interpolated", "repeat"):
            assert all(not NEW_PLANE_KEYS & set(r[kind][p]) for p in "YUV")
    on = quality.evaluate(tq._tagged_frames(9), False, 4, 4, device=_SsimWorld(), ssim=True)
    assert NEW_PLANE_KEYS <= set(on["pairs"][0]["repeat"]["V"]) and NEW_PLANE_KEYS <= set(on["clip"]["interpolated"]["Y"])


# ---- the evaluation means something ----
@pytest.mark.parametrize("hdr,H,W,seed", [(False, 180, 320, 1234), (True, 360, 640, 1234), (False, 360, 640, 7)],
                         ids=["sdr180-1234", "hdr360-1234", "sdr360-7"])
def test_oracle_interpolation_beats_frame_repeat_by_half_of_the_ssim_scale(hdr, H, W, seed):
    """Leave-one-out on synth.Scene at R = 16: on every scored pair (p = 1, 2, 3) the CPU oracle's blended frame at t = 0.5 has a mean
    Y-SSIM at least 0.5 above the repeated first source, both against copyFrame(withheld).  Measured, interpolation / repeat:
        180 x 320 SDR seed 1234   0.647 / 0.048    0.623 / 0.042    0.608 / 0.031
        360 x 640 HDR seed 1234   0.721 / 0.039    0.767 / 0.032    0.754 / 0.036
        360 x 640 SDR seed 7      0.741 / 0.063    0.773 / 0.042    0.764 / 0.038
    The smallest gap is 0.577: 0.5 leaves room for nothing but a broken model."""
    import quality_ssim_cases as qsc
    rows = qsc.oracle_ssim_pairs(hdr, H, W, seed, 16)
    assert [r["pair"] for r in rows] == [1, 2, 3]
    for r in rows:
        a, b = qsc.mean(r["interpolated"]["Y"]), qsc.mean(r["repeat"]["Y"])
        print(f"pair {r['pair']}: interpolation {a:.3f}, repeat {b:.3f}, gap {a - b:.3f}")
        assert r["oob"] == 0 and r["interpolated"]["Y"]["count"] == (W // 4 - 1) * (H // 4 - 1)
        assert a - b >= 0.5, (r["pair"], a, b)
