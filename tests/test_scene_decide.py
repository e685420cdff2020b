"""CPU: the scene-change decision of csrc/hf_scene.h -- what the scene_decide kernel runs per batch member (hf_batch_run_period_auto) --
against the filter it restates: hf_filter_push_frame_delta / hf_filter_detect_scene_change / hf_filter_get_state of the built library
(csrc/hf_filter.cpp:130-161), record for record.  tests/scene_probe.cpp is compiled with plain g++ against the header, like
tests/launch_plan_probe.cpp (no ROCm include path: the header is HIP-free).

The header keeps a ring of at most 12 deltas and takes the filter's 3-second window as a cap on the number held
(scene_history_cap = min(12, frames_in_3s + 1)); the filter keeps a deque keyed by m_frameCount.  The two agree while pushes are
consecutive in m_frameCount, which is what a batch member's periods are."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hopperrender_amd", "csrc")
SOURCE_TIMES = {417083: 71, 3333333: 9, 10000000: 3, 15000000: 2, 30000001: 0}   # source_frame_time -> frames_in_3s


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("scene_probe") / "libscene_probe.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I", CSRC,
                           os.path.join(ROOT, "tests", "scene_probe.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.hsp_new.restype = ctypes.c_void_p
    lib.hsp_free.argtypes = [ctypes.c_void_p]
    lib.hsp_clear.argtypes = [ctypes.c_void_p]
    lib.hsp_cap.argtypes = [ctypes.c_longlong]
    lib.hsp_held.argtypes = [ctypes.c_void_p]
    lib.hsp_push.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32, ctypes.POINTER(ctypes.c_int)]
    lib.hsp_push_many.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_int, ctypes.c_int, ctypes.c_uint32,
                                  ctypes.POINTER(ctypes.c_int)]
    return lib


class Header:
    """One member's state in the header's terms."""

    def __init__(self, lib, source_frame_time=417083, threshold=200):
        self.lib, self.s = lib, ctypes.c_void_p(lib.hsp_new())
        self.cap, self.thr = lib.hsp_cap(source_frame_time), threshold

    def push(self, delta):
        out = (ctypes.c_int * 4)()
        self.lib.hsp_push(self.s, delta, self.cap, self.thr, out)
        return tuple(out)   # kind (1 warp / 0 copy), average, d1, d2

    def push_many(self, deltas):
        a = (ctypes.c_uint32 * len(deltas))(*deltas)
        out = (ctypes.c_int * (4 * len(deltas)))()
        self.lib.hsp_push_many(self.s, a, len(deltas), self.cap, self.thr, out)
        return [tuple(out[4 * i:4 * i + 4]) for i in range(len(deltas))]

    def clear(self):
        self.lib.hsp_clear(self.s)

    def close(self):
        self.lib.hsp_free(self.s)


class Filter:
    """The same member in the filter's terms: push + detect + the read-outs of the last decision."""

    def __init__(self, source_frame_time=417083, threshold=200, first_frame_count=3):
        from hopperrender_amd.protocol import NativeFilter
        self.f = NativeFilter(source_frame_time, 166667, 2, threshold)
        self.count = first_frame_count   # m_frameCount of the first period that has a flow (HopperRender.cpp:955)

    def push(self, delta):
        self.f.push(self.count, delta)
        cut = self.f.detect(self.count)
        self.count += 1
        st = self.f.state()
        return (0 if cut else 1, st["average_frame_delta"], st["scene_change_delta1"], st["scene_change_delta2"])

    def new_segment(self, first_frame_count=3):
        self.f.new_segment(1.0)
        self.count = first_frame_count

    def close(self):
        self.f.close()


def both(probe, deltas, source_frame_time=417083, threshold=200):
    """The decisions of the header for a sequence, checked record for record against the filter's."""
    h, f = Header(probe, source_frame_time, threshold), Filter(source_frame_time, threshold)
    got = [h.push(d) for d in deltas]
    want = [f.push(d) for d in deltas]
    h.close(); f.close()
    assert got == want, (deltas, source_frame_time, threshold, got, want)
    return got


def test_probe_compiles_without_rocm_and_caps_follow_the_window(native_lib, probe):
    assert probe.hsp_history() == 12
    for sft, in_3s in SOURCE_TIMES.items():
        assert int(3.0 * 10000000.0 / sft) == in_3s
        assert probe.hsp_cap(sft) == min(12, in_3s + 1)


def test_fewer_than_three_deltas_never_cut(native_lib, probe):
    # hf_filter.cpp:143 (n < 3): no decision, the read-outs keep their last values (0 on a new filter)
    assert both(probe, [100, 5000]) == [(1, 0, 0, 0), (1, 0, 0, 0)]
    # ... whatever the threshold, 0 included
    assert both(probe, [7, 9], threshold=0) == [(1, 0, 0, 0), (1, 0, 0, 0)]


def test_history_shorter_than_ten_averages_what_it_has(native_lib, probe):
    # :144 count = min(n - 2, 10); :146-147 the average runs over deltas[n - 2 - i]: the current one included, the next one not
    got = both(probe, [100, 100, 100, 1000, 100])
    assert got[2] == (1, 100, 0, 0)            # n = 3: one delta averaged (the current one itself)
    assert got[3] == (1, 100, 0, -900)         # n = 4: the spike is "next"
    assert got[4] == (0, 400, 600, 900)        # n = 5: the spike is current; (1000 + 100 + 100) / 3 = 400
    # ten and more: the window of the average stops growing (14 deltas: count stays 10)
    seq = [100] * 12 + [1300, 100]
    assert both(probe, seq)[-1] == (0, 220, 1080, 1200)   # (1300 + 9 * 100) / 10


def test_second_difference_must_be_positive(native_lib, probe):
    # :160 d2 > 0: a delta that stays high (d2 == 0) or keeps rising (d2 < 0) is no cut
    assert both(probe, [100, 100, 1000, 1000])[-1] == (1, 550, 450, 0)
    assert both(probe, [100, 100, 1000, 2000])[-1] == (1, 550, 450, -1000)
    # ... even at threshold 0, where (uint32)d2 >= thr holds for every d2
    assert both(probe, [100, 100, 1000, 1000], threshold=0)[-1] == (1, 550, 450, 0)


def test_differences_exactly_at_the_threshold_and_one_below(native_lib, probe):
    # :160 (uint32)d1 >= thr && (uint32)d2 >= thr
    assert both(probe, [0, 0, 400, 200], threshold=200)[-1] == (0, 200, 200, 200)   # both exactly at it
    assert both(probe, [0, 0, 400, 200], threshold=201)[-1] == (1, 200, 200, 200)   # both one below
    assert both(probe, [0, 0, 398, 100], threshold=200)[-1] == (1, 199, 199, 298)   # d1 one below
    assert both(probe, [0, 0, 400, 201], threshold=200)[-1] == (1, 200, 200, 199)   # d2 one below


def test_thresholds_zero_one_and_int_max(native_lib, probe):
    # :159-160 threshold 0: any d1 > 0 and d2 > 0 cuts; 1: the same (integers); 2^31 - 1: only differences of exactly that size
    for thr, kind in ((0, 0), (1, 0), (2, 1), (2 ** 31 - 1, 1)):
        assert both(probe, [0, 0, 2, 1], threshold=thr)[-1] == (kind, 1, 1, 1), thr
    big = 2 ** 31 - 1
    assert both(probe, [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, big, 0], threshold=big)[-1][0] == 1     # d1 = big - big / 10 < thr
    # current = (int)(2^32 - 2) = -2, average 2^31 - 1: d1 = -2 - (2^31 - 1) wraps to 2^31 - 1 -- at the threshold, and positive -- but d2 = -2
    assert both(probe, [0, 0, 2 * big, 0], threshold=big)[-1] == (1, big, big, -2)


def test_deltas_at_and_above_two_to_the_31(native_lib, probe):
    # :148 (int) casts of the deltas go negative at 2^31; :145-147 the sum stays exact in unsigned long long
    top = 2 ** 31
    got = both(probe, [top, top, top, top])
    assert got[-1] == (1, -top, 0, 0)                       # average (int)2^31 = INT_MIN, current the same: d1 = d2 = 0
    got = both(probe, [5, 5, top + 7, 5])
    assert got[-1][0] in (0, 1) and got[-1][3] == (top + 7 - 5) - 2 ** 32   # current - next wraps into the negative range: no d2 > 0
    assert got[-1][0] == 1
    both(probe, [2 ** 32 - 1] * 13)                         # ten times 2^32 - 1 does not overflow the sum
    both(probe, [3000, 2 ** 32 - 1, 3000, top, 0, top - 1, top, top + 1, 3000])


def test_rearm_in_mid_sequence_starts_the_history_over(native_lib, probe):
    # hf_filter.cpp:40-46 (NewSegment): the deque is cleared, the read-outs of the last decision stay
    h, f = Header(probe), Filter()
    for d in (100, 100, 1000, 100):
        assert h.push(d) == f.push(d)
    assert h.push(100) == f.push(100) and probe.hsp_held(h.s) == 5
    h.clear(); f.new_segment()
    assert probe.hsp_held(h.s) == 0
    after = [(h.push(d), f.push(d)) for d in (3000, 3001, 9000, 3000, 3000)]
    assert all(a == b for a, b in after), after
    assert after[0][0] == after[1][0] == (1, 400, -300, 0)   # fewer than 3 again: no stale delta decides, the old read-outs are shown
    assert after[3][0][0] == 0                                # the new clip's own spike is found
    h.close(); f.close()


@pytest.mark.parametrize("source_frame_time", sorted(SOURCE_TIMES))
def test_random_sequences_match_the_filter(native_lib, probe, source_frame_time):
    """500 sequences of 40 deltas per source frame time (2500 in all), threshold and value mix drawn per sequence; one re-arm in the
    middle of every fourth."""
    rng = np.random.default_rng(source_frame_time)
    cuts = 0
    for seq in range(500):
        thr = int(rng.choice([0, 1, 50, 200, 201, 1000, 2 ** 31 - 1]))
        kind = rng.integers(0, 4)
        base = rng.integers(0, 2 ** 32, size=40, dtype=np.uint64)
        if kind == 0:
            vals = rng.choice([0, 1, 2, 3, 199, 200, 201, 400], size=40)
        elif kind == 1:
            vals = 3000 + rng.integers(-150, 151, size=40)
            spikes = rng.random(40) < 0.15
            vals = np.where(spikes, vals + rng.integers(150, 1500, size=40), vals)
        elif kind == 2:
            vals = np.where(rng.random(40) < 0.5, base | (1 << 31), rng.integers(0, 5000, size=40))
        else:
            vals = np.where(rng.random(40) < 0.3, 0, np.where(rng.random(40) < 0.5, base, 3000 + rng.integers(0, 800, size=40)))
        deltas = [int(v) & 0xFFFFFFFF for v in vals]
        h, f = Header(probe, source_frame_time, thr), Filter(source_frame_time, thr)
        rearm = 17 if seq % 4 == 0 else None
        if rearm is None:
            got = h.push_many(deltas)
        else:
            got = h.push_many(deltas[:rearm])
            h.clear()
            got += h.push_many(deltas[rearm:])
        want = []
        for i, d in enumerate(deltas):
            if i == rearm:
                f.new_segment(first_frame_count=3)
            want.append(f.push(d))
        h.close(); f.close()
        assert got == want, (seq, thr, deltas, [i for i in range(40) if got[i] != want[i]][:3])
        cuts += sum(1 for r in got if r[0] == 0)
    if SOURCE_TIMES[source_frame_time] < 3:
        assert cuts == 0          # frames_in_3s 0: never 3 deltas held; 2: exactly 3, the average is the current delta itself and d1 == 0
    else:
        assert cuts > 50          # the mix does exercise the cut branch
