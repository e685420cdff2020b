"""Whole clips through a batch that defers its phase planes (HF_FLAG_BATCH_AUTO_DEFERRED): what scene-cut handling costs on the headline path.

    python tools/auto_deferred_cost.py [--members 12] [--n-out 5] [--periods 100] [--warmup 20] [--rounds 5] [--radius 16] [--out FILE]

One batch of `--members` members of 2160p HDR, `--n-out` outputs per member and period (5: 24 fps -> 120 Hz), frames resident on the
device, steady state after `--warmup` periods.  Three paths to the same frames, alternating `--rounds` times in one process on one box:
  * a_plain_deferred   hf_batch_run_period on the deferring batch: the path bench.py times, no scene-cut handling;
  * b_auto_eager       hf_batch_run_period_auto on the HF_FLAG_BATCH_EAGER_PLANES twin: the only way before the flag -- every period pays
                       the stand-alone plane kernel;
  * c_auto_deferred    hf_batch_run_period_auto on the deferring batch whose leader carries HF_FLAG_BATCH_AUTO_DEFERRED.
Each on two clips: `bench` (bench.py's default scene, its pool of six frames walked 0 .. 5 .. 0: every pair is a pair of consecutive
frames) and `cut6` (the six frames, then the same six upside down, and again: a hard cut every sixth pair).  Wall time over `--periods`
periods with one sync at the end, as output frames per second: every round of every path, and min / median / max, so the run-to-run
spread stands beside the differences.  The yardstick of (c) is (b) of the same call.  Outputs of (b) and (c) are compared at the end.
Prints one JSON object.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from hopperrender_amd import capi, synth  # noqa: E402
from hopperrender_amd.calc import DeviceBuffer, FlowBatch, OpticalFlowCalcHDR  # noqa: E402

H, W = 2160, 3840
SOURCE_24 = 417083
PATHS = {"a_plain_deferred": 0, "b_auto_eager": capi.HF_FLAG_BATCH_EAGER_PLANES, "c_auto_deferred": capi.HF_FLAG_BATCH_AUTO_DEFERRED}


def upside_down(f):
    a = f.reshape(H + H // 2, W)
    return np.ascontiguousarray(np.concatenate([a[:H][::-1], a[H:][::-1]])).reshape(-1)


def run_all(n, n_out, periods, warmup, rounds, radius):
    sc = synth.Scene(H, W, True, 1234)
    pool = []
    host = [sc.frame(k) for k in range(6)]
    for f in host + [upside_down(f) for f in host]:
        b = DeviceBuffer(f.nbytes)
        b.upload(f)
        pool.append(b)
    orders = {"bench": [0, 1, 2, 3, 4, 5, 4, 3, 2, 1], "cut6": list(range(12))}
    ts = [(i + 1) / (n_out + 1) for i in range(n_out)]

    def make(name):
        ms = [OpticalFlowCalcHDR(H, W, search_radius=radius, flags=capi.HF_FLAG_ASYNC | capi.HF_FLAG_NO_TIMING | (PATHS[name] if i == 0 else 0)) for i in range(n)]
        b = FlowBatch(ms)
        assert b.defersPlanes() == (name != "b_auto_eager")
        outs = [[DeviceBuffer(ms[0].output_frame_bytes) for _ in range(n_out)] for _ in range(n)]
        prepared = [b.preparePeriod([x.ptr] * n, [ts] * n, [[x.ptr for x in o] for o in outs], 2) for x in pool]
        return ms, b, outs, prepared

    def arm(side):
        ms, b, _, _ = side
        for i, m in enumerate(ms):
            m.m_frameCount = 0
            b.sceneSet(i, SOURCE_24, -1)

    def run(name, side, order, count, k0):
        ms, b, outs, prepared = side
        auto = name != "a_plain_deferred"
        kinds = 0
        for k in range(count):
            p = prepared[order[(k0 + k) % len(order)]]
            if auto:
                frames, _, counts, t, o, mode = p
                if k and k % 100 == 0:     # the record ring holds 128 periods
                    b.sync()
                    kinds += sum(1 - r["kind"] for r in b.sceneRead(0))
                rc = b._lib.hf_batch_run_period_auto(b._b, frames, counts, t, o, mode, None)
                if rc:
                    b._check(rc)
            else:
                b.runPeriod(p)
        b.sync()
        if auto:
            kinds += sum(1 - r["kind"] for r in b.sceneRead(0))
            for i in range(1, n):
                b.sceneRead(i)
        return kinds

    sides = {name: make(name) for name in PATHS}
    res = {"members": n, "n_out": n_out, "periods": periods, "warmup": warmup, "rounds": rounds, "search_radius": radius, "clips": {}}
    for clip, order in orders.items():
        fps = {name: [] for name in PATHS}
        copies = {}
        for name, side in sides.items():
            if name != "a_plain_deferred":
                arm(side)
            run(name, side, order, warmup, 0)
        for _ in range(rounds):
            for name in ("b_auto_eager", "c_auto_deferred", "a_plain_deferred"):
                t0 = time.perf_counter()
                copies[name] = run(name, sides[name], order, periods, warmup)
                fps[name].append(n * n_out * periods / (time.perf_counter() - t0))
        same = all(np.array_equal(x.download(np.uint8), y.download(np.uint8))
                   for rb, rc in zip(sides["b_auto_eager"][2], sides["c_auto_deferred"][2]) for x, y in ((rb[0], rc[0]), (rb[-1], rc[-1])))
        stat = lambda v: {"min": round(min(v), 1), "median": round(float(np.median(v)), 1), "max": round(max(v), 1)}
        res["clips"][clip] = {"frames_per_s": {k: [round(x, 1) for x in v] for k, v in fps.items()},
                              "summary": {k: stat(v) for k, v in fps.items()},
                              "copy_periods_of_member_0_in_the_last_round": {k: v for k, v in copies.items() if k != "a_plain_deferred"},
                              "b_and_c_same_outputs": bool(same),
                              "c_median_above_b_max": bool(np.median(fps["c_auto_deferred"]) > max(fps["b_auto_eager"]))}
    for ms, b, outs, _ in sides.values():
        b.close()
        for m in ms:
            m.close()
        for o in outs:
            for x in o:
                x.free()
    for x in pool:
        x.free()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--members", type=int, default=12)
    ap.add_argument("--n-out", type=int, default=5)
    ap.add_argument("--periods", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--radius", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not 1 <= a.n_out <= capi.HF_MAX_PERIOD_OUTPUTS:
        ap.error("--n-out must be in [1, 6]: the tool times the narrow calls")
    line = json.dumps(run_all(a.members, a.n_out, a.periods, a.warmup, a.rounds, a.radius))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
