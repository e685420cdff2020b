"""Planar 4:2:0 clips through a batch (HF_FLAG_BATCH_PLANAR_IN | HF_FLAG_BATCH_PLANAR_OUT): what the two re-layout launches cost.

    python tools/batch_planar_cost.py [--members 12] [--n-out 5] [--periods 200] [--warmup 20] [--rounds 3] [--out FILE]

At 1080p SDR and 2160p HDR, one batch of `--members` members, `--n-out` outputs per member and period, a planar batch and a plain one
alternating `--rounds` times in one process on one box:
  * wall time per period of hf_batch_run_period over `--periods` periods after `--warmup` (one sync at the end), every round of both, so
    the plain batch's run-to-run spread stands beside the difference;
  * device durations of planar_in_batch / planar_out_batch from the batch timeline (hf_batch_timeline_enable: 8 recorded periods), the
    bytes each moves (a read and a write of every frame it converts) and the GB/s beside this box's streaming-copy probe
    (hf_hbm_copy_probe).
Prints one JSON object.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from hopperrender_amd import capi, synth  # noqa: E402
from hopperrender_amd.calc import DeviceBuffer, FlowBatch, OpticalFlowCalcHDR, OpticalFlowCalcSDR  # noqa: E402

SIZES = (("1080p_sdr", 1080, 1920, False), ("2160p_hdr", 2160, 3840, True))
T = [0.1988, 0.3996, 0.5984, 0.7992, 0.998, 0.5]


def one_size(H, W, hdr, n, n_out, periods, warmup, rounds):
    cls = OpticalFlowCalcHDR if hdr else OpticalFlowCalcSDR
    sc = synth.Scene(H, W, hdr, 3)
    pool = []
    for k in range(6):     # the bench's ping-pong pool; the bytes' layout does not change what a launch costs
        f = sc.frame(k)
        b = DeviceBuffer(f.nbytes)
        b.upload(f)
        pool.append(b)
    order = [0, 1, 2, 3, 4, 5, 4, 3, 2, 1]

    def make(planar):
        lead = (capi.HF_FLAG_BATCH_PLANAR_IN | capi.HF_FLAG_BATCH_PLANAR_OUT) if planar else 0
        ms = [cls(H, W, search_radius=16, flags=capi.HF_FLAG_ASYNC | capi.HF_FLAG_NO_TIMING | (lead if i == 0 else 0)) for i in range(n)]
        b = FlowBatch(ms)
        outs = [[DeviceBuffer(ms[0].output_frame_bytes) for _ in range(n_out)] for _ in range(n)]
        prepared = [b.preparePeriod([pool[j].ptr] * n, [T[:n_out]] * n, [[x.ptr for x in o] for o in outs], 2) for j in range(6)]
        return ms, b, outs, prepared

    def run(b, prepared, count, k0=0):
        for k in range(count):
            b.runPeriod(prepared[order[(k0 + k) % len(order)]])
        b.sync()

    sides = {"plain": make(False), "planar": make(True)}
    wall = {"plain": [], "planar": []}
    for name, (ms, b, outs, prepared) in sides.items():
        run(b, prepared, warmup)
    for _ in range(rounds):
        for name, (ms, b, outs, prepared) in sides.items():
            t0 = time.perf_counter()
            run(b, prepared, periods, warmup)
            wall[name].append((time.perf_counter() - t0) / periods * 1e6)
    # device durations of the two launches: 8 recorded periods of the planar batch
    ms, b, outs, prepared = sides["planar"]
    b.timelineEnable(8 * 34 + 40, 0)
    run(b, prepared, 8, warmup)
    recs = b.timelineRead()
    b.timelineEnable(0)
    dur = {k: [1e3 * (e - s) for (nm, p, s, e) in recs if nm == k] for k in ("planar_in_batch", "planar_out_batch")}
    defers = b.defersPlanes()
    in_bytes, out_bytes = ms[0].input_frame_bytes, ms[0].output_frame_bytes
    for name, (ms_, b_, outs_, _) in sides.items():
        b_.close()
        for m in ms_:
            m.close()
        for o in outs_:
            for x in o:
                x.free()
    for x in pool:
        x.free()
    moved = {"planar_in_batch": 2 * in_bytes * n, "planar_out_batch": 2 * out_bytes * n * n_out}
    res = {"members": n, "n_out": n_out, "defers_planes": defers,
           "wall_us_per_period": {k: [round(x, 1) for x in v] for k, v in wall.items()},
           "wall_median_us": {k: round(float(np.median(v)), 1) for k, v in wall.items()},
           "plain_spread_us": round(max(wall["plain"]) - min(wall["plain"]), 1)}
    res["planar_over_plain_rate"] = round(res["wall_median_us"]["plain"] / res["wall_median_us"]["planar"], 3)
    for k, v in dur.items():
        med = float(np.median(v)) if v else float("nan")
        res[k] = {"records": len(v), "median_us": round(med, 1), "min_us": round(min(v), 1) if v else None, "max_us": round(max(v), 1) if v else None,
                  "bytes": moved[k], "GBps": round(moved[k] / (med * 1e-6) / 1e9, 1) if v else None}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--members", type=int, default=12)
    ap.add_argument("--n-out", type=int, default=5)
    ap.add_argument("--periods", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    gbps = C.c_double()
    capi.check(capi.load().hf_hbm_copy_probe(0, 512 << 20, 5, C.byref(gbps)))
    res = {"hbm_copy_probe_GBps": round(gbps.value, 1)}
    for name, H, W, hdr in SIZES:
        res[name] = one_size(H, W, hdr, a.members, a.n_out, a.periods, a.warmup, a.rounds)
        for k in ("planar_in_batch", "planar_out_batch"):
            if res[name][k]["GBps"]:
                res[name][k]["share_of_copy_probe"] = round(res[name][k]["GBps"] / gbps.value, 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
