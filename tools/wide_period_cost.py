"""Periods of more than six outputs through a batch (hf_batch_run_period_wide): what the chunked fused launches buy.

    python tools/wide_period_cost.py [--members 12] [--n-out 10] [--periods 200] [--warmup 20] [--rounds 3] [--out FILE]

At 1080p SDR and 2160p HDR, one batch of `--members` members, `--n-out` outputs per member and period (10: 23.976 fps -> 240 Hz), two ways
to the same frames alternating `--rounds` times in one process on one box:
  * wide          hf_batch_run_period_wide: update, chain and the period's warps in chunks of six outputs, each ONE fused launch;
  * member_by_member
                  what a host had before the wide calls: hf_batch_run_period for update and chain, then hf_interpolate_period_ex
                  (update_and_flow = 0) of every member on the batch stream -- per member a fused launch per six outputs.
Wall time per period over `--periods` periods after `--warmup` (one sync at the end), every round of both, so the run-to-run spread stands
beside the difference.  The leader carries HF_FLAG_BATCH_EAGER_PLANES on both sides: without the batch's own warps a deferring batch would
build its planes with the stand-alone kernel anyway.  Prints one JSON object.
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
from hopperrender_amd.calc import DeviceBuffer, FlowBatch, OpticalFlowCalcHDR, OpticalFlowCalcSDR  # noqa: E402

SIZES = (("1080p_sdr", 1080, 1920, False), ("2160p_hdr", 2160, 3840, True))


def one_size(H, W, hdr, n, n_out, periods, warmup, rounds):
    cls = OpticalFlowCalcHDR if hdr else OpticalFlowCalcSDR
    sc = synth.Scene(H, W, hdr, 3)
    pool = []
    for k in range(6):     # the bench's ping-pong pool
        f = sc.frame(k)
        b = DeviceBuffer(f.nbytes)
        b.upload(f)
        pool.append(b)
    order = [0, 1, 2, 3, 4, 5, 4, 3, 2, 1]
    ts = [(i + 1) / (n_out + 1) for i in range(n_out)]

    def make(wide):
        ms = [cls(H, W, search_radius=16, flags=capi.HF_FLAG_ASYNC | capi.HF_FLAG_NO_TIMING | (capi.HF_FLAG_BATCH_EAGER_PLANES if i == 0 else 0))
              for i in range(n)]
        b = FlowBatch(ms)
        outs = [[DeviceBuffer(ms[0].output_frame_bytes) for _ in range(n_out)] for _ in range(n)]
        ptrs = [[x.ptr for x in o] for o in outs]
        if wide:
            prepared = [b.preparePeriod([pool[j].ptr] * n, [ts] * n, ptrs, 2) for j in range(6)]
        else:
            prepared = [b.preparePeriod([pool[j].ptr] * n, None, None, 2) for j in range(6)]
        return ms, b, outs, prepared, ptrs

    def run(side, wide, count, k0=0):
        ms, b, outs, prepared, ptrs = side
        for k in range(count):
            b.runPeriod(prepared[order[(k0 + k) % len(order)]])
            if not wide:
                for m, c in enumerate(ms):
                    c.interpolateOnly(ts, ptrs[m], 2)
        b.sync()

    sides = {"wide": make(True), "member_by_member": make(False)}
    wall = {k: [] for k in sides}
    for name, side in sides.items():
        run(side, name == "wide", warmup)
    for _ in range(rounds):
        for name, side in sides.items():
            t0 = time.perf_counter()
            run(side, name == "wide", periods, warmup)
            wall[name].append((time.perf_counter() - t0) / periods * 1e6)
    picks = sorted({0, min(6, n_out - 1), n_out - 1})     # an output of the first chunk, the first of the second, the last
    same = all(np.array_equal(ra[i].download(np.uint8), rb[i].download(np.uint8))
               for ra, rb in zip(sides["wide"][2], sides["member_by_member"][2]) for i in picks)
    for ms, b, outs, _, _ in sides.values():
        b.close()
        for m in ms:
            m.close()
        for o in outs:
            for x in o:
                x.free()
    for x in pool:
        x.free()
    res = {"members": n, "n_out": n_out, "same_outputs": bool(same),
           "wall_us_per_period": {k: [round(x, 1) for x in v] for k, v in wall.items()},
           "wall_median_us": {k: round(float(np.median(v)), 1) for k, v in wall.items()},
           "spread_us": {k: round(max(v) - min(v), 1) for k, v in wall.items()}}
    res["member_by_member_over_wide"] = round(res["wall_median_us"]["member_by_member"] / res["wall_median_us"]["wide"], 3)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--members", type=int, default=12)
    ap.add_argument("--n-out", type=int, default=10)
    ap.add_argument("--periods", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {}
    for name, H, W, hdr in SIZES:
        res[name] = one_size(H, W, hdr, a.members, a.n_out, a.periods, a.warmup, a.rounds)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
