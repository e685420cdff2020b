"""Guarded blend on the device (hf_guarded_blend_enqueue, csrc/hf_kernels.hip): what an output costs, beside the two launches the call
is made of -- the warp disagreement maps, and the plain blended outputs of the same period.

    python tools/guarded_blend_rate.py [--launches 40] [--readings 7] [--out FILE]

Per case -- 3840 x 2160 HDR and 1920 x 1080 SDR -- one asynchronous context, three frames of a moving synth.Scene submitted by device
reference and one flow calculated; that flow is copied into the slot the warps read (the previous flow), so the gathers are displaced
the way a clip displaces them.  The outputs are the five of 24 -> 120 fps (t = 0, .2, .4, .6, .8), each into a buffer of its own, at
tile 16.  Timed side by side, taking turns within every one of the `--readings` rounds (tools/metrics_rate_common.py: the library's own
events around `--launches` back-to-back repetitions after a warm-up, medians reported):
    disagreement   hf_warp_disagreement_map_enqueue for the five t's: the call's first launch on its own
    period         hf_interpolate_period in mode 2 for the same five outputs, no new frame: the plain blend
    guard_off      the new call with (4080, 4081): no tile fires, no store group loads the cross-fade
    guard_half     ... with lo = the median of the tiles' mean differences, hi = lo + 1: about half the tiles at weight 256
    guard_all      ... with (0, 1): every tile fires, every store group loads the cross-fade
With F the bytes of a frame the disagreement launch gathers 2 F per t, the period writes F per t and gathers 2 F once or more, and the
blend launch behind the disagreement launch gathers 2 F and writes F per t, 2 F more where the cross-fade is loaded.  Reported per
kernel: microseconds per t; per guard setting also its time over disagreement + period, the two existing launches that make the same
maps and plain frames.  No threshold is set in advance.  Before the buffers go, guard_off is compared with the period's frames and
guard_all's maps with the disagreement launch's, byte for byte.
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

from metrics_rate_common import CASES, parse_args, probe, timed  # noqa: E402

from hopperrender_amd import capi, synth  # noqa: E402
from hopperrender_amd.calc import DeviceBuffer, OpticalFlowCalcHDR, OpticalFlowCalcSDR, frame_error_maps, guard_weights  # noqa: E402

TILE = 16
TS = [0.0, 0.2, 0.4, 0.6, 0.8]
GUARD_OFF, GUARD_ALL = (4080, 4081), (0, 1)


def case(H, W, hdr, launches, readings):
    c = (OpticalFlowCalcHDR if hdr else OpticalFlowCalcSDR)(H, W, search_radius=8, flags=capi.HF_FLAG_ASYNC)
    bufs = []

    def buffer(nbytes):
        bufs.append(DeviceBuffer(nbytes))
        return bufs[-1]
    try:
        F, n = int(c.input_frame_bytes), len(TS)
        sc = synth.Scene(H, W, hdr, 42)
        for k in range(3):
            f = sc.frame(k)
            b = buffer(f.nbytes)
            b.upload(f)
            c.updateFrameDeviceRef(b.ptr)
        c.calculateOpticalFlow()
        c.sync()
        flow = c.readBlurredFlow(1)
        c.writeBlurredFlow(0, flow)
        tw, th, map_bytes = c.frameErrorMapShape(TILE)
        outs = {k: [buffer(int(c.output_frame_bytes)) for _ in TS] for k in ("period", "guard")}
        maps = {k: buffer(n * map_bytes) for k in ("disagreement", "guard")}
        ptrs = lambda k: [b.ptr for b in outs[k]]
        # the thresholds of guard_half from the maps themselves
        c.warpDisagreementMapEnqueue(TS, TILE, maps["disagreement"].ptr)
        c.sync()
        dis = frame_error_maps(maps["disagreement"].download(np.uint8), n, tw, th)
        cnt = np.minimum(TILE, H - TILE * np.arange(th))[:, None] * np.minimum(TILE, W - TILE * np.arange(tw))[None, :]
        m = (16 * dis["sad"][:, 0].astype(np.int64)) // (cnt << (8 if hdr else 0))
        half = (int(np.median(m)), int(np.median(m)) + 1)
        guards = {"guard_off": GUARD_OFF, "guard_half": half, "guard_all": GUARD_ALL}
        enqueues = {"disagreement": lambda: c.warpDisagreementMapEnqueue(TS, TILE, maps["disagreement"].ptr),
                    "period": lambda: c.interpolateOnly(TS, ptrs("period"), 2)}
        for k, (lo, hi) in guards.items():
            enqueues[k] = lambda lo=lo, hi=hi: c.guardedBlendEnqueue(TS, TILE, lo, hi, maps["guard"].ptr, ptrs("guard"))
        us = timed(c, enqueues, launches, readings)
        r = {"frame_bytes": F, "outputs": n, "tile": TILE, "res_scalar": int(c.m_opticalFlowResScalar),
             "flow_nonzero_share": round(float(np.count_nonzero(flow)) / flow.size, 3), "guard_half_thresholds_q4": list(half)}
        for k, v in us.items():
            r[k] = {"us_per_t_best": round(v[0] / n, 2), "us_per_t_median": round(v[len(v) // 2] / n, 2)}
        both = r["disagreement"]["us_per_t_median"] + r["period"]["us_per_t_median"]
        for k, (lo, hi) in guards.items():
            wt, _ = guard_weights(dis, TILE, lo, hi, H, W, hdr)
            r[k]["tiles_firing_share"] = round(float(np.count_nonzero(wt)) / wt.size, 3)
            r[k]["over_disagreement_plus_period_median"] = round(r[k]["us_per_t_median"] / both, 3)
            r[k]["blend_launches_us_per_t_median"] = round(r[k]["us_per_t_median"] - r["disagreement"]["us_per_t_median"], 2)
        # what was timed is what the definition says
        c.guardedBlendEnqueue(TS, TILE, *GUARD_OFF, maps["guard"].ptr, ptrs("guard"))
        c.interpolateOnly(TS, ptrs("period"), 2)
        c.sync()
        dt, so, rows = (np.uint16 if hdr else np.uint8), int(c.output_frame_bytes) // ((2 if hdr else 1) * (H + H // 2)), H + H // 2
        for a, b in zip(outs["guard"], outs["period"]):
            assert np.array_equal(a.download(dt).reshape(rows, so)[:, :W], b.download(dt).reshape(rows, so)[:, :W])
        assert np.array_equal(maps["guard"].download(np.uint8), maps["disagreement"].download(np.uint8))
        return r
    finally:
        c.close()
        for b in bufs:
            b.free()


def main():
    a = parse_args(__doc__)
    res = {"hbm_copy_probe_GBps_before": round(probe(), 1)}
    for name, H, W, hdr, _ in CASES:
        res[name.rsplit("_", 2)[0]] = case(H, W, hdr, a.launches, a.readings)
    res["hbm_copy_probe_GBps_after"] = round(probe(), 1)
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
