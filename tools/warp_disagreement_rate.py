"""Warp disagreement maps on the device (hf_warp_disagreement_map_enqueue, csrc/hf_kernels.hip): what an output costs, beside the three
launches that compose the same map.

    python tools/warp_disagreement_rate.py [--launches 40] [--readings 7] [--out FILE]

Per case -- 3840 x 2160 HDR and 1920 x 1080 SDR -- one asynchronous context, three frames of a moving synth.Scene submitted by device
reference and one flow calculated; that flow is copied into the slot the warps read (the previous flow), so the gathers are displaced
the way a clip displaces them.  Timed side by side, taking turns within every one of the `--readings` rounds (tools/metrics_rate_common.py:
the library's own events around `--launches` back-to-back repetitions after a warm-up, medians reported), at tile 16 and tile 64:
    composed   per t three launches: the warp with output mode 0 into one buffer, with mode 1 into another, the error map of the two
    fused      the new call, one launch for all t's
each at n_t = 1 (t = 0.5) and at n_t = 5 with the blending scalars of 24 -> 120 fps (0, .2, .4, .6, .8).  With F the bytes of a frame the
composition moves 6 F per t through HBM (each warp gathers one frame, F, and writes one, F; the error map reads both outputs, 2 F) and
the fused launch gathers 2 F; both write 48 bytes per tile and t.  Reported per kernel:
microseconds per t, GB/s of those bytes and their share of this box's streaming-copy probe (hf_hbm_copy_probe, before and after), and
fused over composed.  Before the buffers go, the fused maps are compared with the composed ones, byte for byte.
ACCEPTANCE (asserted): the median time per t of `fused` is not above that of `composed`, in both cases, at both n_t and both tiles.
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

from metrics_rate_common import CASES, parse_args, probe, timed  # noqa: E402

from hopperrender_amd import capi, synth  # noqa: E402
from hopperrender_amd.calc import DeviceBuffer, OpticalFlowCalcHDR, OpticalFlowCalcSDR  # noqa: E402

MAP_TILES = (16, 64)
T_SETS = {1: [0.5], 5: [0.0, 0.2, 0.4, 0.6, 0.8]}


def case(H, W, hdr, launches, readings):
    c = (OpticalFlowCalcHDR if hdr else OpticalFlowCalcSDR)(H, W, search_radius=8, flags=capi.HF_FLAG_ASYNC)
    bufs = []

    def buffer(nbytes):
        bufs.append(DeviceBuffer(nbytes))
        return bufs[-1]
    try:
        F = int(c.input_frame_bytes)
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
        out = [buffer(int(c.output_frame_bytes)) for _ in range(2)]
        shapes = {t: c.frameErrorMapShape(t) for t in MAP_TILES}
        maps = {(k, t, n): buffer(n * shapes[t][2]) for k in ("composed", "fused") for t in MAP_TILES for n in T_SETS}

        def composed(ts, tile, dst):
            for i, t in enumerate(ts):
                c.interpolateOnly([t], [out[0].ptr], 0)
                c.interpolateOnly([t], [out[1].ptr], 1)
                c.frameErrorMapEnqueue([out[0].ptr], [out[1].ptr], tile, dst + i * shapes[tile][2])

        enqueues = {}
        for tile in MAP_TILES:
            for n, ts in T_SETS.items():
                enqueues[f"composed_tile{tile}_nt{n}"] = lambda ts=ts, tile=tile, n=n: composed(ts, tile, maps[("composed", tile, n)].ptr)
                enqueues[f"fused_tile{tile}_nt{n}"] = lambda ts=ts, tile=tile, n=n: c.warpDisagreementMapEnqueue(ts, tile, maps[("fused", tile, n)].ptr)
        us = timed(c, enqueues, launches, readings)
        r = {"frame_bytes": F, "flow_nonzero_share": round(float(np.count_nonzero(flow)) / flow.size, 3), "res_scalar": int(c.m_opticalFlowResScalar)}
        for k, v in us.items():
            n = int(k.rsplit("nt", 1)[1])
            moved = (6 if k.startswith("composed") else 2) * F
            med = v[len(v) // 2] / n
            r[k] = {"us_per_t_best": round(v[0] / n, 2), "us_per_t_median": round(med, 2), "bytes_moved_per_t": moved,
                    "GBps_median": round(moved / (med * 1e-6) / 1e9, 1)}
        for tile in MAP_TILES:
            for n in T_SETS:
                a, b = r[f"composed_tile{tile}_nt{n}"], r[f"fused_tile{tile}_nt{n}"]
                b["over_composed_median"] = round(b["us_per_t_median"] / a["us_per_t_median"], 3)
                got, want = maps[("fused", tile, n)].download(np.uint8), maps[("composed", tile, n)].download(np.uint8)
                assert np.array_equal(got, want) and got.any(), (tile, n)
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
    pr = max(res["hbm_copy_probe_GBps_before"], res["hbm_copy_probe_GBps_after"])
    worst = 0.0
    for v in res.values():
        if isinstance(v, dict):
            for e in v.values():
                if isinstance(e, dict):
                    e["share_of_copy_probe"] = round(e["GBps_median"] / pr, 3)
                    worst = max(worst, e.get("over_composed_median", 0.0))
    res["acceptance_fused_not_above_composed"] = worst <= 1.0
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")
    assert worst <= 1.0, f"the fused launch took {worst} of the composition's time per t"


if __name__ == "__main__":
    main()
