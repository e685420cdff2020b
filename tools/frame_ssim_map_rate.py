"""Per-tile SSIM maps on the device (hf_frame_ssim_map_enqueue, csrc/hf_metrics.hip): what one launch costs, beside the SSIM launch.

    python tools/frame_ssim_map_rate.py [--launches 40] [--readings 7] [--out FILE]

tools/frame_error_map_rate.py with the SSIM map launch at tile 16 and at tile 64 timed beside the error-sum launch and the SSIM launch
in the same process, on the same buffers: n = 60 pairs at 3840 x 2160 HDR and n = 160 pairs at 1920 x 1080 SDR -- every frame a buffer of
its own, 3 GB and 1 GB of them, so nothing is served from the 256 MB cache -- between the library's own events (hf_timer_begin /
hf_timer_end) around `--launches` back-to-back launches after a warm-up.  The four launches take turns within every one of the
`--readings` rounds, so a drift of the box meets them alike; the median per kernel is reported.  This box's streaming-copy probe
(hf_hbm_copy_probe) runs before and after.  All four kernels read 2 F bytes per pair from memory; the map kernel also writes 72 bytes
per tile (counted apart).  Prints one JSON object: per case and kernel the microseconds per launch, bytes read per second and the share
of the probe, and the ratio of each map launch's time to the SSIM launch's (over_ssim_median: the yardstick is the unchanged frame_ssim
launch of the same run).  Before the buffers go, the maps of the first pair are checked against its hf_frame_ssim result.
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from hopperrender_amd import capi  # noqa: E402
from hopperrender_amd.calc import DeviceBuffer, OpticalFlowCalcHDR, OpticalFlowCalcSDR, frame_ssim_maps  # noqa: E402

CASES = (("2160p_hdr_60_pairs", 2160, 3840, True, 60), ("1080p_sdr_160_pairs", 1080, 1920, False, 160))
MAP_TILES = (16, 64)


def probe():
    g = C.c_double()
    capi.check(capi.load().hf_hbm_copy_probe(0, 512 << 20, 5, C.byref(g)))
    return g.value


def timed(c, enqueues, launches, readings):
    """{kernel: sorted microseconds per launch}: `readings` rounds, in each of which every kernel has `launches` back-to-back launches"""
    for enqueue in enqueues.values():
        for _ in range(3):
            enqueue()
    c.sync()
    us = {k: [] for k in enqueues}
    for _ in range(readings):
        for k, enqueue in enqueues.items():
            c.timerBegin()
            for _ in range(launches):
                enqueue()
            us[k].append(c.timerEnd() * 1e3 / launches)
    return {k: sorted(v) for k, v in us.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", type=int, default=40); ap.add_argument("--readings", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"hbm_copy_probe_GBps_before": round(probe(), 1)}
    kernels = ["frame_error", "frame_ssim"] + [f"frame_ssim_map_tile{t}" for t in MAP_TILES]
    for name, H, W, hdr, n in CASES:
        c = (OpticalFlowCalcHDR if hdr else OpticalFlowCalcSDR)(H, W, flags=capi.HF_FLAG_ASYNC)
        nb = int(c.input_frame_bytes)
        rng = np.random.default_rng(1)
        host = [rng.integers(0, 256, nb, dtype=np.uint8) for _ in range(2)]
        fa, fb = [DeviceBuffer(nb) for _ in range(n)], [DeviceBuffer(nb) for _ in range(n)]
        for x in fa:
            x.upload(host[0])
        for x in fb:
            x.upload(host[1])
        pa, pb = [x.ptr for x in fa], [x.ptr for x in fb]
        shapes = {t: c.frameSsimMapShape(t) for t in MAP_TILES}
        maps = {t: DeviceBuffer(n * shapes[t][2]) for t in MAP_TILES}
        enqueues = {"frame_error": lambda: c.frameErrorEnqueue(pa, pb, 0), "frame_ssim": lambda: c.frameSsimEnqueue(pa, pb, 0)}
        for t in MAP_TILES:
            enqueues[f"frame_ssim_map_tile{t}"] = lambda t=t: c.frameSsimMapEnqueue(pa, pb, t, maps[t].ptr)
        rate = lambda t: 2 * nb * n / (t * 1e-6) / 1e9
        res[name] = {"pairs": n, "bytes_read": 2 * nb * n}
        for kernel, us in timed(c, enqueues, a.launches, a.readings).items():
            med = us[len(us) // 2]
            res[name][kernel] = {"us_per_launch_best": round(us[0], 1), "us_per_launch_median": round(med, 1), "us_per_pair_median": round(med / n, 3),
                                 "GBps_read_best": round(rate(us[0]), 1), "GBps_read_median": round(rate(med), 1), "pairs_per_s_median": round(n / (med * 1e-6))}
        res[name]["frame_ssim"]["over_error_median"] = round(res[name]["frame_ssim"]["us_per_launch_median"] / res[name]["frame_error"]["us_per_launch_median"], 3)
        err, ssim = c.frameErrorRead(0, 1)[0], c.frameSsimRead(0, 1)[0]
        assert err["Y"]["count"] == H * W and ssim["Y"]["count"] == (W // 4 - 1) * (H // 4 - 1), (err, ssim)
        for t in MAP_TILES:
            k = f"frame_ssim_map_tile{t}"
            res[name][k]["bytes_written"] = n * shapes[t][2]
            res[name][k]["over_ssim_median"] = round(res[name][k]["us_per_launch_median"] / res[name]["frame_ssim"]["us_per_launch_median"], 3)
            m = frame_ssim_maps(maps[t].download(np.uint8, shapes[t][2]), 1, shapes[t][0], shapes[t][1])[0]
            for i, p in enumerate("YUV"):
                got = (int(m["sum_loss_q32"][i].astype(object).sum()), int(m["max_loss_q32"][i].max()), int(m["count"][i].astype(object).sum()))
                assert got == (ssim[p]["sum_loss_q32"], ssim[p]["max_loss_q32"], ssim[p]["count"]), (t, p, got, ssim[p])
        for x in fa + fb + list(maps.values()):
            x.free()
        c.close()
    res["hbm_copy_probe_GBps_after"] = round(probe(), 1)
    pr = max(res["hbm_copy_probe_GBps_before"], res["hbm_copy_probe_GBps_after"])
    for name, *_ in CASES:
        for kernel in kernels:
            res[name][kernel]["share_of_copy_probe"] = round(res[name][kernel]["GBps_read_median"] / pr, 3)
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
