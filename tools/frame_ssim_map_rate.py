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
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

from metrics_rate_common import finish, parse_args, rates, run, timed  # noqa: E402

from hopperrender_amd.calc import frame_ssim_maps  # noqa: E402

MAP_TILES = (16, 64)


def main():
    a = parse_args(__doc__)
    kernels = ["frame_error", "frame_ssim"] + [f"frame_ssim_map_tile{t}" for t in MAP_TILES]

    def case(fr, H, W, n):
        c = fr.c
        shapes = {t: c.frameSsimMapShape(t) for t in MAP_TILES}
        maps = {t: fr.buffer(n * shapes[t][2]) for t in MAP_TILES}
        enqueues = {"frame_error": lambda: c.frameErrorEnqueue(fr.pa, fr.pb, 0), "frame_ssim": lambda: c.frameSsimEnqueue(fr.pa, fr.pb, 0)}
        for t in MAP_TILES:
            enqueues[f"frame_ssim_map_tile{t}"] = lambda t=t: c.frameSsimMapEnqueue(fr.pa, fr.pb, t, maps[t].ptr)
        r = {k: rates(us, fr.nb, n) for k, us in timed(c, enqueues, a.launches, a.readings).items()}
        r["frame_ssim"]["over_error_median"] = round(r["frame_ssim"]["us_per_launch_median"] / r["frame_error"]["us_per_launch_median"], 3)
        err, ssim = c.frameErrorRead(0, 1)[0], c.frameSsimRead(0, 1)[0]
        assert err["Y"]["count"] == H * W and ssim["Y"]["count"] == (W // 4 - 1) * (H // 4 - 1), (err, ssim)
        for t in MAP_TILES:
            k = f"frame_ssim_map_tile{t}"
            r[k]["bytes_written"] = n * shapes[t][2]
            r[k]["over_ssim_median"] = round(r[k]["us_per_launch_median"] / r["frame_ssim"]["us_per_launch_median"], 3)
            m = frame_ssim_maps(maps[t].download(np.uint8, shapes[t][2]), 1, shapes[t][0], shapes[t][1])[0]
            for i, p in enumerate("YUV"):
                got = (int(m["sum_loss_q32"][i].astype(object).sum()), int(m["max_loss_q32"][i].max()), int(m["count"][i].astype(object).sum()))
                assert got == (ssim[p]["sum_loss_q32"], ssim[p]["max_loss_q32"], ssim[p]["count"]), (t, p, got, ssim[p])
        return r

    finish(run(case), lambda r: [r[k] for k in kernels], a.out)


if __name__ == "__main__":
    main()
