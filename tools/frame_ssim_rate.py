"""Windowed SSIM on the device (hf_frame_ssim_enqueue, csrc/hf_metrics.hip): what one launch costs, beside the frame error sums.

    python tools/frame_ssim_rate.py [--launches 40] [--readings 7] [--out FILE]

tools/frame_error_rate.py with the SSIM launch timed beside the error launch in the same process, on the same buffers: n = 60 pairs at
3840 x 2160 HDR and n = 160 pairs at 1920 x 1080 SDR -- every frame a buffer of its own, 3 GB and 1 GB of them, so nothing is served from
the 256 MB cache -- between the library's own events (hf_timer_begin / hf_timer_end) around `--launches` back-to-back launches after a
warm-up, the median of `--readings` readings; this box's streaming-copy probe (hf_hbm_copy_probe) before and after.  Both kernels read
2 F bytes per pair (the SSIM kernel reads its tiles' halo again, mostly from L2: not counted); the probe reports read + write bytes per
second.  Prints one JSON object: per case and kernel the microseconds per launch, bytes read per second and the share of the probe, and
the ratio of SSIM time to error time.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from metrics_rate_common import finish, parse_args, rates, run, timed  # noqa: E402


def main():
    a = parse_args(__doc__)

    def case(fr, H, W, n):
        c = fr.c
        enqueues = {"frame_error": lambda: c.frameErrorEnqueue(fr.pa, fr.pb, 0), "frame_ssim": lambda: c.frameSsimEnqueue(fr.pa, fr.pb, 0)}
        r = {k: rates(us, fr.nb, n) for k, us in timed(c, enqueues, a.launches, a.readings).items()}
        r["ssim_over_error_median"] = round(r["frame_ssim"]["us_per_launch_median"] / r["frame_error"]["us_per_launch_median"], 3)
        err, ssim = c.frameErrorRead(0, 1)[0], c.frameSsimRead(0, 1)[0]
        assert err["Y"]["count"] == H * W and err["U"]["count"] == H * W // 4, err
        assert ssim["Y"]["count"] == (W // 4 - 1) * (H // 4 - 1) and ssim["U"]["count"] == (W // 8 - 1) * (H // 8 - 1) and ssim["Y"]["sum_loss_q32"] > 0, ssim
        return r

    finish(run(case), lambda r: [r["frame_error"], r["frame_ssim"]], a.out)


if __name__ == "__main__":
    main()
