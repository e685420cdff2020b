"""Frame error sums on the device (hf_frame_error_enqueue, csrc/hf_metrics.hip): what one launch costs.

    python tools/frame_error_rate.py [--launches 40] [--readings 7] [--out FILE]

Device time of one launch over n = 60 pairs at 3840 x 2160 HDR and n = 160 pairs at 1920 x 1080 SDR -- every frame a buffer of its own, 3 GB
and 1 GB of them, so nothing is served from the 256 MB cache -- between the library's own events (hf_timer_begin / hf_timer_end) around
`--launches` back-to-back launches after a warm-up, `--readings` times; beside this box's streaming-copy probe (hf_hbm_copy_probe) in the
same process, before and after.  The probe reports read + write bytes per second; the kernel only reads, 2 F bytes per pair.
Prints one JSON object.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from metrics_rate_common import finish, parse_args, rates, run, timed  # noqa: E402


def main():
    a = parse_args(__doc__)

    def case(fr, H, W, n):
        c = fr.c
        us = timed(c, {"frame_error": lambda: c.frameErrorEnqueue(fr.pa, fr.pb, 0)}, a.launches, a.readings)
        got = c.frameErrorRead(0, 1)[0]
        assert got["Y"]["count"] == H * W and got["U"]["count"] == H * W // 4, got
        return rates(us["frame_error"], fr.nb, n)

    finish(run(case), lambda r: [r], a.out)


if __name__ == "__main__":
    main()
