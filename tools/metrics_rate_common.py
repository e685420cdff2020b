"""What the four tools/frame_*_rate.py share: the two cases, the streaming-copy probe, the frames of a case on the device, the timing
loop and the JSON tail.  Not a tool itself.

A case is n pairs of frames, every frame a buffer of its own (3 GB and 1 GB of them, so nothing is served from the 256 MB cache).
Launches are timed between the library's own events (hf_timer_begin / hf_timer_end) around `launches` back-to-back launches after a
warm-up; the kernels of a tool take turns within every one of the `readings` rounds, so a drift of the box meets them alike.
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
from hopperrender_amd.calc import DeviceBuffer, OpticalFlowCalcHDR, OpticalFlowCalcSDR  # noqa: E402

CASES = (("2160p_hdr_60_pairs", 2160, 3840, True, 60), ("1080p_sdr_160_pairs", 1080, 1920, False, 160))


def parse_args(doc):
    ap = argparse.ArgumentParser(description=doc, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", type=int, default=40); ap.add_argument("--readings", type=int, default=7)
    ap.add_argument("--out", default=None)
    return ap.parse_args()


def probe():
    g = C.c_double()
    capi.check(capi.load().hf_hbm_copy_probe(0, 512 << 20, 5, C.byref(g)))
    return g.value


class Frames:
    """A case's context c and its n pairs of random frames on the device (pa[i], pb[i]; nb bytes a frame); free() releases both and
    every buffer made with buffer()."""

    def __init__(self, H, W, hdr, n):
        self.c = (OpticalFlowCalcHDR if hdr else OpticalFlowCalcSDR)(H, W, flags=capi.HF_FLAG_ASYNC)
        self.nb = int(self.c.input_frame_bytes)
        rng = np.random.default_rng(1)
        host = [rng.integers(0, 256, self.nb, dtype=np.uint8) for _ in range(2)]
        self.bufs = []
        fa, fb = [self.buffer(self.nb) for _ in range(n)], [self.buffer(self.nb) for _ in range(n)]
        for x in fa:
            x.upload(host[0])
        for x in fb:
            x.upload(host[1])
        self.pa, self.pb = [x.ptr for x in fa], [x.ptr for x in fb]

    def buffer(self, nbytes):
        self.bufs.append(DeviceBuffer(nbytes))
        return self.bufs[-1]

    def free(self):
        for x in self.bufs:
            x.free()
        self.c.close()


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


def rates(us, nb, n):
    """the figures of one kernel of a case from its sorted readings; every kernel reads 2 nb bytes per pair"""
    rate = lambda t: 2 * nb * n / (t * 1e-6) / 1e9
    med = us[len(us) // 2]
    return {"us_per_launch_best": round(us[0], 1), "us_per_launch_median": round(med, 1), "us_per_pair_median": round(med / n, 3),
            "GBps_read_best": round(rate(us[0]), 1), "GBps_read_median": round(rate(med), 1), "pairs_per_s_median": round(n / (med * 1e-6))}


def run(case):
    """{probe before, case name: pairs, bytes_read and what case(frames, H, W, n) returns, ..., probe after}"""
    res = {"hbm_copy_probe_GBps_before": round(probe(), 1)}
    for name, H, W, hdr, n in CASES:
        fr = Frames(H, W, hdr, n)
        try:
            res[name] = {"pairs": n, "bytes_read": 2 * fr.nb * n}
            res[name].update(case(fr, H, W, n))
        finally:
            fr.free()
    res["hbm_copy_probe_GBps_after"] = round(probe(), 1)
    return res


def finish(res, entries, out):
    """share_of_copy_probe into every entry (entries(res[case]) lists the dicts that carry GBps_read_median), print, and --out"""
    pr = max(res["hbm_copy_probe_GBps_before"], res["hbm_copy_probe_GBps_after"])
    for name, *_ in CASES:
        for e in entries(res[name]):
            e["share_of_copy_probe"] = round(e["GBps_read_median"] / pr, 3)
    s = json.dumps(res, indent=1)
    print(s)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(s + "\n")
