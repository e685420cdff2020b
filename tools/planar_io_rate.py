"""Planar 4:2:0 frames at the device boundary (HF_FLAG_PLANAR_IN / HF_FLAG_PLANAR_OUT): what they cost.

    python tools/planar_io_rate.py [--kernels-only] [--launches 200] [--rounds 3] [--out FILE]

1. Device time per frame of the re-layout kernels alone (hf_planar_convert_device, csrc/hf_planar.hip) at 1080p SDR and 2160p HDR:
   HIP events on the context's stream around `--launches` back-to-back launches after a warm-up, with the bytes each moves (one read
   and one write of the frame) and the GB/s beside this box's streaming-copy probe (hf_hbm_copy_probe, as tools/hbm_rw_probe.py).
   `--kernels-only` stops here (for a `rocprofv3 --kernel-trace --stats -- python tools/planar_io_rate.py --kernels-only` run).
2. HostIoRunner output frames/s (one rank, pinned rings, async H2D / D2H) at 2160p HDR 24 -> 120 and 1080p SDR 24 -> 60, from an
   in-memory source, with a sink that only touches the frame, three variants alternated `--rounds` times in the same process:
     (a) NV12 / P010 contexts, the source already semi-planar;
     (b) planar contexts (HF_FLAG_PLANAR_IN | _OUT), the source planar;
     (c) NV12 / P010 contexts with the host re-layout the CLI used before (y4m.planar_to_semiplanar in fill, semiplanar_to_planar + three
         tobytes + join in sink).
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

from hopperrender_amd import capi, synth, y4m  # noqa: E402
from hopperrender_amd.batch import shard_timeline  # noqa: E402
from hopperrender_amd.calc import DeviceBuffer, OpticalFlowCalcHDR, OpticalFlowCalcSDR  # noqa: E402
from hopperrender_amd.hostio import HostIoRunner  # noqa: E402
from hopperrender_amd.protocol import SOURCE_24, TARGET_60, TARGET_120  # noqa: E402

SIZES = (("1080p_sdr", 1080, 1920, False, TARGET_60), ("2160p_hdr", 2160, 3840, True, TARGET_120))


def kernel_times(launches):
    lib = capi.load()
    gbps = C.c_double()
    capi.check(lib.hf_hbm_copy_probe(0, 512 << 20, 5, C.byref(gbps)))
    res = {"hbm_copy_probe_GBps": round(gbps.value, 1)}
    for name, H, W, hdr, _ in SIZES:
        c = (OpticalFlowCalcHDR if hdr else OpticalFlowCalcSDR)(H, W, flags=capi.HF_FLAG_ASYNC | capi.HF_FLAG_PLANAR_IN | capi.HF_FLAG_PLANAR_OUT)
        nb = c.input_frame_bytes
        a, b = DeviceBuffer(nb), DeviceBuffer(nb)
        a.upload(np.random.default_rng(1).integers(0, 256, nb, dtype=np.uint8))
        for direction, label in ((0, "ingest"), (1, "egress")):
            src, dst = (a, b) if direction == 0 else (b, a)
            for _ in range(20):
                capi.check(lib.hf_planar_convert_device(c._ctx, direction, C.c_void_p(src.ptr), C.c_void_p(dst.ptr)), c._ctx)
            c.sync()
            c.timerBegin()
            for _ in range(launches):
                capi.check(lib.hf_planar_convert_device(c._ctx, direction, C.c_void_p(src.ptr), C.c_void_p(dst.ptr)), c._ctx)
            ms = c.timerEnd()
            us = ms * 1e3 / launches
            res[f"{name}_{label}"] = {"us_per_frame": round(us, 2), "bytes": 2 * nb, "GBps": round(2 * nb / (us * 1e-6) / 1e9, 1),
                                      "share_of_copy_probe": round(2 * nb / (us * 1e-6) / 1e9 / gbps.value, 3)}
        a.free(); b.free(); c.close()
    return res


def hostio_rates(rounds, n_src):
    res = {}
    for name, H, W, hdr, target in SIZES:
        sc = synth.Scene(H, W, hdr, 3)
        nv = [sc.frame(k) for k in range(6)]
        planar = [np.concatenate([p.reshape(-1) for p in y4m.semiplanar_to_planar(f, H, W, hdr)]) for f in nv]
        planes = [(p[:H * W].reshape(H, W), p[H * W:H * W * 5 // 4].reshape(H // 2, W // 2), p[H * W * 5 // 4:].reshape(H // 2, W // 2))
                  for p in planar]
        chunk = shard_timeline(n_src, 1, 0, SOURCE_24, target)
        dt = np.dtype("<u2") if hdr else np.dtype(np.uint8)
        sink_bytes = []

        def run(variant):
            flags = capi.HF_FLAG_PLANAR_IN | capi.HF_FLAG_PLANAR_OUT if variant == "b" else 0
            r = HostIoRunner(hdr, H, W, flags=flags)
            if variant == "a":
                def fill(k, arr):
                    arr[:] = nv[k % len(nv)]

                def sink(i, arr, kind):
                    sink_bytes.append(int(arr[i % arr.size]))
            elif variant == "b":
                def fill(k, arr):
                    arr[:] = planar[k % len(planar)]

                def sink(i, arr, kind):
                    sink_bytes.append(int(arr[i % arr.size]))
            else:
                def fill(k, arr):
                    arr[:] = y4m.planar_to_semiplanar(*planes[k % len(planes)], hdr)

                def sink(i, arr, kind):
                    yy, uu, vv = y4m.semiplanar_to_planar(arr, H, W, hdr)
                    data = b"FRAME\n" + b"".join(np.ascontiguousarray(p, dtype=dt).tobytes() for p in (yy, uu, vv))
                    sink_bytes.append(len(data))
            r.run(chunk, fill, sink, 2, None, SOURCE_24, target)   # warm-up: allocations, graph captures
            t0 = time.perf_counter()
            kinds = r.run(chunk, fill, sink, 2, None, SOURCE_24, target)
            dt_s = time.perf_counter() - t0
            r.close()
            return len(kinds) / dt_s

        rates = {"a": [], "b": [], "c": []}
        for _ in range(rounds):
            for v in ("a", "b", "c"):
                rates[v].append(run(v))
        med = {v: float(np.median(x)) for v, x in rates.items()}
        res[name] = {"frames_per_s": {v: [round(x, 1) for x in xs] for v, xs in rates.items()},
                     "median": {v: round(x, 1) for v, x in med.items()},
                     "planar_over_nv12": round(med["b"] / med["a"], 3), "host_relayout_over_nv12": round(med["c"] / med["a"], 3),
                     "source_frames": n_src}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--source-frames", type=int, default=48)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"kernels": kernel_times(a.launches)}
    if not a.kernels_only:
        res["hostio"] = hostio_rates(a.rounds, a.source_frames)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
