"""tests/golden/make_ref_live.py -- generates tests/golden/ref_live.json, the record tests/test_ref_live_gpu.py is judged by.

Runs THE REFERENCE ITSELF (oracle/_ref/ref_runner, built by oracle/Makefile from the reference's sources in the build
container) on an MI355X through the AMD OpenCL runtime, once per case of tests/ref_live_cases.py, and stores for each case the
SHA-256 of its input frames, the reference's `stats` lines and the dtype, shape and SHA-256 of every array it wrote.

Usage (on the GPU box, from the repo root, with oracle/_ref built):
    python tests/golden/make_ref_live.py [--out tests/golden/ref_live.json]
"""
import argparse
import json
import os
import shutil
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import oracle  # noqa: E402
import ref_live_cases  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=ref_live_cases.RECORD)
    a = ap.parse_args()
    if not oracle.ref_available():
        sys.exit("needs oracle/_ref/ref_runner and an OpenCL GPU")
    records = {}
    for case in ref_live_cases.all_cases():
        t0 = time.perf_counter()
        s = oracle.RefSession(*case["session"])
        case["script"](s)
        js, arrays = s.run()
        shutil.rmtree(s.tmp, ignore_errors=True)
        records[case["key"]] = ref_live_cases.record_of(js, arrays, case["frames"])
        print(f"{case['key']}: {len(arrays)} arrays, {time.perf_counter() - t0:.1f} s", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(records, fh, indent=0, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
