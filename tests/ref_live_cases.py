"""The cases of tests/test_ref_live_gpu.py: seeded inputs and the script the reference itself runs on them.

A case is the reference (oracle/_ref/ref_runner: the unmodified reference host code and OpenCL kernels) driven through the
filter's call protocol on synthetic frames.  tests/golden/make_ref_live.py runs every case on an MI355X and stores what the
reference returned -- its `stats` lines and the dtype, shape and SHA-256 of every array it wrote -- in tests/golden/ref_live.json.
The tests regenerate the inputs from the seeds (their SHA-256 is recorded too, to catch generator drift) and hold the HIP path
to that record bit for bit, so they need neither the reference's sources nor an OpenCL runtime.
"""
import hashlib
import json
import os

import numpy as np

from hopperrender_amd import synth

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_live.json")

HIP_CASES = [   # hdr, H, W, si, so, R, delta, nb, seed, max_res
    (0, 270, 480, 0, 0, 16, 8, 6, 501, 270),
    (1, 270, 480, 512, 496, 12, 8, 6, 502, 270),
    (0, 1080, 1920, 0, 0, 16, 8, 6, 503, 270),
    (1, 1080, 1920, 0, 0, 5, 6, 10, 504, 270),
    (1, 2160, 3840, 0, 0, 16, 8, 6, 505, 270),
    (0, 568, 1388, 0, 0, 12, 3, 4, 506, 1000),      # maxCalcRes above the default: 1388-wide grid, windows > 32 at neighbour-term levels
    (1, 540, 960, 0, 0, 9, 8, 6, 507, 540),         # rs = 0 at qHD
    # a kind of tests/chain_content.py in place of the seed: exact ties between a window's best candidates at every step class
    # (tests/test_chain_tie_model.py), so the record pins the reference's own choice among equal sums, the first
    (0, 256, 480, 0, 0, 16, 0, 0, "tie-d0", 270),
    (1, 540, 960, 0, 0, 16, 3, 2, "tie-d3", 270),
]
HIP_TVALS = [0.0, 0.1998, 0.3996, 0.5994, 0.999]
TINY_CASES = [(0, 4, 4), (1, 4, 4), (0, 6, 10)]     # hdr, H, W
LEVELS = [(16.0, 16.0), (0.0, 0.0), (200.0, 100.0), (-20.0, 300.0), (0.0, 1e-3), (255.0, 0.0)]   # (black, white)
RANDOM_SEEDS = list(range(52))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def hip_case(hdr, H, W, si, so, R, delta, nb, seed, max_res):
    if isinstance(seed, str):
        import chain_content
        rs = next(r for r in range(16) if (H >> r) <= max_res)
        f = chain_content.frames(seed, H, W, bool(hdr), chain_content.kind_seed(seed), 4, si, rs)
    else:
        sc = synth.Scene(H, W, bool(hdr), seed, in_stride=si)
        f = [sc.frame(k) for k in range(4)]

    def script(s):
        s.radius(R)
        for x in f[:3]:
            s.update(x)
        s.calc(); s.stats(); s.dump_offsets("off"); s.dump_blurred(1, "blur")
        s.update(f[3]); s.calc(); s.stats()
        if isinstance(seed, str):
            s.dump_offsets("off2")
        for m in (0, 1, 2):
            for t in HIP_TVALS:
                s.warp(t, m); s.download(f"w{m}_{t}")
        s.copy(); s.download("copy")
    return dict(key=f"hip/hdr{hdr}_{H}x{W}_si{si}_so{so}_R{R}_d{delta}_n{nb}_seed{seed}_res{max_res}", frames=f,
                session=(hdr, H, W, si, so, delta, nb, 0.0, 255.0, max_res), script=script)


def tiny_case(hdr, H, W):
    f = [synth.random_frame(H, W, bool(hdr), seed=900 + 7 * i + H + W) for i in range(4)]

    def script(s):
        s.radius(5)
        for x in f[:3]:
            s.update(x)
        s.calc(); s.update(f[3]); s.calc()
        s.dump_blurred(0, "flow")
        for m in (0, 1, 2):
            s.warp(0.43, m); s.download(f"w{m}")
        s.copy(); s.download("copy")
    return dict(key=f"tiny/hdr{hdr}_{H}x{W}", frames=f, session=(hdr, H, W, 0, 0, 8, 6, 0.0, 255.0, 270), script=script)


def levels_case(hdr, bk, wh):
    H, W = 36, 64
    sc = synth.Scene(H, W, bool(hdr), 5)
    f = [sc.frame(k) for k in range(4)]

    def script(s):
        s.radius(8)
        for x in f[:3]:
            s.update(x)
        s.calc(); s.update(f[3]); s.calc()
        s.warp(0.4, 2); s.download("w2")
        s.copy(); s.download("copy")
    return dict(key=f"levels/hdr{hdr}_black{bk!r}_white{wh!r}", frames=f, H=H, W=W,
                session=(hdr, H, W, 0, 0, 8, 6, bk, wh, 270), script=script)


def random_case(seed):
    """The randomized sweep of test_random_gpu.py: geometry, pitches, resolution scalar, search radius 2..16, scalars, levels."""
    rng = np.random.default_rng(9000 + seed)
    hdr = int(rng.integers(0, 2))
    H = int(rng.integers(8, 120)) * 2
    W = int(rng.integers(16, 200)) * 2
    if seed >= 40:                          # frames up to ~1100 x 2000: resolution scalars 2-3, 16-byte warp threads, many tiles
        H = int(rng.integers(280, 560)) * 2
        W = int(rng.integers(500, 1000)) * 2
        if seed % 2:
            W = (W + 15) // 16 * 16
    si = W + int(rng.choice([0, 0, 2, 16, 6]))
    so = W + int(rng.choice([0, 0, 2, 16, 10]))
    max_res = int(rng.choice([270, 270, 64, 40, 1000]))
    R = int(rng.integers(2, 17))
    delta, nb = int(rng.integers(0, 11)), int(rng.integers(0, 11))
    bk, wh = float(rng.choice([0.0, 16.0, 3.5])), float(rng.choice([255.0, 235.0, 200.25]))
    sc = synth.Scene(H, W, bool(hdr), seed=700 + seed, in_stride=si, max_rect_speed=int(rng.integers(2, 30)))
    f = [sc.frame(k) for k in range(4)]
    ts = [0.0, float(np.float32(rng.random())), 0.999]

    def script(s):
        s.radius(R)
        for x in f[:3]:
            s.update(x)
        s.calc(); s.stats(); s.dump_offsets("off"); s.dump_blurred(1, "blur")
        s.update(f[3]); s.radius(R); s.calc(); s.stats()
        for m in (0, 1, 2):
            for t in ts:
                s.warp(t, m); s.download(f"w{m}_{t}")
        s.copy(); s.download("copy")
    cfg = dict(hdr=hdr, H=H, W=W, si=si, so=so, max_res=max_res, R=R, delta=delta, nb=nb, bk=bk, wh=wh)
    return dict(key=f"random/seed{seed}", frames=f, cfg=cfg, ts=ts, session=(hdr, H, W, si, so, delta, nb, bk, wh, max_res), script=script)


def all_cases():
    yield from (hip_case(*p) for p in HIP_CASES)
    yield from (tiny_case(*p) for p in TINY_CASES)
    yield from (levels_case(hdr, bk, wh) for hdr in (0, 1) for bk, wh in LEVELS)
    yield from (random_case(seed) for seed in RANDOM_SEEDS)


def record_of(js, arrays, frames):
    """What the record keeps of one reference run (its `stats` lines without the timings, which differ from run to run)."""
    return {"inputs_sha": [sha(x) for x in frames], "stats": [{k: v for k, v in line.items() if not k.endswith("_time")} for line in js],
            "outputs": {k: {"dtype": str(a.dtype), "shape": list(a.shape), "sha256": sha(a)} for k, a in arrays.items()}}


_records = None


class Recorded:
    """The reference's results for one case, read from tests/golden/ref_live.json."""

    def __init__(self, case):
        global _records
        if _records is None:
            with open(RECORD) as fh:
                _records = json.load(fh)
        assert case["key"] in _records, f"{case['key']} is not in {RECORD} (regenerate it with tests/golden/make_ref_live.py)"
        rec = _records[case["key"]]
        assert [sha(x) for x in case["frames"]] == rec["inputs_sha"], "synthetic generator drifted from the recorded inputs"
        self.stats = rec["stats"]
        self.outputs = rec["outputs"]

    def same(self, name, a):
        """True when `a` is bit for bit the array the reference wrote under `name` (dtype, shape and SHA-256)."""
        e = self.outputs[name]
        return a.dtype == np.dtype(e["dtype"]) and list(a.shape) == e["shape"] and sha(a) == e["sha256"]
