"""CPU: periods of more than six outputs through a batch (hf_batch_*_wide, include/hopperflow.h).  The split of a period into chunks of at
most kMaxWarpOutputs outputs per member is ONE host-only function, plan_period_chunks of csrc/hf_launch_plan.h; tests/period_chunks_probe.cpp
exposes it (plain g++, no ROCm include path -- the compile proves the header HIP-free, as tests/launch_plan_probe.py does for the launch
plans).  Held here over every n_out vector of VALUES for 1 and 2 members, and for 32 members over the vectors (a, b, VALUES cyclically from
s) for every a, b, s plus 2,000 random ones (all 8^32 cannot be walked; the function treats members independently, so a member's row
depends on its own n_out only, which the one- and two-member grids hold exhaustively -- the 32-member vectors hold the indexing and the
chunk count over a full batch).  The same probe runs once as a stand-alone program under -fsanitize=address,undefined.  And the symbols and
constants of the new calls as capi binds them."""
import ctypes
import itertools
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hopperrender_amd", "csrc")
PROBE = os.path.join(ROOT, "tests", "period_chunks_probe.cpp")
VALUES = (0, 1, 5, 6, 7, 12, 13, 24)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("period_chunks") / "libperiod_chunks_probe.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I", CSRC, PROBE, "-o", so])
    lib = ctypes.CDLL(so)
    k = (ctypes.c_int * 4)()
    lib.hfc_constants(k)
    lib.K = tuple(k)
    return lib


def split(lib, n_out):
    """(n_chunks, [chunk][member] counts) of plan_period_chunks"""
    _, _, max_chunks, max_batch = lib.K
    out = (ctypes.c_int * (1 + max_chunks * max_batch))()
    n = lib.hfc_plan_period_chunks(len(n_out), (ctypes.c_int * len(n_out))(*n_out), out)
    assert n == out[0]
    rows = [[out[1 + c * max_batch + m] for m in range(max_batch)] for c in range(max_chunks)]
    assert all(v == 0 for r in rows for v in r[len(n_out):])                      # nothing for members the batch does not have
    return n, [r[:len(n_out)] for r in rows]


def check(lib, n_out):
    per_chunk = lib.K[0]
    n_chunks, rows = split(lib, n_out)
    assert n_chunks == max(-(-v // per_chunk) for v in n_out), n_out              # ceil(max n_out / 6)
    assert all(v == 0 for r in rows[n_chunks:] for v in r), n_out
    for m, total in enumerate(n_out):
        col = [r[m] for r in rows]
        assert all(0 <= v <= per_chunk for v in col), (n_out, m)                  # no chunk holds more than 6 outputs of a member
        # every output in exactly one chunk, in order: chunk c holds [6 c, min(6 c + 6, total))
        assert col == [max(0, min(per_chunk, total - c * per_chunk)) for c in range(len(col))], (n_out, m, col)
        assert sum(col) == total
        assert (col[0] > 0) == (total > 0), (n_out, m)                            # chunk 0 holds every member with an output


def test_constants_of_the_split(probe):
    from hopperrender_amd import capi
    assert probe.K == (capi.HF_MAX_PERIOD_OUTPUTS, capi.HF_MAX_PERIOD_OUTPUTS_WIDE, 4, 32)
    assert max(VALUES) == capi.HF_MAX_PERIOD_OUTPUTS_WIDE


@pytest.mark.parametrize("members", [1, 2])
def test_every_vector_of_one_and_two_members(probe, members):
    for n_out in itertools.product(VALUES, repeat=members):
        check(probe, list(n_out))


def test_batches_of_32(probe):
    for a, b, s in itertools.product(VALUES, VALUES, range(len(VALUES))):
        check(probe, [a, b] + [VALUES[(s + m) % len(VALUES)] for m in range(2, 32)])
    rng = random.Random(7)
    for _ in range(2000):
        check(probe, [rng.choice(VALUES) for _ in range(32)])
    check(probe, [0] * 32)
    check(probe, [24] * 32)


def test_out_of_range_counts_are_clamped_not_indexed(probe):
    """The callers refuse such an n_out (check_period_args); the plan is computed before that in one place and must stay inside its table."""
    assert split(probe, [-3, 7])[1][0] == [0, 6] and split(probe, [-3, 7])[0] == 2
    assert split(probe, [1000])[0] == 4 and [r[0] for r in split(probe, [1000])[1]] == [6, 6, 6, 6]


def test_the_probe_is_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "period_chunks_probe")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DHF_PROBE_MAIN", "-I", CSRC, PROBE, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "period_chunks_probe ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_symbols_and_constants(native_lib):
    from hopperrender_amd import capi
    for name in ("hf_batch_interpolate_period_wide", "hf_batch_run_period_wide", "hf_batch_run_period_auto_wide"):
        assert name in capi.SIGNATURES and getattr(native_lib, name).argtypes == capi.SIGNATURES[name][1]
    assert capi.HF_MAX_PERIOD_OUTPUTS == 6 and capi.HF_MAX_PERIOD_OUTPUTS_WIDE == 24
    assert native_lib.hf_abi_version() == 6
    hdr = open(os.path.join(ROOT, "include", "hopperflow.h")).read()
    assert "#define HF_MAX_PERIOD_OUTPUTS 6\n" in hdr and "#define HF_MAX_PERIOD_OUTPUTS_WIDE 24 " in hdr


def test_the_wide_calls_refuse_a_null_batch(native_lib):
    """No GPU needed: the argument checks that come before the device is touched."""
    from hopperrender_amd import capi
    assert native_lib.hf_batch_interpolate_period_wide(None, 7, None, None, None, 2) == capi.HF_ERR_INVALID_ARGUMENT
    assert native_lib.hf_batch_run_period_wide(None, None, 0, 7, None, None, None, 2) == capi.HF_ERR_INVALID_ARGUMENT
    assert native_lib.hf_batch_run_period_auto_wide(None, None, 7, None, None, None, 2, None) == capi.HF_ERR_INVALID_ARGUMENT


def test_the_schedules_the_wide_calls_exist_for():
    """Outputs per source period of a 23.976 fps clip at the display rates above 120 Hz: all within HF_MAX_PERIOD_OUTPUTS_WIDE, all but
    120 Hz beyond HF_MAX_PERIOD_OUTPUTS in some period."""
    from hopperrender_amd import capi
    from hopperrender_amd.protocol import SOURCE_24, BlendSchedule
    counts = {target: [len(ts) for ts in BlendSchedule(SOURCE_24, target).plan(14)] for target in (83333, 69444, 60606, 41667, 20833)}
    assert counts[83333][:3] == [6, 5, 5] and max(counts[83333]) == capi.HF_MAX_PERIOD_OUTPUTS
    assert counts[69444][:4] == [7, 6, 6, 6]
    assert counts[60606][:10] == [7, 7, 7, 7, 7, 7, 7, 7, 6, 7]
    assert counts[41667][:3] == [11, 10, 10]
    assert counts[20833][:3] == [21, 20, 20] and max(counts[20833]) <= capi.HF_MAX_PERIOD_OUTPUTS_WIDE
