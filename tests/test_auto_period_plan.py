"""CPU: the order of one hf_batch_run_period_auto period (include/hopperflow.h), which a batch that defers its phase planes takes under
HF_FLAG_BATCH_AUTO_DEFERRED.  The order is ONE host-only function, plan_auto_period of csrc/hf_launch_plan.h, which hf_batch.hip follows step by
step; tests/auto_period_plan_probe.cpp exposes it (plain g++, no ROCm include path -- the compile proves the header HIP-free).  Held here over
the whole grid of its inputs: the four booleans, modes -1 .. 7, chunk counts -1 .. kMaxPeriodChunks + 1.  The same probe runs once as a
stand-alone program under -fsanitize=address,undefined.  And the flag's value as capi binds it and as the header defines it."""
import ctypes
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hopperrender_amd", "csrc")
PROBE = os.path.join(ROOT, "tests", "auto_period_plan_probe.cpp")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("auto_period_plan") / "libauto_period_plan_probe.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I", CSRC, PROBE, "-o", so])
    lib = ctypes.CDLL(so)
    k = (ctypes.c_int * 12)()
    lib.hfa_constants(k)
    lib.K = tuple(k)
    return lib


def steps(lib, defers, flag, pending, mode, all_have, chunks):
    """(early, [(kind name, chunk)]) of plan_auto_period"""
    max_steps = lib.K[0]
    names = dict(zip(lib.K[2:8], ("early_warps", "chain", "decide", "warps", "copy", "convert")))
    out = (ctypes.c_int * (2 * max_steps))()
    early = ctypes.c_int(-1)
    n = lib.hfa_plan_auto_period(int(defers), int(flag), int(pending), mode, int(all_have), chunks, out, ctypes.byref(early))
    assert 0 < n <= max_steps
    assert all(out[2 * k] == 0 and out[2 * k + 1] == 0 for k in range(n, max_steps))          # nothing behind the last step
    return bool(early.value), [(names[out[2 * k]], out[2 * k + 1]) for k in range(n)]


def grid(lib):
    max_chunks = lib.K[1]
    return itertools.product((False, True), (False, True), (False, True), range(-1, 8), (False, True), range(-1, max_chunks + 2))


def test_constants(probe):
    assert probe.K[:2] == (2 + 3 * 4, 4)                                                       # three launches per chunk, chain, decision
    assert len(set(probe.K[2:8])) == 6
    assert probe.K[8:] == (1, 2, 4, 7)


def test_the_early_order_exactly_where_it_applies_and_todays_order_everywhere_else(probe):
    max_chunks = probe.K[1]
    seen_early = 0
    for defers, flag, pending, mode, all_have, chunks in grid(probe):
        early, plan = steps(probe, defers, flag, pending, mode, all_have, chunks)
        n_chunks = min(max(chunks, 1), max_chunks)          # (a period without outputs keeps its one empty chunk: its copy launch goes out)
        want_early = defers and flag and pending and 0 <= mode <= 2 and all_have and chunks >= 1
        assert early == want_early
        later = [(kind, c) for c in range(1, n_chunks) for kind in ("warps", "copy", "convert")]
        if want_early:
            assert plan == [("early_warps", 0), ("chain", 0), ("decide", 0), ("copy", 0), ("convert", 0)] + later
            seen_early += 1
        else:
            assert plan == [("chain", 0), ("decide", 0), ("warps", 0), ("copy", 0), ("convert", 0)] + later
    assert seen_early == 3 * max_chunks + 3                 # modes 0 .. 2 x chunks 1 .. kMaxPeriodChunks + 1 (clamped), all four booleans set


def test_every_chunk_once_and_in_order_and_no_copy_ahead_of_the_decision(probe):
    max_chunks = probe.K[1]
    for args in grid(probe):
        _, plan = steps(probe, *args)
        n_chunks = min(max(args[5], 1), max_chunks)
        assert plan.count(("chain", 0)) == 1 and plan.count(("decide", 0)) == 1
        assert plan.index(("chain", 0)) < plan.index(("decide", 0))
        for c in range(n_chunks):
            warps = [k for k, s in enumerate(plan) if s in (("warps", c), ("early_warps", c))]
            copy = [k for k, s in enumerate(plan) if s == ("copy", c)]
            convert = [k for k, s in enumerate(plan) if s == ("convert", c)]
            assert len(warps) == len(copy) == len(convert) == 1, (args, plan)
            assert warps[0] < copy[0] < convert[0], (args, plan)
            assert plan.index(("decide", 0)) < copy[0], (args, plan)
            if c:                                            # the later chunks are whole and follow each other: the stages are reused
                assert (warps[0], copy[0], convert[0]) == (warps[0], warps[0] + 1, warps[0] + 2)
                assert warps[0] > [k for k, s in enumerate(plan) if s == ("convert", c - 1)][0]
        assert all(c < n_chunks for _, c in plan)
        assert [s for s in plan if s[0] == "early_warps"] in ([], [("early_warps", 0)])
        if ("early_warps", 0) in plan:
            assert plan[0] == ("early_warps", 0)


def test_the_probe_is_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "auto_period_plan_probe")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DHF_PROBE_MAIN", "-I", CSRC, PROBE, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "auto_period_plan_probe ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_the_flag_in_capi_and_in_the_header():
    from hopperrender_amd import capi
    assert capi.HF_FLAG_BATCH_AUTO_DEFERRED == 0x80000
    hdr = open(os.path.join(ROOT, "include", "hopperflow.h")).read()
    assert "#define HF_FLAG_BATCH_AUTO_DEFERRED 0x80000 " in hdr
    others = [getattr(capi, k) for k in dir(capi) if k.startswith("HF_FLAG_") and k != "HF_FLAG_BATCH_AUTO_DEFERRED"]
    assert all(v != capi.HF_FLAG_BATCH_AUTO_DEFERRED for v in others)                          # a bit of its own
