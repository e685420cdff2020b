"""GPU: everything the library creates for itself comes back.  hf_debug_live_resources (include/hopperflow_diag.h) counts the device
buffers, pinned buffers, streams, events and graph executables the library holds, exactly -- where the device's free memory moves with
everybody else's work and sees no event, stream or graph at all.  Each scenario runs in ONE fresh child process
(tests/resource_lifetime_child.py), so the counts start at zero; the child prints them as JSON and the test asserts on them.  Memory
handed to the caller (hf_device_malloc, hf_host_malloc_pinned) and the timeline's process-lifetime reference event are not counted.
All shapes are 180 x 320."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ["device_buffers", "pinned_buffers", "streams", "events", "graph_execs"]
ZERO = {k: 0 for k in KINDS}


def run(scenario, native_lib):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "resource_lifetime_child.py"), scenario], capture_output=True, text=True,
                       cwd=ROOT, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["error"] is None, res["error"]     # no call reported an error, HIP's included
    return res


def test_everything_comes_back(native_lib):
    """A lone blocking planar context with a profile through every lazy allocation of a context (planar stages in and out, six period
    stages over two chunks, the side streams of asynchronous host I/O with their events and output ring, diagnostic counters on and off,
    error slots, profile spans); then three asynchronous contexts through a single-stream batch with planar sides and through a
    dual-stream batch, each with a timeline and scene state, each destroyed right behind its last enqueue -- after which a plain period
    on every former member's own stream equals a never-batched twin's."""
    res = run("everything", native_lib)
    assert res["start"] == ZERO
    for alive in ("alive_context", "alive_planar_batch", "alive_dual_batch"):
        assert all(res[alive][k] > 0 for k in KINDS), (alive, res[alive])
    c = res["counters"]   # on: exactly one device buffer more, off: exactly one less (switching them also drops the cached graphs)
    assert c["on"] == dict(c["before"], device_buffers=c["before"]["device_buffers"] + 1, graph_execs=0)
    assert c["off"] == dict(c["before"], graph_execs=0)
    assert res["profile"]["warp_launches"] > 0 and res["profile"]["flow_chains"] > 0
    assert res["after_context"] == ZERO
    assert res["planar_members_equal_twins"] and res["dual_members_equal_twins"]
    assert res["end"] == ZERO


def test_twenty_cycles_return_to_the_same_counts(native_lib):
    """tools/leak_check.py's loop twenty times: a context, and a batch of three around contexts, created, used (three updates, one
    chain, one fused three-output period) and destroyed; SDR and HDR, single- and dual-stream alternate.  The counts are exact."""
    res = run("cycles", native_lib)
    assert len(res["after_cycle"]) == 20
    for i, after in enumerate(res["after_cycle"]):
        assert after == res["start"], (i, after)


def test_destroy_behind_work_in_flight(native_lib):
    """hf_destroy's contract, its clFinish: an asynchronous context closed directly behind an enqueued chain and period, a batch closed
    directly behind hf_batch_run_period, no sync by the caller; the process then runs one period on a new context bit-exact against the
    oracle and holds nothing more than before."""
    res = run("in_flight", native_lib)
    assert res["after_destroys"] == res["start"] == ZERO
    assert res["period_bit_exact"]
    assert res["end"] == res["start"]
