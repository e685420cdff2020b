"""CPU: hf_debug_live_resources (include/hopperflow_diag.h) -- the library's own count of the device buffers, pinned buffers, streams,
events and graph executables it holds for itself.  It takes no context and needs no device, so it answers here.  The counts are per
process: they are read in a fresh child, which no object of another test of the session disturbs.  What the counts do while contexts
and batches live is tests/test_resource_lifetime_gpu.py's."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ["device_buffers", "pinned_buffers", "streams", "events", "graph_execs"]
HF_ERR_INVALID_ARGUMENT, HF_ERR_NO_DEVICE = -1, -2

CHILD = r"""
import ctypes as C, json, sys
sys.path.insert(0, {root!r})
from hopperrender_amd import capi
L = capi.load()
res = {{"fresh": capi.live_resources()}}
# a create that fails: the device one past the last (with no device present: any device)
cfg = capi.HfConfig(struct_size=C.sizeof(capi.HfConfig), is_hdr=0, frame_height=180, frame_width=320, delta_scalar=8, neighbor_scalar=6,
                    black_level=0.0, white_level=255.0, max_calc_res=270, device_index=L.hf_device_count())
ctx = C.c_void_p()
res["create_rc"] = L.hf_create(C.byref(cfg), C.byref(ctx))
res["ctx_is_null"] = not ctx.value
res["after_failed_create"] = capi.live_resources()
res["null_rc"] = L.hf_debug_live_resources(None)
print(json.dumps(res))
"""


@pytest.fixture(scope="module")
def res(native_lib):
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT)], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_live_resources_of_a_process_that_created_nothing(res):
    assert res["fresh"] == {k: 0 for k in KINDS}


def test_a_failed_create_leaves_nothing_behind(res):
    assert res["create_rc"] == HF_ERR_NO_DEVICE and res["ctx_is_null"]
    assert res["after_failed_create"] == {k: 0 for k in KINDS}


def test_null_argument_is_refused(native_lib, res):
    assert native_lib.hf_debug_live_resources(None) == HF_ERR_INVALID_ARGUMENT
    assert res["null_rc"] == HF_ERR_INVALID_ARGUMENT
