"""GPU: every phase-plane builder against the numpy model of the documented layout (tests/phase_plane_model.py) at resolution scalars 0 to 3,
and the planes a batch leaves to its warp launch at 3 and 4.  The chain never reads a frame, it reads the plane -- and its margins, mx columns
on either side with the reference's edge reflection baked in (calcDeltaSumsKernelSDR.h:86-95), are far wider than any content of the chain
tests reaches.  Here every element in use, columns [-mx, lw + mx) of every phase pair and row, is compared; the data is exact.

tests/plane_builder_model.py is the matrix and says which builder the library takes for each case (prep_phase_fast_kernel<E, RS, NT> or
prep_phase_kernel<E>, and why); tests/test_plane_builders_model.py proves on the CPU that this restates the compiled decision, that the
matrix reaches all 16 fast instantiations of rs 0 .. 3, the generic kernel for every reason on its own, both margin regimes, mx == lw and
both plane_fast_task<E, RS, 1> instantiations of the warp launch, and that a builder with a wrong swap, mirrored row, chroma pair,
reflection, rounding or second luma byte shows on every case.  A mismatch names (row, phase pair, column j) and the predicted builder.

  * per case, a lone context: three updateFrame calls; a case whose frames sit 8 bytes into their allocation is shown them through
    updateFrameDevice (copied into the context's own slot first: the alignment does not reach the builder) and through updateFrameDeviceRef
    (it does: the generic kernel);
  * per case, a batch of three with distinct content, FlowBatch.updateFramesDeviceRef: one launch builds all three planes;
  * the deferred cases: the grid samples of prep_grid_kernel while the plane is incomplete, the plane once the next period's warp launch
    has built it (one member's by the generic kernel: its frames are misaligned), and the flow of the chain that read it against the oracle;
  * the small cases once more in a child process on the bounds-checking library: no violation."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import phase_plane_model as P  # noqa: E402
import plane_builder_model as B  # noqa: E402
from test_chain_deep_rs_gpu import assert_planes  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_context(case, flags=0):
    from hopperrender_amd.calc import OpticalFlowCalcHDR, OpticalFlowCalcSDR
    c = (OpticalFlowCalcHDR if case.hdr else OpticalFlowCalcSDR)(case.H, case.W, case.in_stride, 0, 8, 6, 0.0, 255.0, case.max_res, search_radius=16,
                                                                flags=flags)
    rs, lw, lh, _ = B.geometry(case)
    assert (c.m_opticalFlowResScalar, c.m_opticalFlowFrameWidth, c.m_opticalFlowFrameHeight) == (rs, lw, lh), case.name
    return c


def put(frame, off):
    """The frame in a device buffer of its own, `off` bytes behind the (at least 16-byte aligned) start of the allocation."""
    from hopperrender_amd import capi
    from hopperrender_amd.calc import DeviceBuffer
    b = DeviceBuffer(frame.nbytes + 64)
    assert b.ptr % 16 == 0
    capi.check(capi.load().hf_memcpy_h2d(0, C.c_void_p(b.ptr + off), frame.ctypes.data_as(C.c_void_p), frame.nbytes))
    return b


def said(b):
    return "the model says %s%s" % (b.name, " (%s)" % ", ".join(b.reasons) if b.reasons else "")


def run_lone(case):
    fr = B.frames(case, 0)
    off = case.offs[0]
    for entry in (["device", "device-ref"] if off else ["host"]):
        b = B.builder(case, False, copied=entry != "device-ref")
        c, dev = make_context(case), []
        try:
            for f in fr:
                if entry == "host":
                    c.updateFrame(f)
                else:
                    dev.append(put(f, off))
                    (c.updateFrameDevice if entry == "device" else c.updateFrameDeviceRef)(dev[-1].ptr + off)
            assert_planes(case, c, fr, "lone, %s frames; %s" % (entry, said(b)))
        finally:
            c.close()
            for d in dev:
                d.free()


def run_batch(case):
    from hopperrender_amd import capi
    from hopperrender_amd.calc import FlowBatch
    fr = [B.frames(case, m) for m in range(3)]
    b = B.builder(case, True)
    cs = [make_context(case, capi.HF_FLAG_ASYNC) for _ in range(3)]
    dev, batch = [], None
    try:
        dev = [[put(f, case.offs[m]) for f in fr[m]] for m in range(3)]
        batch = FlowBatch(cs)
        assert not batch.defersPlanes()
        for s in range(3):
            batch.updateFramesDeviceRef([dev[m][s].ptr + case.offs[m] for m in range(3)])
        batch.sync()
        for m in range(3):
            assert_planes(case, cs[m], fr[m], "batch member %d; %s" % (m, said(b)))
    finally:
        if batch is not None:
            batch.close()
        for c in cs:
            c.close()
        for d in [x for row in dev for x in row]:
            d.free()


@pytest.mark.parametrize("case", B.CASES, ids=lambda c: c.name)
def test_lone_context_planes_equal_the_layout_model(native_lib, case):
    run_lone(case)


@pytest.mark.parametrize("case", B.CASES, ids=lambda c: c.name)
def test_batch_planes_equal_the_layout_model(native_lib, case):
    run_batch(case)


# ------------------------------------------------------------------------------------------------
# deferred planes: prep_grid_kernel, then plane_fast_task<E, RS, 1> inside the next period's warp launch
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", B.DEFERRED_CASES, ids=lambda c: c.name)
def test_deferred_planes_equal_the_layout_model(native_lib, case):
    """Three noise frames shown in turn, member m starting at frame m.  Period k (k >= 2) warps frames k - 2 and k - 1 ahead of its chain, and
    that launch builds the plane of frame k - 1; the member at base + 8 bytes gets its plane from the generic kernel."""
    from hopperrender_amd import capi
    from hopperrender_amd.calc import DeviceBuffer, FlowBatch
    from oracle import oracle
    rs, lw, lh, L = B.geometry(case)
    n, H = case.n, case.H
    g = oracle.make_geom(case.hdr, H, case.W, case.in_stride, 0, case.max_res)
    fr = B.frames(case, 0)
    want = [P.plane(f, bool(case.hdr), H, case.W, case.in_stride, L, lw) for f in fr]
    shown = lambda m, k: (m + k) % 3
    grid_rows = np.arange(lh) << rs
    cs = [make_context(case, capi.HF_FLAG_ASYNC | capi.HF_FLAG_NO_TIMING) for _ in range(n)]
    dev, dev_odd, outs, batch = [], [], [], None

    def read(m, slot, complete, what):
        words, done = cs[m].readPhasePlane(slot)
        assert done == complete, (case.name, what, "member", m, "slot", slot)
        return P.used(words, H, L, lw)

    def assert_grid_samples(k):
        """what prep_grid_kernel wrote of the newest frame: phase pair 0, rows cy << rs, columns [0, lw)"""
        for m in range(n):
            got = read(m, 2, False, "period %d, newest" % k)[grid_rows, 0, L.mx:L.mx + lw]
            bad = got != want[shown(m, k)][grid_rows, 0, L.mx:L.mx + lw]
            assert not bad.any(), (case.name, "grid samples, period", k, "member", m, int(bad.sum()), "first (grid row, column):", np.argwhere(bad)[:4].tolist())

    def assert_older_plane(k, who):
        """slot 1 after period k: the plane of frame k - 1, complete"""
        for m in range(n):
            bad = read(m, 1, True, "period %d, older" % k) != want[shown(m, k - 1)]
            assert not bad.any(), (case.name, "period", k, "member", m, "generic.%s (misaligned base)" % ("u16" if case.hdr else "u8") if m == case.odd else who,
                                   int(bad.sum()), "first (row, phase pair, column j):", [(int(y), int(p2), int(j) - L.mx) for y, p2, j in np.argwhere(bad)[:4]])

    try:
        dev, dev_odd = [put(f, 0) for f in fr], [put(f, 8) for f in fr]
        src = lambda k: [dev_odd[shown(m, k)].ptr + 8 if m == case.odd else dev[shown(m, k)].ptr for m in range(n)]
        outs = [[DeviceBuffer(c.output_frame_bytes) for _ in range(2)] for c in cs]
        plans, optr = [[0.25, 0.75]] * n, [[b.ptr for b in o] for o in outs]
        batch = FlowBatch(cs)
        assert batch.defersPlanes() and cs[0].phase_plane_bytes == L.bytes
        batch.runPeriod(batch.preparePeriod(src(0), None, None, calculate_flow=False))
        batch.sync()
        assert_grid_samples(0)
        batch.runPeriod(batch.preparePeriod(src(1), None, None))                 # no outputs, no warp launch: frame 0's planes from ONE plane launch,
        batch.sync()                                                             # which the misaligned member sends to the generic kernel
        assert_older_plane(1, "generic.%s (misaligned base of member %d)" % ("u16" if case.hdr else "u8", case.odd))
        warp = "plane_fast_task<%s, %d, 1> in the warp launch" % ("uint16_t" if case.hdr else "uint8_t", rs)
        for k in (2, 3):
            batch.runPeriod(batch.preparePeriod(src(k), plans, optr, 2))
            batch.sync()
            if k == 2:
                assert_grid_samples(k)
            assert_older_plane(k, warp)
            if k == 2:                                                           # the chain of (1, 2) read the plane the warp launch built
                flows = {}
                for m in range(n):
                    pair = (shown(m, 1), shown(m, 2))
                    if pair not in flows:
                        _, flows[pair], _, oob = oracle.calculate_optical_flow(fr[pair[0]], fr[pair[1]], g, 16)
                        assert oob == 0, (case.name, pair)
                    assert np.array_equal(cs[m].readBlurredFlow(1), flows[pair]), (case.name, "flow of the chain behind the warp-built plane, member", m)
    finally:
        if batch is not None:
            batch.close()
        for c in cs:
            c.close()
        for b in dev + dev_odd + [x for o in outs for x in o]:
            b.free()


# ------------------------------------------------------------------------------------------------
# the small cases on the bounds-checking library
# ------------------------------------------------------------------------------------------------
CHILD = r"""
import sys, ctypes as C
sys.path.insert(0, {root!r}); sys.path.insert(0, {root!r} + "/tests")
from hopperrender_amd import capi
from hopperrender_amd.calc import OpticalFlowCalcSDR
import plane_builder_model as B
import test_plane_builders_gpu as T
assert capi.is_debug_bounds_build()
for case in B.CASES:
    T.run_lone(case)
    T.run_batch(case)
probe = OpticalFlowCalcSDR(64, 96)
n = C.c_uint32(0); first = (C.c_uint32 * 4)()
capi.check(probe._lib.hf_debug_bounds_violations(probe._ctx, C.byref(n), first, 0), probe._ctx)
assert n.value == 0, (n.value, list(first))
probe.close()
print("PLANE-BOUNDS-OK")
"""


def test_small_cases_under_the_bounds_checking_build(native_lib):
    """Every load and store of the plane builders checked against the frame and the plane (csrc/hf_kernels.h HF_DBG_CHECK): zero violations,
    and the same planes."""
    from hopperrender_amd import build
    dbg = build.build_flow(debug_bounds=True)
    env = dict(os.environ, HF_LIB=dbg)
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT)], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0 and "PLANE-BOUNDS-OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
