"""GPU: the flow chain and the phase-plane builders at resolution scalars 4, 5 and 6 against the CPU oracle.  The scalar is bounded by nothing
but the frame height and the calculation-resolution setting (2160p at a setting of 64 runs at rs 6, 8K at the default at rs 4), and the code
that depends on it changes behaviour exactly there: the chain's staged Y-row and 8-window forms are compiled for rs 0 .. 4 and refuse beyond
(every tile of rs 5 and 6 takes the fallback bodies, which below only see edge tiles and R != 16), the fast plane kernel stops at rs 4 (the
generic kernel then builds 16 or 32 phase-pair rows per luma row), strips and margins scale with 2^rs on grids of a few tiles, and on a
frame whose width is no multiple of 2^rs the last grid column's higher phases lie beyond the frame.  chain_variant_model.DEEP_CASES is the
matrix; tests/test_chain_deep_rs_model.py proves on the CPU that its content lands winners on every phase pair and beyond every frame edge
with the reference defined (oob == 0), and that it reaches the variants and tile classes.

  * the chain: machinery and bar of tests/test_chain_variants_gpu.py -- two consecutive pairs and the graph's replay, every member against the
    oracle of its own pair, offsets, blurred flow and total frame delta bit-exact (integer arithmetic), the table counters against the model
    where tables run at R 16.  A batch size of 1 is a lone context, one kind after the other; one batch runs without the lazy argmin, one
    lone context without its graph, and per scalar one plain blocking context.
  * the batched update path: FlowBatch.runPeriod on device frames (one plane launch for the frames of all members), three members, two
    periods with outputs: both flows against the oracle, the outputs of mode 2 bit-exact against oracle.warp_frames.
  * the planes themselves: hf_read_phase_plane of all three ring slots against the numpy model of the documented layout
    (tests/phase_plane_model.py), on the columns in use, for a lone context and for the members of a batch whose frames one launch takes.
    rs 4 on the aligned shapes holds prep_phase_fast_kernel<E, 4, .> (both store policies), everything else prep_phase_kernel: a mismatch
    names the builder instead of surfacing as a flipped winner."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_variant_model as M  # noqa: E402
import phase_plane_model as P  # noqa: E402
from test_chain_variants_gpu import assert_members, assert_table_counters, case_frames, oracle_results, read, run_case  # noqa: E402

pytestmark = pytest.mark.gpu

BY_RS = {rs: [c for c in M.DEEP_CASES if M.geometry(c).rs == rs] for rs in (4, 5, 6)}


def more_flags(case):
    from hopperrender_amd import capi
    return {M.DEEP_NO_LAZY: capi.HF_FLAG_NO_LAZY_ARGMIN, M.DEEP_NO_GRAPH: capi.HF_FLAG_NO_GRAPH}.get(case.name, 0)


def make_context(case, flags, **kw):
    from hopperrender_amd import capi
    from hopperrender_amd.calc import OpticalFlowCalcHDR, OpticalFlowCalcSDR
    cls = OpticalFlowCalcHDR if case.hdr else OpticalFlowCalcSDR
    flags |= {M.ALWAYS: capi.HF_FLAG_SAD_REUSE_ALWAYS, M.NEVER: capi.HF_FLAG_NO_SAD_REUSE, M.DEFAULT: 0}[case.tables]
    c = cls(case.H, case.W, case.in_stride, 0, case.delta, case.nb, 0.0, 255.0, case.max_res, iterations=case.iterations,
            blur_radius=case.blur_radius, search_radius=case.R, flags=flags, **kw)
    g = M.geometry(case)
    assert (c.m_opticalFlowResScalar, c.m_opticalFlowFrameWidth, c.m_opticalFlowFrameHeight) == (g.rs, g.lw, g.lh), case.name
    return c


def run_lone(case, kinds, flags):
    """One context per kind, no batch: both pairs against the oracle, the second once more (the context's own cached graph, if it keeps one)."""
    counted = bool(M.tables_on(case)) and case.R == 16
    for kind in kinds:
        f = case_frames(case, kind)
        c = make_context(case, flags)
        try:
            for x in f[:3]:
                c.updateFrame(x)
            for pair in (1, 2):
                if pair == 2:
                    c.updateFrame(f[3])
                    if counted:
                        c.countersEnable(True)
                c.calculateOpticalFlow()
                want = oracle_results(case, {(kind, pair): (f[pair], f[pair + 1])})
                c.sync()
                got, = assert_members(case, [c], [(kind, pair)], want, f"lone {kind} pair {pair}")
                assert c.stats()["sad_tables"] == int(M.tables_on(case)), (case.name, kind)
            if counted:
                assert_table_counters(case, c.counters(reset=True))
                c.countersEnable(False)
            c.calculateOpticalFlow()
            c.sync()
            again = read(c)
            assert (again[0] == got[0]).all() and (again[1] == got[1]).all() and again[2] == got[2], (case.name, kind, "replay")
        finally:
            c.close()


@pytest.mark.parametrize("case", M.DEEP_CASES, ids=lambda c: c.name)
def test_deep_chain_matches_oracle(native_lib, case):
    from hopperrender_amd import capi
    if case.n == 1:
        run_lone(case, M.deep_member_kinds(case), capi.HF_FLAG_ASYNC | more_flags(case))
    else:
        run_case(case, kinds=M.deep_member_kinds(case), more_flags=more_flags(case))


@pytest.mark.parametrize("rs", [4, 5, 6])
def test_plain_blocking_context_matches_oracle(native_lib, rs):
    """No flag but the table mode's: calculateOpticalFlow returns with the results there."""
    case = next(c for c in BY_RS[rs] if c.n == 1 and M.tables_on(c))
    run_lone(case, ["drift-ne", "chaotic"], 0)


# ------------------------------------------------------------------------------------------------
# the batched update path: FlowBatch.runPeriod on device frames
# ------------------------------------------------------------------------------------------------
PERIOD_CASES = {5: "r5-hdr1608-n3-notab", 6: "r6-sdr1608-n3-notab"}      # the ragged shapes: the generic plane kernel with phases beyond the frame
PERIOD_KINDS = ["drift-se", "noise", "chaotic"]
PERIOD_TS = [(0.25, 0.75), (0.5, 1.0), (0.0, 0.625)]


@pytest.mark.parametrize("rs", sorted(PERIOD_CASES))
def test_batched_periods_on_device_frames(native_lib, rs):
    """Period k warps frames k - 2 and k - 1 with the flow of that pair and computes the flow of (k - 1, k); the frames of the three members
    arrive as device pointers and their planes are built by ONE launch (launch_prep_frames over n frames) -- no batch at rs >= 5 defers."""
    from hopperrender_amd import capi
    from hopperrender_amd.calc import FlowBatch
    from oracle import oracle
    from test_warp_variants_gpu import Buf
    case = M.case(PERIOD_CASES[rs])
    g = M.geometry(case)
    assert g.rs == rs and case.n == len(PERIOD_KINDS) and case.R == 16
    oracle.set_flavour(1, 1, None)
    dt = np.uint16 if case.hdr else np.uint8
    fr = {k: case_frames(case, k) for k in PERIOD_KINDS}
    flows = {(k, p): oracle.calculate_optical_flow(fr[k][p - 1], fr[k][p], g, case.R, case.iterations, case.delta, case.nb, case.blur_radius)[1]
             for k in PERIOD_KINDS for p in (1, 2, 3)}
    cs = [make_context(case, capi.HF_FLAG_ASYNC | capi.HF_FLAG_NO_TIMING) for _ in PERIOD_KINDS]
    src, outs, batch = [], [], None
    try:
        for k in PERIOD_KINDS:
            row = []
            for f in fr[k]:
                b = Buf(f.nbytes, 0)
                b.put(f)
                row.append(b)
            src.append(row)
        outs = [[Buf(c.output_frame_bytes, 0) for _ in ts] for c, ts in zip(cs, PERIOD_TS)]
        batch = FlowBatch(cs)
        assert not batch.defersPlanes()
        ptrs = lambda p: [row[p].ptr for row in src]
        batch.runPeriod(batch.preparePeriod(ptrs(0), None, None, calculate_flow=False))
        batch.runPeriod(batch.preparePeriod(ptrs(1), None, None))
        plans, optr = [list(ts) for ts in PERIOD_TS], [[b.ptr for b in row] for row in outs]
        for p in (2, 3):
            batch.runPeriod(batch.preparePeriod(ptrs(p), plans, optr, 2))
            batch.sync()
            for i, (c, k) in enumerate(zip(cs, PERIOD_KINDS)):
                assert np.array_equal(c.readBlurredFlow(0), flows[(k, p - 1)]), (case.name, p, i, "flow of the warped pair")
                assert np.array_equal(c.readBlurredFlow(1), flows[(k, p)]), (case.name, p, i, "flow of the chain behind the update")
                assert all(c.readPhasePlane(s)[1] for s in range(3)), (case.name, p, i, "plane not complete")
                for j, t in enumerate(PERIOD_TS[i]):
                    want = oracle.warp_frames(fr[k][p - 2], fr[k][p - 1], flows[(k, p - 1)], g, np.float32(t), 2, 0.0, 255.0)
                    got = outs[i][j].get(dt)
                    bad = got != want
                    assert not bad.any(), (case.name, p, i, t, int(bad.sum()), np.flatnonzero(bad)[:4].tolist())
                    outs[i][j].reset()
    finally:
        if batch is not None:
            batch.close()
        for c in cs:
            c.close()
        for b in [x for row in outs + src for x in row]:
            b.free()


# ------------------------------------------------------------------------------------------------
# the planes
# ------------------------------------------------------------------------------------------------
PLANE_KINDS = ["noise", "drift-se", "drift-nw"]    # ("noise": every code value; for P010 the low byte must not leak into the top 8 bits)


def assert_planes(case, c, frames3, what):
    g = M.geometry(case)
    L = P.layout(g.H, g.rs, g.lw, g.lh)
    assert c.phase_plane_bytes == L.bytes, (case.name, what, c.phase_plane_bytes, L)
    for slot in range(3):
        words, complete = c.readPhasePlane(slot)
        assert complete, (case.name, what, slot)
        got = P.used(words, g.H, L, g.lw)
        want = P.plane(frames3[slot], bool(case.hdr), g.H, g.W, case.in_stride, L, g.lw)
        bad = got != want
        assert not bad.any(), (case.name, what, "slot", slot, int(bad.sum()), "first (row, phase pair, column j):",
                               [(int(y), int(p2), int(j) - L.mx) for y, p2, j in np.argwhere(bad)[:4]])


@pytest.mark.parametrize("key", list(M.DEEP_GEOMETRIES), ids=lambda k: "%s%dx%d-res%d" % ("hdr" if k[0] else "sdr", k[1], k[2], k[3]))
def test_phase_planes_equal_the_layout_model(native_lib, key):
    """Ring slot 0 is frame N - 2, slot 2 frame N.  The batch's leader asks for eager planes: on the aligned rs 4 shapes the batch would
    otherwise leave the planes to the warp launch; everywhere else the flag changes nothing."""
    from hopperrender_amd import capi
    from hopperrender_amd.calc import DeviceBuffer, FlowBatch
    case = next(c for c in M.DEEP_CASES if M.deep_geom_key(c) == key)
    fr = {k: case_frames(case, k)[:3] for k in PLANE_KINDS}
    c = make_context(case, 0)
    try:
        for x in fr["noise"]:
            c.updateFrame(x)
        assert_planes(case, c, fr["noise"], "lone")
    finally:
        c.close()
    cs = [make_context(case, capi.HF_FLAG_ASYNC | (capi.HF_FLAG_BATCH_EAGER_PLANES if i == 0 else 0)) for i in range(len(PLANE_KINDS))]
    dev, batch = [], None
    try:
        for k in PLANE_KINDS:
            row = []
            for f in fr[k]:
                b = DeviceBuffer(f.nbytes)
                b.upload(f)
                row.append(b)
            dev.append(row)
        batch = FlowBatch(cs)
        assert not batch.defersPlanes()
        for s in range(3):
            batch.updateFramesDeviceRef([row[s].ptr for row in dev])
        batch.sync()
        for i, (m, k) in enumerate(zip(cs, PLANE_KINDS)):
            assert_planes(case, m, fr[k], f"batch member {i}")
    finally:
        if batch is not None:
            batch.close()
        for m in cs:
            m.close()
        for b in [x for row in dev for x in row]:
            b.free()
