"""GPU: the refinement chain at the top of its numeric range.  hf_flow.hip keeps its sums just inside narrow integer widths -- a strip's
two halves side by side in one register, 16 candidates x u16 per 2 x 2 block in the SAD tables, u16 pairs through the packed butterfly up
to 16 blocks (48,960), u32 atomics and a wrapping (sum << delta) + npix * bias for the large windows -- and every one of those arguments
is about the LARGEST SAD there is, 765 per pixel, which no other content of the suite comes near (full-range noise averages a third of it).
Here every member of a batch gets a saturation kind of tests/chain_content.py: "saturated", "sat-y", "sat-uv" (every entry at its maximum,
zero flow, every window reuses; the first-level sum behind m_totalFrameDelta wraps at delta 10; P010 codes whose low byte would show in a
plane build that rounds) and "specks" (near-saturated, the winner of most windows of 32, 16 and 8 depends on the high bits of the sums --
tests/test_chain_saturation_model.py proves it on the CPU, together with the matrix's coverage of the kernel variants and tile classes).
Machinery and bar are those of tests/test_chain_variants_gpu.py: two consecutive pairs and a graph replay, offsets, blurred flow and total
frame delta bit-identical to the oracle's for every member, the table-window counters where tables run at R 16.  A batch size of 1 is a
lone context through its own calculateOpticalFlow, once per kind."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_saturation_model as S  # noqa: E402
import chain_variant_model as M  # noqa: E402
from chain_content import SAT_KINDS  # noqa: E402
from test_chain_variants_gpu import assert_members, assert_table_counters, case_frames, make_members, oracle_results, read, run_case  # noqa: E402

pytestmark = pytest.mark.gpu


def more_flags(case):
    from hopperrender_amd import capi
    return {None: 0, S.NO_LAZY: capi.HF_FLAG_NO_LAZY_ARGMIN, S.NO_GRAPH: capi.HF_FLAG_NO_GRAPH}[S.FLAGS.get(case.name)]


def run_lone(case):
    """One context per kind, no batch: both pairs against the oracle, the second once more (the context's own cached graph, if it keeps one)."""
    counted = bool(M.tables_on(case)) and case.R == 16
    for kind in SAT_KINDS:
        f = case_frames(case, kind)
        c, = make_members(case, more_flags=more_flags(case))
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


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c.name)
def test_saturated_chain_matches_oracle(native_lib, case):
    if case.n == 1:
        run_lone(case)
    else:
        run_case(case, kinds=S.member_kinds(case), more_flags=more_flags(case))
