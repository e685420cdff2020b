"""GPU: the refinement chain where a window's best candidates cost exactly the same.  The reference takes a window's offset by a sequential
scan with a strict '<' (determineLowestLayerKernelSDR.h:19-24; hf_oracle.c hfo_determine_lowest_layer): among equal sums the lowest candidate
index wins.  hf_flow.hip does not scan; it keeps that rule by hand at five sites:
  * the per-lane `sum < b.sum` over ascending cz;
  * best_min's `(s == b.sum && cz < b.cz)` clause, on which the sentinel Best{0xFFFFFFFF, 16} of the candidates cz >= R rests too;
  * group_argmin<2 | 4 | 16 | 64>, through another sequence of best_xor stages per group width, once on gathered SADs and once on SADs
    summed from the tables;
  * resolve_pending, the lazy argmin of a large-window step;
  * flow_big_argmin_kernel, the explicit one.
A site that lost the clause, or a fusion that reordered lanes, would be wrong only in windows whose two best candidates tie, and no other
content of the suite has more than a handful of those above level 4.  Here every member of a batch gets a tie kind of
tests/chain_content.py in turn: flat frames with luma marks that are mirror images about a window's centre, so that candidates -d and +d
of that window cost the same and beat d = 0 -- at every step class from 128 down to 2 on both axes, in full tiles, in reusing windows for
the table bodies, at R 16, 11 and 5, with tied pairs (7, 9), (6, 10), (5, 11), (8, 9), .. (tests/test_chain_tie_model.py proves it on the
CPU, and that the last minimum, or a best_xor stage that keeps its partner on equality, changes the chain's result on this content).
Machinery and bar are those of tests/test_chain_variants_gpu.py: two consecutive pairs and a graph replay, offsets, blurred flow and total
frame delta bit-identical to the oracle's for every member -- integer arithmetic, no tolerance -- and the table-window counters where
tables run at R 16.  A batch size of 1 is a lone context through its own calculateOpticalFlow, once per kind."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_tie_model as T  # noqa: E402
import chain_variant_model as M  # noqa: E402
from chain_content import TIE_KINDS  # noqa: E402
from test_chain_variants_gpu import assert_members, assert_table_counters, case_frames, make_members, oracle_results, read, run_case  # noqa: E402

pytestmark = pytest.mark.gpu


def more_flags(case):
    from hopperrender_amd import capi
    return {None: 0, T.NO_LAZY: capi.HF_FLAG_NO_LAZY_ARGMIN, T.NO_GRAPH: capi.HF_FLAG_NO_GRAPH}[T.FLAGS.get(case.name)]


def run_lone(case):
    """One context per kind, no batch: both pairs against the oracle, the second once more (the context's own cached graph, if it keeps one)."""
    counted = bool(M.tables_on(case)) and case.R == 16
    for kind in TIE_KINDS:
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


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.name)
def test_tied_chain_matches_oracle(native_lib, case):
    if case.n == 1:
        run_lone(case)
    else:
        run_case(case, kinds=T.member_kinds(case), more_flags=more_flags(case))
