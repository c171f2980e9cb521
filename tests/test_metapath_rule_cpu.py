"""The rule of metapath walks and of PinSAGE over a metapath (legion_amd/csrc/metapath_rule.h) is host-only text in front of the
launches.  tests/cpu/metapath_rule_test.cpp pins it over literal tables: every refusal at and beside its edge and their order, the
period index and the packed metapath at L in {1, 2, 3, 64}, where PinSAGE's termination draw and its visit fall at L in {1, 3}.  And one
test of what the reference (tests/metapath_ref.py) means: a step is uniform over its type's segment, and never leaves it.  No GPU."""
import numpy as np

from tests import metapath_ref as ref
from tests import walk_ref
from tests.rule_table import assert_catches, assert_passes, run_table

TYPE_RULE = "if (!metapath_types_legal(metapath, period, num_types)) return"


def test_the_rules_over_a_table_of_arguments(tmp_path):
    assert_passes(run_table(tmp_path, "metapath_rule"))


def test_the_table_catches_a_dropped_rule(tmp_path):
    """Without the rule on the metapath's entries a type the graph lacks comes back ok: the table says so."""
    assert_catches(run_table(tmp_path, "metapath_rule", ("metapath_rule.h", TYPE_RULE, "if (false) return")))


def test_a_step_is_uniform_over_its_segment_and_never_leaves_it():
    """200 000 first steps from the 65-entry row, type 63: its segment is entries 30 .. 64, one of them dead.  Every entry's count lies
    within five binomial standard deviations of n / 35, and no entry outside the segment is ever picked."""
    ref.assert_hand_graph()
    indptr, col, _ = ref.hand_graph()
    n, v, lo, hi = 200000, 8, 30, 65
    live = col.copy()
    live[indptr[v] + 40] = 5                                       # (the dead entry: counted like the others)
    _, eid = ref.step(indptr, live, ref.keys(64), np.full(n, v, dtype=np.int64), ref.C, walk_ref.draws(0, n))
    assert np.all(eid >= indptr[v] + lo) and np.all(eid < indptr[v] + hi)
    count = np.bincount(eid - indptr[v] - lo, minlength=hi - lo)
    p = 1.0 / (hi - lo)
    assert np.all(np.abs(count - n * p) <= 5 * np.sqrt(n * p * (1 - p))), count
