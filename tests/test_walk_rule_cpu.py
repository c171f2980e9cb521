"""The argument rules of random walks and of PinSAGE's neighbour sampler (legion_amd/csrc/walk_rule.h: which calls legion_random_walk and
legion_pinsage_neighbors refuse) are host-only logic in front of the launches.  tests/cpu/walk_rule_test.cpp pins them over a literal
table: counts at -1, 0 and 1, length at 0 and 1, a negative base, the draw index at its last legal value, one past it and far past it
(a product near 2^62, a base at the end of int64), weighted at -1, 2 and 1 without a table, the probability at -0.0, 0, 1, the next float
above 1, NaN and +-inf, PinSAGE's visits and num_neighbors at 1024 and 1025, and the order of the checks.  Compiled on the host, no GPU, no
HIP."""
from tests.rule_table import assert_catches, assert_passes, run_table

PROB_RULE = "if (!walk_probability(restart_prob)) return"


def test_the_rules_over_a_table_of_arguments(tmp_path):
    assert_passes(run_table(tmp_path, "walk_rule"))


def test_the_table_catches_a_dropped_rule(tmp_path):
    """Without the walk's probability rule the entries with a restart_prob outside [0, 1] come back ok: the table says so, so the test
    above is able to fail."""
    assert_catches(run_table(tmp_path, "walk_rule", ("walk_rule.h", PROB_RULE, "if (false) return")))
