"""The argument rule of node2vec walks (legion_amd/csrc/node2vec_rule.h: which calls legion_node2vec_walk refuses, and the bias in double
the kernel gets) is host-only logic in front of the launch.  tests/cpu/node2vec_rule_test.cpp pins it over a literal table: counts, the
draw index at its edge, weighted with and without a table, max_tries at 0, 1, 256 and 257, p and q zero, negative, NaN and infinite, the
ratio of 16 at and past its edge, a graph unchecked and unsorted, and the order of the checks.  Compiled on the host, no GPU, no HIP."""
from tests.rule_table import assert_catches, assert_passes, run_table

RATIO_RULE = "if (least * (double)LEGION_NODE2VEC_MAX_BIAS < w.mx) return"


def test_the_rule_over_a_table_of_arguments(tmp_path):
    assert_passes(run_table(tmp_path, "node2vec_rule"))


def test_the_table_catches_a_dropped_rule(tmp_path):
    """Without the ratio rule the entries past a ratio of 16 come back ok: the table says so, so the test above is able to fail."""
    assert_catches(run_table(tmp_path, "node2vec_rule", ("node2vec_rule.h", RATIO_RULE, "if (false) return")))
