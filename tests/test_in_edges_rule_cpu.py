"""The argument rules of the full-neighbour ops (legion_amd/csrc/in_edges_rule.h: which calls legion_row_offsets and legion_in_edges
refuse, and the scratch size of the first) are host-only logic in front of the launches.  tests/cpu/in_edges_rule_test.cpp pins them over
a literal table: n at -1, 0, 2^20 and 2^20 + 1, m at -1, 0, 2^31 - 1 and 2^31, the scratch size at and below its edge, and the order of
the checks.  Compiled on the host, no GPU, no HIP."""
from tests.rule_table import assert_catches, assert_passes, run_table

SLOTS_RULE = "if (m < 0 || m > (int64_t)0x7FFFFFFF) return"


def test_the_rules_over_a_table_of_arguments(tmp_path):
    assert_passes(run_table(tmp_path, "in_edges_rule"))


def test_the_table_catches_a_dropped_rule(tmp_path):
    """Without the rule on m the entries with m = -1 and m = 2^31 come back ok: the table says so, so the test above is able to fail."""
    assert_catches(run_table(tmp_path, "in_edges_rule", ("in_edges_rule.h", SLOTS_RULE, "if (false) return")))
