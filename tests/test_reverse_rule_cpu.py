"""The rules of the reverse CSR (legion_amd/csrc/reverse_rule.h: which graphs legion_graph_build_reverse refuses, the class that sorts a
reverse row of a given length, a long row's runs, merge passes and buffers, the scan's levels and scratch, the lists' capacities) are
host-only logic in front of the launches.  tests/cpu/reverse_rule_test.cpp pins them over a literal table: node_num at 2^28 and one
past it, lengths at 1, 2, 64, 65, 4 096, 4 097 and where the number of passes changes, the scan at 2^20 and 2^20 + 1 vertices.
Compiled on the host, no GPU, no HIP."""
from tests.rule_table import assert_catches, assert_passes, run_table

NODES_RULE = "if (node_num > LEGION_REVERSE_MAX_NODES) return"
TILE_RULE = "if (len <= LG_REVERSE_TILE) return ReverseClass::Tile;"


def test_the_rules_over_a_table_of_arguments(tmp_path):
    assert_passes(run_table(tmp_path, "reverse_rule"))


def test_the_table_catches_a_dropped_rule(tmp_path):
    """Without the rule on node_num the entries past 2^28 come back ok: the table says so, so the test above is able to fail."""
    assert_catches(run_table(tmp_path, "reverse_rule", ("reverse_rule.h", NODES_RULE, "if (false) return")))


def test_the_table_catches_a_moved_class_boundary(tmp_path):
    """A workgroup's class that ends one entry early sends a row of 4 096 entries to the merge: the table names the length."""
    res = run_table(tmp_path, "reverse_rule", ("reverse_rule.h", TILE_RULE, "if (len < LG_REVERSE_TILE) return ReverseClass::Tile;"))
    assert_catches(res)
    assert "length 4096" in res.stdout
