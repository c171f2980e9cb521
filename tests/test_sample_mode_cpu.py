"""The sampler's mode rules (legion_amd/csrc/sample_mode.h: which (replace, edge_ids, weighted) a pool may be set to, what a launch
needs on top, and the draw rule -- the kernel instance -- a mode picks) are host-only logic behind every setter and enqueue path.
tests/cpu/sample_mode_test.cpp pins them over a literal table: all eight combinations, fan-outs 1, 256 and 257, a graph with and
without a prefix table, values outside {0, 1}.  Compiled on the host, no GPU, no HIP."""
from tests.rule_table import assert_catches, assert_passes, run_table

WEIGHTED_NEEDS_REPLACE = "if (m.weighted && !m.replace) return"


def test_the_rules_over_a_table_of_modes(tmp_path):
    assert_passes(run_table(tmp_path, "sample_mode"))


def test_the_table_catches_a_dropped_rule(tmp_path):
    """Without "weighted needs replacement" the twelve weighted-without-replacement entries come back ok (or as a fan-out or table
    refusal): the table says so, so the test above is able to fail."""
    assert_catches(run_table(tmp_path, "sample_mode", ("sample_mode.h", WEIGHTED_NEEDS_REPLACE, "if (false) return")))
