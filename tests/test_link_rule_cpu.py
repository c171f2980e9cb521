"""The argument rules of the link-prediction seed ops (legion_amd/csrc/link_rule.h: which calls legion_find_edges, legion_negative_sample
and legion_unique_ids refuse, and the scratch size of the last) are host-only logic in front of the launches.
tests/cpu/link_rule_test.cpp pins them over a literal table: counts, k, the draw index at its edge and far past it, exclude outside
[0, 3], max_tries at 0, 1, 256 and 257, a graph unchecked and unsorted with and without the edge exclusion, the id limit, the scratch size
at and below its edge, outputs overlapping the input by one element, and the order of the checks.  Compiled on the host, no GPU, no HIP."""
import pytest

from tests.rule_table import assert_catches, assert_passes, run_table

SORTED_RULE = "if ((exclude & 2) && rows_sorted != 1) return"


def test_the_rules_over_a_table_of_arguments(tmp_path):
    assert_passes(run_table(tmp_path, "link_rule"))


def test_the_table_catches_a_dropped_rule(tmp_path):
    """Without the sorted-rows rule the entries that exclude edges on an unchecked graph come back ok: the table says so, so the test
    above is able to fail."""
    assert_catches(run_table(tmp_path, "link_rule", ("link_rule.h", SORTED_RULE, "if (false) return")))


# a rule of the id table that unique_ids keeps in its scratch (id_table_rule.h, under link_rule.h) -> what it is replaced with
TABLE_RULES = {
    "the table at least twice the ids": ("while (s < 2 * (int64_t)k) s <<= 1;", "while (s < (int64_t)k) s <<= 1;"),
    "the table at least 256 slots": ("int64_t s = 256;", "int64_t s = 128;"),
    "the hash": ("constexpr uint32_t ID_TABLE_HASH = 2654435769u;", "constexpr uint32_t ID_TABLE_HASH = 2654435761u;"),
}


@pytest.mark.parametrize("name", sorted(TABLE_RULES))
def test_the_table_catches_a_changed_id_table(tmp_path, name):
    """The scratch size at m = 128 and 129 sees the table's slots, the home slots its hash: with either changed the table says MISMATCH."""
    assert_catches(run_table(tmp_path, "link_rule", ("id_table_rule.h",) + TABLE_RULES[name]))
