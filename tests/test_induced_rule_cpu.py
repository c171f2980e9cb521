"""The rule of the vertex set and of induced subgraphs (legion_amd/csrc/induced_rule.h: the table's slots, shift, home slot and size,
which calls legion_node_set_build, legion_node_set_lookup, legion_induced_count, legion_induced_edges and legion_dst_offsets refuse, the
scratch size) is constexpr text that the kernels run on the device and operators.hip asks in front of the launches.
tests/cpu/induced_rule_test.cpp pins it over a literal table: the table's size at k = 0, 1, 127 .. 129, 256, 257, 2^19, 2^19 + 1 and 2^20,
home slots computed with Python integers (the ids of the last two slots of a 256-slot table and 2^31 - 1 among them), every refusal at
and beside its edge, the order of the checks, and the scratch size at m = 0, 1, 1 024, 1 025, 262 144, 262 145, 2^30 and 2^30 + 1.
Compiled on the host, no GPU, no HIP."""
import pytest

from tests.rule_table import assert_catches, assert_passes, run_table

# a rule -> the header that states it (induced_rule.h, or id_table_rule.h and kept_rule.h under it) and what it is replaced with
DROPPED = {
    "the set-size check": ("induced_rule.h", "    if (k < 0 || k > LEGION_NODE_SET_MAX_IDS) return InducedRefusal::SetSize;\n", "", 4),
    "the set-bytes check": ("induced_rule.h", "    if (set_bytes < node_set_bytes(k)) return InducedRefusal::SetBytes;\n", "", 4),
    "the capacity check": ("induced_rule.h", "if (cap < 0 || cap > (int64_t)0x7FFFFFFF) return", "if (false) return", 2),
    "the table at least twice the nodes": ("id_table_rule.h", "while (s < 2 * (int64_t)k) s <<= 1;", "while (s < (int64_t)k) s <<= 1;", 1),
    "the table at least 256 slots": ("id_table_rule.h", "int64_t s = 256;", "int64_t s = 128;", 1),
    "the hash": ("id_table_rule.h", "constexpr uint32_t ID_TABLE_HASH = 2654435769u;", "constexpr uint32_t ID_TABLE_HASH = 2654435761u;", 1),
    "the total's entry of the scratch": ("kept_rule.h", "8 * (kept_tiles(m) + 1 + kept_groups(m))", "8 * (kept_tiles(m) + kept_groups(m))", 1),
    "the lookup's count check": ("induced_rule.h", "    if (m < 0 || m > (int64_t)0x7FFFFFFF) return InducedRefusal::Slots;\n", "", 1),
}


def test_the_rule_over_a_table(tmp_path):
    assert_passes(run_table(tmp_path, "induced_rule"))


@pytest.mark.parametrize("name", sorted(DROPPED))
def test_the_table_catches_a_dropped_rule(tmp_path, name):
    """Without one rule of the headers the table says MISMATCH, so the test above is able to fail."""
    assert_catches(run_table(tmp_path, "induced_rule", DROPPED[name]))
