"""The rule of temporal neighbour sampling (legion_amd/csrc/temporal_rule.h) is constexpr text that the kernels run on the device and
operators.hip asks in front of the launches.  tests/cpu/temporal_rule_test.cpp pins the candidate test, the slot counts, the ranks of
LAST, the draws, the refusals in their order and the scratch size over a literal table; the same draws and ranks are checked against
tests/temporal_ref.py here.  Compiled on the host, no GPU, no HIP."""
from tests import temporal_ref as ref
from tests.rule_table import assert_passes, run_table


def test_the_rule_over_a_table(tmp_path):
    assert_passes(run_table(tmp_path, "temporal_rule"))


def test_the_references_ranks_are_the_tables():
    """The table's Floyd draws at C = 7, f = 3 are the reference's candidates (3, ., 5); LAST and a row taken whole are contiguous."""
    assert ref.ranks(0, 0, 7, 3, ref.UNIFORM, False)[::2] == [3, 5] and ref.ranks(5, 9, 100, 64, ref.UNIFORM, True)[63] == 95
    assert ref.ranks(1, 2, 7, 3, ref.LAST, False) == [4, 5, 6] and ref.ranks(1, 2, 5, 64, ref.UNIFORM, False) == [0, 1, 2, 3, 4]
    assert ref.ranks(1, 2, 5, -1, ref.LAST, False) == [0, 1, 2, 3, 4] and ref.ranks(1, 2, 0, 5, ref.UNIFORM, True) == []
    for salt in range(50):
        r = ref.ranks(salt, 3, 9, 5, ref.UNIFORM, False)
        assert len(set(r)) == 5 and min(r) >= 0 and max(r) < 9
