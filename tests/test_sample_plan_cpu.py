"""The sampler's launch plans (legion_amd/csrc/sample_plan.h: the hash-bucket class and list sizes of a pool; the grids, partition
tile and de-duplication instance of a hop) are host-only logic that no GPU test can see -- the de-duplication's result never depends
on the hash, so a wrong class, claim count, tile or grid gives the same bits, only slower.  tests/cpu/sample_plan_test.cpp pins them
over a literal table of shapes: every class boundary, the PreSC hint and its +10 %, LEGION_LDS_SMALL_BUCKETS, forced capacities,
claims per thread, the partition tile, the grids' caps and the one-round rule.  Compiled on the host, no GPU, no HIP."""
import pytest

from tests.rule_table import assert_catches, assert_passes, run_table

ONE_ROUND = "if (total > resident && total < 6 * resident)"
MARGIN = "return counted * 11 / 10;"


def test_the_plans_over_a_table_of_shapes(tmp_path):
    assert_passes(run_table(tmp_path, "sample_plan"))


@pytest.mark.parametrize("rule, broken", [(ONE_ROUND, "if (false)"), (MARGIN, "return counted;")], ids=["one_round_rule", "hint_margin"])
def test_the_table_catches_a_dropped_rule(tmp_path, rule, broken):
    """Without the one-round rule B = 8000 on 64 lanes samples with 64 workgroups per lane instead of 32; without the hint's +10 % the
    class and claims-per-thread boundaries move.  The table says so either way: the test above is able to fail."""
    assert_catches(run_table(tmp_path, "sample_plan", ("sample_plan.h", rule, broken)))
