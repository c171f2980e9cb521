"""A lane's memory plan (legion_amd/csrc/pool_plan.h: the fan-out product of a shape, the bytes of its trainer-visible arrays, the list
of its private arrays) is host-only arithmetic that decides how large a pipeline's private block is; a pool allocates by walking
the list and creation checks on the GPU that a lane took exactly the plan's sum.  tests/cpu/pool_plan_test.cpp pins the sums to what
the library asked for per lane BEFORE the plan existed (printed on an MI355X), over every bucket class, forced
capacities, column slots on and off, one to six hops, and the 2^31 - 16384 limit.  Compiled on the host, no GPU, no HIP."""
from tests.rule_table import assert_catches, assert_passes, run_table

ROUNDED = "p.sum += pool_round(bytes);"


def test_the_plan_over_a_table_of_shapes(tmp_path):
    assert_passes(run_table(tmp_path, "pool_plan"))


def test_the_table_catches_a_dropped_rounding(tmp_path):
    """One entry -- the byte per id of tmp_part_ind -- added up without its 256-byte rounding, and the sums no longer are what a lane
    takes from its block: the test above is able to fail."""
    broken = "p.sum += what == PA_TMP_PART_IND ? bytes : pool_round(bytes);"
    assert_catches(run_table(tmp_path, "pool_plan", ("pool_plan.h", ROUNDED, broken)))
