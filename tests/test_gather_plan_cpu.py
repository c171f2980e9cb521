"""The gather's launch plan (legion_amd/csrc/gather_plan.h: row format, rows per tile, UNROLL and TAIL of the gather_kernel instance a
gather launches) is host-only logic that no GPU test can see -- the gathered rows do not depend on the tile size.
tests/cpu/gather_plan_test.cpp pins it over a literal table of shapes: every (dtype, out_dtype) pair, the tile rule's boundaries,
launches of few tiles, LEGION_GATHER_ROWS, and the refused inputs.  Compiled on the host, no GPU, no HIP."""
from tests.rule_table import assert_catches, assert_passes, run_table

RULE = "while (p.rows < 256 && (int64_t)p.rows * 2 * row_bytes <= payload + payload / 4) p.rows *= 2;"


def test_the_plan_over_a_table_of_shapes(tmp_path):
    assert_passes(run_table(tmp_path, "gather_plan"))


def test_the_table_catches_a_looser_rule(tmp_path):
    """Without the quarter of a payload of margin the tile rule picks other tile sizes (D = 72: 64 rows instead of 128), and the
    table says so: the test above is able to fail."""
    assert_catches(run_table(tmp_path, "gather_plan", ("gather_plan.h", RULE, RULE.replace(" + payload / 4", ""))))
