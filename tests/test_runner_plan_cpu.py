"""GPURunner's sizing (legion_amd/csrc/runner_plan.h: the rows of a lane's and a pipe slot's feature buffer; lanes, groups in flight,
their arena and the overflow buffers) and the schedule's group rule (runner_schedule.h) decide how many lanes a server runs and
whether an oversized validation batch is served or stops it -- host-only arithmetic no GPU test pins.  tests/cpu/runner_plan_test.cpp
does, on both sides of every condition: the lanes' two caps, forced lanes, the schedule's largest group, none to three halvings
against free HBM, the slots' clamp, the overflow buffers granted and refused for each of their reasons, the 1.2 x rule scaled,
clamped and floored, and a schedule with a mode change and a gap in its local ids.  Compiled on the host, no GPU, no HIP."""
from tests.rule_table import assert_catches, assert_passes, run_table

SIX_TENTHS = "free_bytes / 10 * 6"


def test_the_plans_over_their_tables(tmp_path):
    assert_passes(run_table(tmp_path, "runner_plan"))


def test_the_table_catches_a_moved_threshold(tmp_path):
    """Lanes halved against 0.7 of the free HBM instead of 0.6, and the rows at the threshold's edge say so: the test above is able
    to fail."""
    assert_catches(run_table(tmp_path, "runner_plan", ("runner_plan.h", SIX_TENTHS, "free_bytes / 10 * 7")))
