"""The op order of a mini-batch (legion_amd/csrc/batch_ops.h: which ops a phase of a whole-batch enqueue issues, in which order, with
which op ids, and which gathers share a launch) is host-only logic that no GPU test sees cheaply -- an op on the wrong side of the
weave cut, or the seeds' rows gathered in a launch of their own, gives the same batch, only slower.  tests/cpu/batch_ops_test.cpp
pins it over a literal table: every phase x 0 ... 6 hops x serving / PreSC x CacheProfiling on / off, the whole-batch gather, and
the row bound of a gather launch.  Compiled on the host, no GPU, no HIP."""
import pytest

from tests.rule_table import assert_catches, assert_passes, run_table

RIDE_ALONG = "const bool seeds_ride = hop_num >= 2;"
REST_ORDER = ("        put(BatchOpKind::EndOfBatch, -1, -1, -1);\n"
              "        if (gathers)\n"
              "            for (int32_t h = -1; h < hop_num; h++) gather(h);\n")
REST_ORDER_BROKEN = ("        if (gathers)\n"
                     "            for (int32_t h = -1; h < hop_num; h++) gather(h);\n"
                     "        put(BatchOpKind::EndOfBatch, -1, -1, -1);\n")


def test_the_op_lists_over_a_literal_table(tmp_path):
    assert_passes(run_table(tmp_path, "batch_ops"))


@pytest.mark.parametrize("rule, broken", [(RIDE_ALONG, "const bool seeds_ride = false;"), (REST_ORDER, REST_ORDER_BROKEN)],
                         ids=["seeds_never_ride", "rest_ends_the_batch_after_its_gathers"])
def test_the_table_catches_a_changed_order(tmp_path, rule, broken):
    """Seeds that never ride along cost one more launch per group; an end of batch behind the gathers is the same kernels in another
    order.  Neither changes a batch's bits.  The table says so either way: the test above is able to fail."""
    assert_catches(run_table(tmp_path, "batch_ops", ("batch_ops.h", rule, broken)))
