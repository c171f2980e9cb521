"""The op order of a mini-batch (legion_amd/csrc/batch_ops.h: which ops a phase of a whole-batch enqueue issues, in which order, with
which op ids, and which gathers share a launch) is host-only logic that no GPU test sees cheaply -- an op on the wrong side of the
weave cut, or the seeds' rows gathered in a launch of their own, gives the same batch, only slower.  tests/cpu/batch_ops_test.cpp
pins it over a literal table: every phase x 0 ... 6 hops x serving / PreSC x CacheProfiling on / off, the whole-batch gather, and
the row bound of a gather launch.  Compiled with g++, no GPU, no HIP."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RIDE_ALONG = "const bool seeds_ride = hop_num >= 2;"
REST_ORDER = ("        put(BatchOpKind::EndOfBatch, -1, -1, -1);\n"
              "        if (gathers)\n"
              "            for (int32_t h = -1; h < hop_num; h++) gather(h);\n")
REST_ORDER_BROKEN = ("        if (gathers)\n"
                     "            for (int32_t h = -1; h < hop_num; h++) gather(h);\n"
                     "        put(BatchOpKind::EndOfBatch, -1, -1, -1);\n")


def _run(tmp_path, header_text=None):
    src = os.path.join(ROOT, "tests", "cpu", "batch_ops_test.cpp")
    if header_text is not None:
        (tmp_path / "batch_ops.h").write_text(header_text)
        text = open(src).read().replace("../../legion_amd/csrc/batch_ops.h", "batch_ops.h")
        (tmp_path / "t.cpp").write_text(text)
        src = str(tmp_path / "t.cpp")
    exe = str(tmp_path / "batch_ops_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", src, "-o", exe], cwd=tmp_path)
    return subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)


def test_the_op_lists_over_a_literal_table(tmp_path):
    res = _run(tmp_path)
    assert res.returncode == 0 and " 0 failed" in res.stdout, res.stdout[-3000:]


@pytest.mark.parametrize("rule, broken", [(RIDE_ALONG, "const bool seeds_ride = false;"), (REST_ORDER, REST_ORDER_BROKEN)],
                         ids=["seeds_never_ride", "rest_ends_the_batch_after_its_gathers"])
def test_the_table_catches_a_changed_order(tmp_path, rule, broken):
    """Seeds that never ride along cost one more launch per group; an end of batch behind the gathers is the same kernels in another
    order.  Neither changes a batch's bits.  The table says so either way: the test above is able to fail."""
    hdr = open(os.path.join(ROOT, "legion_amd", "csrc", "batch_ops.h")).read()
    assert hdr.count(rule) == 1
    res = _run(tmp_path, hdr.replace(rule, broken))
    assert res.returncode != 0 and "MISMATCH" in res.stdout, res.stdout[-3000:]
