"""GPURunner's sizing (legion_amd/csrc/runner_plan.h: the rows of a lane's and a pipe slot's feature buffer; lanes, groups in flight,
their arena and the overflow buffers) and the schedule's group rule (runner_schedule.h) decide how many lanes a server runs and
whether an oversized validation batch is served or stops it -- host-only arithmetic no GPU test pins.  tests/cpu/runner_plan_test.cpp
does, on both sides of every condition: the lanes' two caps, forced lanes, the schedule's largest group, none to three halvings
against free HBM, the slots' clamp, the overflow buffers granted and refused for each of their reasons, the 1.2 x rule scaled,
clamped and floored, and a schedule with a mode change and a gap in its local ids.  Compiled with g++, no GPU, no HIP."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "legion_amd", "csrc")
SIX_TENTHS = "free_bytes / 10 * 6"


def _run(tmp_path, header_text=None):
    src = os.path.join(ROOT, "tests", "cpu", "runner_plan_test.cpp")
    if header_text is not None:
        (tmp_path / "runner_plan.h").write_text(header_text)
        text = open(src).read().replace("../../legion_amd/csrc/runner_plan.h", "runner_plan.h")
        text = text.replace("../../legion_amd/csrc/runner_schedule.h", os.path.join(CSRC, "runner_schedule.h"))
        (tmp_path / "t.cpp").write_text(text)
        src = str(tmp_path / "t.cpp")
    exe = str(tmp_path / "runner_plan_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe], cwd=tmp_path)
    return subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)


def test_the_plans_over_their_tables(tmp_path):
    res = _run(tmp_path)
    assert res.returncode == 0 and " 0 failed" in res.stdout, res.stdout[-3000:]


def test_the_table_catches_a_moved_threshold(tmp_path):
    """Lanes halved against 0.7 of the free HBM instead of 0.6, and the rows at the threshold's edge say so: the test above is able
    to fail."""
    hdr = open(os.path.join(CSRC, "runner_plan.h")).read()
    assert hdr.count(SIX_TENTHS) == 1
    hdr = hdr.replace(SIX_TENTHS, "free_bytes / 10 * 7").replace('#include "pool_plan.h"', '#include "%s"' % os.path.join(CSRC, "pool_plan.h"))
    res = _run(tmp_path, hdr)
    assert res.returncode != 0 and "MISMATCH" in res.stdout, res.stdout[-3000:]
