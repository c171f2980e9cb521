"""A lane's memory plan (legion_amd/csrc/pool_plan.h: the fan-out product of a shape, the bytes of its trainer-visible arrays, the list
of its private arrays) is host-only arithmetic that decides how large a pipeline's private block is; a pool allocates by walking
the list and creation checks on the GPU that a lane took exactly the plan's sum.  tests/cpu/pool_plan_test.cpp pins the sums to what
the library asked for per lane BEFORE the plan existed (printed on an MI355X), over every bucket class, forced
capacities, column slots on and off, one to six hops, and the 2^31 - 16384 limit.  Compiled with g++, no GPU, no HIP."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDED = "p.sum += pool_round(bytes);"


def _run(tmp_path, header_text=None):
    src = os.path.join(ROOT, "tests", "cpu", "pool_plan_test.cpp")
    if header_text is not None:
        (tmp_path / "pool_plan.h").write_text(header_text)
        text = open(src).read().replace("../../legion_amd/csrc/pool_plan.h", "pool_plan.h")
        (tmp_path / "t.cpp").write_text(text)
        src = str(tmp_path / "t.cpp")
    exe = str(tmp_path / "pool_plan_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe], cwd=tmp_path)
    return subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)


def test_the_plan_over_a_table_of_shapes(tmp_path):
    res = _run(tmp_path)
    assert res.returncode == 0 and " 0 failed" in res.stdout, res.stdout[-3000:]


def test_the_table_catches_a_dropped_rounding(tmp_path):
    """One entry -- the byte per id of tmp_part_ind -- added up without its 256-byte rounding, and the sums no longer are what a lane
    takes from its block: the test above is able to fail."""
    hdr = open(os.path.join(ROOT, "legion_amd", "csrc", "pool_plan.h")).read()
    assert hdr.count(ROUNDED) == 1
    hdr = hdr.replace(ROUNDED, "p.sum += what == PA_TMP_PART_IND ? bytes : pool_round(bytes);")
    hdr = hdr.replace('#include "sample_plan.h"', '#include "%s"' % os.path.join(ROOT, "legion_amd", "csrc", "sample_plan.h"))
    res = _run(tmp_path, hdr)
    assert res.returncode != 0 and "MISMATCH" in res.stdout, res.stdout[-3000:]
