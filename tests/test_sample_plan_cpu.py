"""The sampler's launch plans (legion_amd/csrc/sample_plan.h: the hash-bucket class and list sizes of a pool; the grids, partition
tile and de-duplication instance of a hop) are host-only logic that no GPU test can see -- the de-duplication's result never depends
on the hash, so a wrong class, claim count, tile or grid gives the same bits, only slower.  tests/cpu/sample_plan_test.cpp pins them
over a literal table of shapes: every class boundary, the PreSC hint and its +10 %, LEGION_LDS_SMALL_BUCKETS, forced capacities,
claims per thread, the partition tile, the grids' caps and the one-round rule.  Compiled with g++, no GPU, no HIP."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE_ROUND = "if (total > resident && total < 6 * resident)"
MARGIN = "return counted * 11 / 10;"


def _run(tmp_path, header_text=None):
    src = os.path.join(ROOT, "tests", "cpu", "sample_plan_test.cpp")
    if header_text is not None:
        (tmp_path / "sample_plan.h").write_text(header_text)
        text = open(src).read().replace("../../legion_amd/csrc/sample_plan.h", "sample_plan.h")
        (tmp_path / "t.cpp").write_text(text)
        src = str(tmp_path / "t.cpp")
    exe = str(tmp_path / "sample_plan_test")
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", inc, src, "-o", exe], cwd=tmp_path)
    return subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)


def test_the_plans_over_a_table_of_shapes(tmp_path):
    res = _run(tmp_path)
    assert res.returncode == 0 and " 0 failed" in res.stdout, res.stdout[-3000:]


@pytest.mark.parametrize("rule, broken", [(ONE_ROUND, "if (false)"), (MARGIN, "return counted;")], ids=["one_round_rule", "hint_margin"])
def test_the_table_catches_a_dropped_rule(tmp_path, rule, broken):
    """Without the one-round rule B = 8000 on 64 lanes samples with 64 workgroups per lane instead of 32; without the hint's +10 % the
    class and claims-per-thread boundaries move.  The table says so either way: the test above is able to fail."""
    hdr = open(os.path.join(ROOT, "legion_amd", "csrc", "sample_plan.h")).read()
    assert hdr.count(rule) == 1
    hdr = hdr.replace(rule, broken).replace('#include "../../include/legion_hip.h"', '#include "legion_hip.h"')
    res = _run(tmp_path, hdr)
    assert res.returncode != 0 and "MISMATCH" in res.stdout, res.stdout[-3000:]
