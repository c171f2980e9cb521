"""The gather's launch plan (legion_amd/csrc/gather_plan.h: row format, rows per tile, UNROLL and TAIL of the gather_kernel instance a
gather launches) is host-only logic that no GPU test can see -- the gathered rows do not depend on the tile size.
tests/cpu/gather_plan_test.cpp pins it over a literal table of shapes: every (dtype, out_dtype) pair, the tile rule's boundaries,
launches of few tiles, LEGION_GATHER_ROWS, and the refused inputs.  Compiled with g++, no GPU, no HIP."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULE = "while (p.rows < 256 && (int64_t)p.rows * 2 * row_bytes <= payload + payload / 4) p.rows *= 2;"


def _run(tmp_path, header_text=None):
    src = os.path.join(ROOT, "tests", "cpu", "gather_plan_test.cpp")
    if header_text is not None:
        (tmp_path / "gather_plan.h").write_text(header_text)
        text = open(src).read().replace("../../legion_amd/csrc/gather_plan.h", "gather_plan.h")
        (tmp_path / "t.cpp").write_text(text)
        src = str(tmp_path / "t.cpp")
    exe = str(tmp_path / "gather_plan_test")
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", inc, src, "-o", exe], cwd=tmp_path)
    return subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)


def test_the_plan_over_a_table_of_shapes(tmp_path):
    res = _run(tmp_path)
    assert res.returncode == 0 and " 0 failed" in res.stdout, res.stdout[-3000:]


def test_the_table_catches_a_looser_rule(tmp_path):
    """Without the quarter of a payload of margin the tile rule picks other tile sizes (D = 72: 64 rows instead of 128), and the
    table says so: the test above is able to fail."""
    hdr = open(os.path.join(ROOT, "legion_amd", "csrc", "gather_plan.h")).read()
    assert RULE in hdr
    hdr = hdr.replace(RULE, RULE.replace(" + payload / 4", "")).replace('#include "../../include/legion_hip.h"', '#include "legion_hip.h"')
    res = _run(tmp_path, hdr)
    assert res.returncode != 0 and "MISMATCH" in res.stdout, res.stdout[-3000:]
