"""The sampler's mode rules (legion_amd/csrc/sample_mode.h: which (replace, edge_ids, weighted) a pool may be set to, what a launch
needs on top, and the draw rule -- the kernel instance -- a mode picks) are host-only logic behind every setter and enqueue path.
tests/cpu/sample_mode_test.cpp pins them over a literal table: all eight combinations, fan-outs 1, 256 and 257, a graph with and
without a prefix table, values outside {0, 1}.  Compiled with g++, no GPU, no HIP."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTED_NEEDS_REPLACE = "if (m.weighted && !m.replace) return"


def _run(tmp_path, header_text=None):
    src = os.path.join(ROOT, "tests", "cpu", "sample_mode_test.cpp")
    if header_text is not None:
        (tmp_path / "sample_mode.h").write_text(header_text)
        text = open(src).read().replace("../../legion_amd/csrc/sample_mode.h", "sample_mode.h")
        (tmp_path / "t.cpp").write_text(text)
        src = str(tmp_path / "t.cpp")
    exe = str(tmp_path / "sample_mode_test")
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", inc, src, "-o", exe], cwd=tmp_path)
    return subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)


def test_the_rules_over_a_table_of_modes(tmp_path):
    res = _run(tmp_path)
    assert res.returncode == 0 and " 0 failed" in res.stdout, res.stdout[-3000:]


def test_the_table_catches_a_dropped_rule(tmp_path):
    """Without "weighted needs replacement" the twelve weighted-without-replacement entries come back ok (or as a fan-out or table
    refusal): the table says so, so the test above is able to fail."""
    hdr = open(os.path.join(ROOT, "legion_amd", "csrc", "sample_mode.h")).read()
    assert hdr.count(WEIGHTED_NEEDS_REPLACE) == 1
    hdr = hdr.replace(WEIGHTED_NEEDS_REPLACE, "if (false) return").replace('#include "../../include/legion_hip.h"', '#include "legion_hip.h"')
    res = _run(tmp_path, hdr)
    assert res.returncode != 0 and "MISMATCH" in res.stdout, res.stdout[-3000:]
