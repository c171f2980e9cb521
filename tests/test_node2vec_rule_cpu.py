"""The argument rule of node2vec walks (legion_amd/csrc/node2vec_rule.h: which calls legion_node2vec_walk refuses, and the bias in double
the kernel gets) is host-only logic in front of the launch.  tests/cpu/node2vec_rule_test.cpp pins it over a literal table: counts, the
draw index at its edge, weighted with and without a table, max_tries at 0, 1, 256 and 257, p and q zero, negative, NaN and infinite, the
ratio of 16 at and past its edge, a graph unchecked and unsorted, and the order of the checks.  Compiled with g++, no GPU, no HIP."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIO_RULE = "if (least * (double)LEGION_NODE2VEC_MAX_BIAS < w.mx) return"


def _run(tmp_path, header_text=None):
    src = os.path.join(ROOT, "tests", "cpu", "node2vec_rule_test.cpp")
    if header_text is not None:
        (tmp_path / "node2vec_rule.h").write_text(header_text)
        text = open(src).read().replace("../../legion_amd/csrc/node2vec_rule.h", "node2vec_rule.h")
        (tmp_path / "t.cpp").write_text(text)
        src = str(tmp_path / "t.cpp")
    exe = str(tmp_path / "node2vec_rule_test")
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", inc, src, "-o", exe], cwd=tmp_path)
    return subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)


def test_the_rule_over_a_table_of_arguments(tmp_path):
    res = _run(tmp_path)
    assert res.returncode == 0 and " 0 failed" in res.stdout, res.stdout[-3000:]


def test_the_table_catches_a_dropped_rule(tmp_path):
    """Without the ratio rule the entries past a ratio of 16 come back ok: the table says so, so the test above is able to fail."""
    hdr = open(os.path.join(ROOT, "legion_amd", "csrc", "node2vec_rule.h")).read()
    assert hdr.count(RATIO_RULE) == 1
    hdr = hdr.replace(RATIO_RULE, "if (false) return").replace('#include "../../include/legion_hip.h"', '#include "legion_hip.h"')
    res = _run(tmp_path, hdr)
    assert res.returncode != 0 and "MISMATCH" in res.stdout, res.stdout[-3000:]
