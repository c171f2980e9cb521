"""The argument rules of the full-neighbour ops (legion_amd/csrc/in_edges_rule.h: which calls legion_row_offsets and legion_in_edges
refuse, and the scratch size of the first) are host-only logic in front of the launches.  tests/cpu/in_edges_rule_test.cpp pins them over
a literal table: n at -1, 0, 2^20 and 2^20 + 1, m at -1, 0, 2^31 - 1 and 2^31, the scratch size at and below its edge, and the order of
the checks.  Compiled with g++, no GPU, no HIP."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOTS_RULE = "if (m < 0 || m > (int64_t)0x7FFFFFFF) return"


def _run(tmp_path, header_text=None):
    src = os.path.join(ROOT, "tests", "cpu", "in_edges_rule_test.cpp")
    if header_text is not None:
        (tmp_path / "in_edges_rule.h").write_text(header_text)
        text = open(src).read().replace("../../legion_amd/csrc/in_edges_rule.h", "in_edges_rule.h")
        (tmp_path / "t.cpp").write_text(text)
        src = str(tmp_path / "t.cpp")
    exe = str(tmp_path / "in_edges_rule_test")
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", inc, src, "-o", exe], cwd=tmp_path)
    return subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)


def test_the_rules_over_a_table_of_arguments(tmp_path):
    res = _run(tmp_path)
    assert res.returncode == 0 and " 0 failed" in res.stdout, res.stdout[-3000:]


def test_the_table_catches_a_dropped_rule(tmp_path):
    """Without the rule on m the entries with m = -1 and m = 2^31 come back ok: the table says so, so the test above is able to fail."""
    hdr = open(os.path.join(ROOT, "legion_amd", "csrc", "in_edges_rule.h")).read()
    assert hdr.count(SLOTS_RULE) == 1
    hdr = hdr.replace(SLOTS_RULE, "if (false) return").replace('#include "../../include/legion_hip.h"', '#include "legion_hip.h"')
    res = _run(tmp_path, hdr)
    assert res.returncode != 0 and "MISMATCH" in res.stdout, res.stdout[-3000:]
