"""The argument rules of the link-prediction seed ops (legion_amd/csrc/link_rule.h: which calls legion_find_edges, legion_negative_sample
and legion_unique_ids refuse, and the scratch size of the last) are host-only logic in front of the launches.
tests/cpu/link_rule_test.cpp pins them over a literal table: counts, k, the draw index at its edge and far past it, exclude outside
[0, 3], max_tries at 0, 1, 256 and 257, a graph unchecked and unsorted with and without the edge exclusion, the id limit, the scratch size
at and below its edge, outputs overlapping the input by one element, and the order of the checks.  Compiled with g++, no GPU, no HIP."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SORTED_RULE = "if ((exclude & 2) && rows_sorted != 1) return"


def _run(tmp_path, header_text=None):
    src = os.path.join(ROOT, "tests", "cpu", "link_rule_test.cpp")
    if header_text is not None:
        (tmp_path / "link_rule.h").write_text(header_text)
        text = open(src).read().replace("../../legion_amd/csrc/link_rule.h", "link_rule.h")
        (tmp_path / "t.cpp").write_text(text)
        src = str(tmp_path / "t.cpp")
    exe = str(tmp_path / "link_rule_test")
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", inc, src, "-o", exe], cwd=tmp_path)
    return subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)


def test_the_rules_over_a_table_of_arguments(tmp_path):
    res = _run(tmp_path)
    assert res.returncode == 0 and " 0 failed" in res.stdout, res.stdout[-3000:]


def test_the_table_catches_a_dropped_rule(tmp_path):
    """Without the sorted-rows rule the entries that exclude edges on an unchecked graph come back ok: the table says so, so the test
    above is able to fail."""
    hdr = open(os.path.join(ROOT, "legion_amd", "csrc", "link_rule.h")).read()
    assert hdr.count(SORTED_RULE) == 1
    hdr = hdr.replace(SORTED_RULE, "if (false) return").replace('#include "../../include/legion_hip.h"', '#include "legion_hip.h"')
    res = _run(tmp_path, hdr)
    assert res.returncode != 0 and "MISMATCH" in res.stdout, res.stdout[-3000:]
