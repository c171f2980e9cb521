"""The argument rules of random walks and of PinSAGE's neighbour sampler (legion_amd/csrc/walk_rule.h: which calls legion_random_walk and
legion_pinsage_neighbors refuse) are host-only logic in front of the launches.  tests/cpu/walk_rule_test.cpp pins them over a literal
table: counts at -1, 0 and 1, length at 0 and 1, a negative base, the draw index at its last legal value, one past it and far past it
(a product near 2^62, a base at the end of int64), weighted at -1, 2 and 1 without a table, the probability at -0.0, 0, 1, the next float
above 1, NaN and +-inf, PinSAGE's visits and num_neighbors at 1024 and 1025, and the order of the checks.  Compiled with g++, no GPU, no
HIP."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROB_RULE = "if (!walk_probability(restart_prob)) return"


def _run(tmp_path, header_text=None):
    src = os.path.join(ROOT, "tests", "cpu", "walk_rule_test.cpp")
    if header_text is not None:
        (tmp_path / "walk_rule.h").write_text(header_text)
        text = open(src).read().replace("../../legion_amd/csrc/walk_rule.h", "walk_rule.h")
        (tmp_path / "t.cpp").write_text(text)
        src = str(tmp_path / "t.cpp")
    exe = str(tmp_path / "walk_rule_test")
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", inc, src, "-o", exe], cwd=tmp_path)
    return subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)


def test_the_rules_over_a_table_of_arguments(tmp_path):
    res = _run(tmp_path)
    assert res.returncode == 0 and " 0 failed" in res.stdout, res.stdout[-3000:]


def test_the_table_catches_a_dropped_rule(tmp_path):
    """Without the walk's probability rule the entries with a restart_prob outside [0, 1] come back ok: the table says so, so the test
    above is able to fail."""
    hdr = open(os.path.join(ROOT, "legion_amd", "csrc", "walk_rule.h")).read()
    assert hdr.count(PROB_RULE) == 1
    hdr = hdr.replace(PROB_RULE, "if (false) return").replace('#include "../../include/legion_hip.h"', '#include "legion_hip.h"')
    res = _run(tmp_path, hdr)
    assert res.returncode != 0 and "MISMATCH" in res.stdout, res.stdout[-3000:]
