"""The rule of layer-neighbour sampling (legion_amd/csrc/labor_rule.h: the hash of (src, salt), the integer predicate, which calls
legion_labor_count and legion_labor_edges refuse, the scratch size) is constexpr text that the kernels run on the device and
operators.hip asks in front of the launches.  tests/cpu/labor_rule_test.cpp pins it over a literal table: hash values computed with
synth.splitmix64_np (a negative salt and v = 2^31 - 1 among them), the predicate at d = fanout, at d = fanout + 1 with the largest number,
at h = 0, at d = 2^32 and 2^32 + 1 on both sides of the threshold and at fanout = 2^31 - 1, every refusal at and beside its edge, the
order of the checks, and the scratch size at m = 0, 1, 1 024, 1 025, 262 144, 262 145, 2^30 and 2^30 + 1.  Compiled with g++, no GPU,
no HIP."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# a rule of the header -> what it is replaced with
DROPPED = {
    "the fan-out check": ("    if (fanout < 1) return LaborRefusal::Fanout;\n", "", 2),
    "the capacity check": ("if (cap < 0 || cap > (int64_t)0x7FFFFFFF) return", "if (false) return", 1),
    "the salt hashed first": ("return splitmix64((uint64_t)salt); }", "return (uint64_t)salt; }", 1),
    "the high half of the degree": ("(uint64_t)h * dh + ", "", 1),
    "the total's entry of the scratch": ("8 * (labor_tiles(m) + 1 + labor_groups(m))", "8 * (labor_tiles(m) + labor_groups(m))", 1),
}


def _run(tmp_path, header_text=None):
    src = os.path.join(ROOT, "tests", "cpu", "labor_rule_test.cpp")
    if header_text is not None:
        (tmp_path / "labor_rule.h").write_text(header_text)
        text = open(src).read().replace("../../legion_amd/csrc/labor_rule.h", "labor_rule.h")
        (tmp_path / "t.cpp").write_text(text)
        src = str(tmp_path / "t.cpp")
    exe = str(tmp_path / "labor_rule_test")
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", inc, src, "-o", exe], cwd=tmp_path)
    return subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)


def test_the_rule_over_a_table(tmp_path):
    res = _run(tmp_path)
    assert res.returncode == 0 and " 0 failed" in res.stdout, res.stdout[-3000:]


@pytest.mark.parametrize("name", sorted(DROPPED))
def test_the_table_catches_a_dropped_rule(tmp_path, name):
    """Without one rule of the header the table says MISMATCH, so the test above is able to fail."""
    old, new, times = DROPPED[name]
    hdr = open(os.path.join(ROOT, "legion_amd", "csrc", "labor_rule.h")).read()
    assert hdr.count(old) == times, name
    hdr = hdr.replace(old, new).replace('#include "../../include/legion_hip.h"', '#include "legion_hip.h"')
    res = _run(tmp_path, hdr)
    assert res.returncode != 0 and "MISMATCH" in res.stdout, res.stdout[-3000:]
