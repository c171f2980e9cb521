"""The rule of layer-neighbour sampling (legion_amd/csrc/labor_rule.h: the hash of (src, salt), the integer predicate, which calls
legion_labor_count and legion_labor_edges refuse, the scratch size) is constexpr text that the kernels run on the device and
operators.hip asks in front of the launches.  tests/cpu/labor_rule_test.cpp pins it over a literal table: hash values computed with
synth.splitmix64_np (a negative salt and v = 2^31 - 1 among them), the predicate at d = fanout, at d = fanout + 1 with the largest number,
at h = 0, at d = 2^32 and 2^32 + 1 on both sides of the threshold and at fanout = 2^31 - 1, every refusal at and beside its edge, the
order of the checks, and the scratch size at m = 0, 1, 1 024, 1 025, 262 144, 262 145, 2^30 and 2^30 + 1.  Compiled on the host, no GPU,
no HIP."""
import pytest

from tests.rule_table import assert_catches, assert_passes, run_table

# a rule -> the header that states it (labor_rule.h, or kept_rule.h under it) and what it is replaced with
DROPPED = {
    "the fan-out check": ("labor_rule.h", "    if (fanout < 1) return LaborRefusal::Fanout;\n", "", 2),
    "the capacity check": ("labor_rule.h", "if (cap < 0 || cap > (int64_t)0x7FFFFFFF) return", "if (false) return", 1),
    "the salt hashed first": ("labor_rule.h", "return splitmix64((uint64_t)salt); }", "return (uint64_t)salt; }", 1),
    "the high half of the degree": ("labor_rule.h", "(uint64_t)h * dh + ", "", 1),
    "the total's entry of the scratch": ("kept_rule.h", "8 * (kept_tiles(m) + 1 + kept_groups(m))", "8 * (kept_tiles(m) + kept_groups(m))", 1),
}


def test_the_rule_over_a_table(tmp_path):
    assert_passes(run_table(tmp_path, "labor_rule"))


@pytest.mark.parametrize("name", sorted(DROPPED))
def test_the_table_catches_a_dropped_rule(tmp_path, name):
    """Without one rule of the headers the table says MISMATCH, so the test above is able to fail."""
    assert_catches(run_table(tmp_path, "labor_rule", DROPPED[name]))
