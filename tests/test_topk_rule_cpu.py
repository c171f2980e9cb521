"""The rule of the per-row selection (legion_amd/csrc/topk_rule.h: the exponential variate of an entry, the monotone integer of a float32
weight, the three keys, eligibility, which calls legion_row_topk and legion_topk_keys refuse, the scratch size) is constexpr text that the
kernels run on the device and operators.hip asks in front of the launches.  tests/cpu/topk_rule_test.cpp pins it over a literal table
whose values come from tests/topk_ref.py: E at x = 0, 2^64 - 1, 1 << 12, 2^63, 2^63 - 1, the two x on either side of the m < SQ branch and
two where the last series term decides the last bit; negative salts; the ordering at +-0, +-denormal, +-inf, NaN and FLT_MAX; every
refusal at and beside its edge and the order of the checks; the scratch size at n = 0, 1, 2^20 and 2^20 + 1.  The first test here checks
the table's values against topk_ref again, so that neither can drift.  Compiled on the host, no GPU, no HIP."""
import re

import numpy as np
import pytest

from tests import topk_ref as ref
from tests.rule_table import ROOT, assert_catches, assert_passes, run_table

# a rule of the header -> what it is replaced with
DROPPED = {
    "the salt hashed first": ("return topk_exp_keyed(labor_key(salt), e); }", "return topk_exp_keyed((uint64_t)salt, e); }", 1),
    "the m < SQ fold": ("    if (m < 0.7071067811865476) { m = 2.0 * m; ex -= 1; }\n", "", 1),
    "the last series term": ("    double p = 1.0 / 21.0;\n    p = p * z + 1.0 / 19.0;\n", "    double p = 1.0 / 19.0;\n", 1),
    "-0 folded to +0": ("    if (b == 0x80000000u) b = 0u;\n", "", 1),
    "the k > 64 check": ("    if (k > LEGION_TOPK_MAX_K) return TopkRefusal::KLarge;\n", "", 1),
}


def table(name):
    """The rows of one literal table of the C++ file, as lists of strings."""
    text = open(f"{ROOT}/tests/cpu/topk_rule_test.cpp").read()
    body = text.split(f" {name}[] = {{", 1)[1].split("\n};", 1)[0]
    body = re.sub(r"//[^\n]*", "", body)
    return [[x.strip() for x in row.split(",")] for row in re.findall(r"\{([^{}]*)\}", body)]


def test_the_tables_values_are_the_references():
    xs = table("variates")
    assert len(xs) == 10
    x = np.array([int(r[0][:-3], 16) for r in xs], dtype=np.uint64)
    want = np.array([int(r[1][:-3], 16) for r in xs], dtype=np.uint64)
    assert np.array_equal(ref.exp_of_hash(x).view(np.uint64), want)
    assert {0, 2 ** 64 - 1, 1 << 12, 2 ** 63, 2 ** 63 - 1} <= set(x.tolist())
    m = np.frexp(((x >> np.uint64(12)) * np.uint64(2) + np.uint64(1)).astype(np.float64))[0]
    below = np.nonzero((m[:-1] < ref.SQ) & (m[1:] >= ref.SQ) & (x[1:] - x[:-1] == 1 << 12))[0]
    assert below.size >= 1, "two neighbouring x on either side of the m < SQ branch"
    assert (ref.exp_of_hash(x, terms=10).view(np.uint64) != want).sum() >= 2, "the last series term decides some bit of the table"
    assert (ref.exp_of_hash(x, fold=False).view(np.uint64) != want).sum() >= 2, "so does the fold"
    for e, salt, bits in table("exps"):
        salt = -2 ** 63 if "- 1" in salt else int(salt[:-2])
        assert int(ref.exp_variate(np.array([int(e[:-2])]), salt).view(np.uint64)[0]) == int(bits[:-3], 16), (e, salt)
    assert any("-" in r[1] for r in table("exps")), "a negative salt"
    E = ref.exp_of_hash(np.array([0, 2 ** 64 - 1], dtype=np.uint64))
    assert abs(E[0] - 36.7368) < 1e-4 and abs(E[1] - 1.11e-16) < 1e-18


def test_the_variate_is_minus_log_u():
    """Over 2 x 10^6 hashed values the formula lies within 4.8e-16 relative of -np.log(u) (measured: 4.80e-16; the bound is the rounding
    of some fifteen operations), and 0 < E < 37."""
    x = ref.splitmix64_np(np.arange(2_000_000, dtype=np.uint64))
    u = ((x >> np.uint64(12)) * np.uint64(2) + np.uint64(1)).astype(np.float64) * 2.0 ** -53
    E = ref.exp_of_hash(x)
    assert np.max(np.abs(E + np.log(u)) / np.abs(np.log(u))) < 6e-16 and E.min() > 0 and E.max() < 37


def test_the_rule_over_a_table(tmp_path):
    assert_passes(run_table(tmp_path, "topk_rule"))


@pytest.mark.parametrize("name", sorted(DROPPED))
def test_the_table_catches_a_dropped_rule(tmp_path, name):
    """Without one rule of the header the table says MISMATCH, so the test above is able to fail."""
    assert_catches(run_table(tmp_path, "topk_rule", ("topk_rule.h",) + DROPPED[name]))
