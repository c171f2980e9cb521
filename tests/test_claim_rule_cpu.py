"""The bit formats through which the kernels of a sampled hop talk (legion_amd/csrc/claim_rule.h: the hash with its bucket and sub-bucket
bits, the claim pair, the claim lists' layout, the de-duplication's table words and the verdict of a surviving word, the losers' codes, the
compaction's look-back word) are constexpr text that kernels_sample.hip runs on the device.  tests/cpu/claim_rule_test.cpp pins them over
literal tables and the properties the kernels rest on; the first test here computes the hash and home literals again in numpy, so that
neither can drift.  Compiled on the host, no GPU, no HIP."""
import re

import numpy as np
import pytest

from tests.rule_table import ROOT, assert_catches, assert_passes, run_table

# a rule of the header -> what it is replaced with
MUTATED = {
    "the pending bit at bit 30": ("LG_TAB_PENDING = 0x80000000u;", "LG_TAB_PENDING = 0x40000000u;"),
    "st_word shifts the edges by 32": ("(uint64_t)(uint32_t)e << 31)", "(uint64_t)(uint32_t)e << 32)"),
    "the list index without its NB factor": ("(k >> LG_CLAIM_CHUNK_BITS) * nb) + b)", "(k >> LG_CLAIM_CHUNK_BITS)) + b)"),
    "the sub-bucket without its shift": ("return (h >> bb) & (passes - 1u);", "return h & (passes - 1u);"),
    "another hash multiplier": ("x *= 0x846ca68bu;", "x *= 0x846ca68du;"),
}


def table(name):
    """The rows of one literal table of the C++ file, as lists of strings."""
    text = open(f"{ROOT}/tests/cpu/claim_rule_test.cpp").read()
    body = text.split(f" {name}[] = {{", 1)[1].split("\n};", 1)[0]
    return [[x.strip() for x in row.split(",")] for row in re.findall(r"\{([^{}]*)\}", body)]


def tab_hash(v):
    x = np.asarray(v, dtype=np.int64).astype(np.int32).view(np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def test_the_tables_literals_are_numpys():
    rows = table("hashes")
    v = np.array([eval(r[0]) for r in rows], dtype=np.int64)            # ("-2147483647 - 1" is how C++ spells INT32_MIN)
    want = np.array([int(r[1][:-1], 16) for r in rows], dtype=np.uint32)
    assert {0, 1, -1, 2 ** 31 - 1, -2 ** 31} <= set(v.tolist()) and len(rows) >= 7
    with np.errstate(over="ignore"):
        assert np.array_equal(tab_hash(v), want)
    rows = table("homes")
    assert sorted(int(r[1]) for r in rows) == [13, 13, 14, 14]
    for h, tb, home in rows:
        assert ((int(h[:-1], 16) * 0x9E3779B1) & 0xFFFFFFFF) >> (32 - int(tb)) == int(home), (h, tb)


def test_the_rule_over_a_table(tmp_path):
    assert_passes(run_table(tmp_path, "claim_rule"))


@pytest.mark.parametrize("name", sorted(MUTATED))
def test_the_table_catches_a_mutated_rule(tmp_path, name):
    """With one format of the header changed the table says MISMATCH, so the test above is able to fail."""
    assert_catches(run_table(tmp_path, "claim_rule", ("claim_rule.h",) + MUTATED[name]))
