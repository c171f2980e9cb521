"""The rule of seed-edge exclusion (legion_amd/csrc/exclude_rule.h: the slots, the shift, the home slot and the bytes of the set of edge
ids, which calls are refused and in which order, the filter's scratch) is constexpr text that kernels_exclude.hip runs on the device and
operators.hip asks in front of the launches.  tests/cpu/exclude_rule_test.cpp pins it over a literal table; here the table runs, its
home slots are checked against tests/exclude_ref.py and Python's integers so that neither can drift, and it is shown to catch a dropped
rule and a moved boundary.  Compiled on the host, no GPU, no HIP."""
import re

import numpy as np
import pytest

from tests import exclude_ref as ref
from tests.rule_table import ROOT, assert_catches, assert_passes, run_table

# a rule of the header -> what it is replaced with
DROPPED = {
    "a key of 64 bits in the hash": ("return ((uint64_t)e * EDGE_SET_HASH) >> shift; }", "return ((uint64_t)(uint32_t)e * EDGE_SET_HASH) >> shift; }", 1),
    "a hash of 64 bits": ("return ((uint64_t)e * EDGE_SET_HASH) >> shift; }",
                          "return (uint64_t)(((uint32_t)e * 2654435769u) >> (shift - 32)); }", 1),
    "at least 2 k slots": ("    while (s < 2 * (int64_t)k) s <<= 1;\n", "    while (s < (int64_t)k) s <<= 1;\n", 1),
    "the limit of the set moved": ("    if (k < 0 || k > LEGION_EDGE_SET_MAX_IDS) return -1;\n", "    if (k < 0 || k >= LEGION_EDGE_SET_MAX_IDS) return -1;\n", 1),
    "sorted rows for via 0": ("    if (via == 0 && rows_sorted != 1) return ExcludeRefusal::Unsorted;\n", "", 1),
    "a built reverse for via 1": ("    if (via == 1 && !have_reverse) return ExcludeRefusal::NoReverse;\n", "", 1),
    "n at most 2^31 - 1": ("    if (n < 0 || n > (int64_t)0x7FFFFFFF) return ExcludeRefusal::Count;\n", "    if (n < 0) return ExcludeRefusal::Count;\n", 1),
    "the overlap check": ("exclude_ranges_overlap(out[o], width[o] * (uint64_t)cap, in[i], width[i] * (uint64_t)m)) return ExcludeRefusal::Alias;",
                          "false) return ExcludeRefusal::Alias;", 1),
    "an empty range overlaps nothing": ("    return a_bytes != 0 && b_bytes != 0 && a < b + b_bytes && b < a + a_bytes;\n",
                                        "    return a < b + b_bytes && b < a + a_bytes;\n", 1),
    "eight bytes an edge id in the overlap": ("    const uint64_t width[3] = {4, 4, 8};\n", "    const uint64_t width[3] = {4, 4, 4};\n", 1),
    "the limit of the filter moved": ("    if (m < 0 || m > LEGION_EDGE_FILTER_MAX_EDGES) return -1;\n", "    if (m < 0 || m >= LEGION_EDGE_FILTER_MAX_EDGES) return -1;\n", 1),
}


def table(name):
    """The rows of one literal table of the C++ file, as lists of strings."""
    text = open(f"{ROOT}/tests/cpu/exclude_rule_test.cpp").read()
    body = text.split(f" {name}[] = {{", 1)[1].split("\n};", 1)[0]
    body = re.sub(r"//[^\n]*", "", body)
    return [[x.strip() for x in row.split(",")] for row in re.findall(r"\{([^{}]*)\}", body)]


def test_the_tables_values_are_the_references():
    homes = [(int(e), int(slots), int(home)) for e, slots, home in table("homes")]
    assert len(homes) >= 15 and sum(e >= 2 ** 32 for e, _, _ in homes) >= 6, "ids past 2^32"
    for e, slots, home in homes:
        bits = slots.bit_length() - 1
        assert home == ((e * ref.HASH) % 2 ** 64) >> (64 - bits), (e, slots)
        k = slots // 2
        assert ref.set_slots(k) == slots and int(ref.home_slots(np.array([e]), k)[0]) == home, (e, slots)
    cut = [(e, slots, home) for e, slots, home in homes if int(ref.home_slots_hash32(np.array([e]), slots // 2)[0]) != home]
    assert len(cut) >= 10, "a hash cut to 32 bits gives other homes"
    pairs = {(e % 2 ** 32, slots): home for e, slots, home in homes if e < 2 ** 32}
    assert sum(1 for e, slots, home in homes if e >= 2 ** 32 and pairs.get((e % 2 ** 32, slots), home) != home) >= 2, \
        "ids with equal low halves and different homes: a key cut to 32 bits is caught"
    for k, slots, shift, nbytes in table("sizes"):
        k, nbytes = int(k), int(nbytes)
        assert nbytes == ref.set_bytes(k), k
        if nbytes >= 0:
            assert int(slots) == ref.set_slots(k) and int(shift) == 64 - (int(slots).bit_length() - 1)
    assert {0, 128, 129, 2 ** 21, 2 ** 21 + 1, -1} <= {int(r[0]) for r in table("sizes")}


def test_the_rule_over_a_table(tmp_path):
    assert_passes(run_table(tmp_path, "exclude_rule"))


@pytest.mark.parametrize("name", sorted(DROPPED))
def test_the_table_catches_a_dropped_rule(tmp_path, name):
    """Without one rule of the header, or with a boundary moved by one, the table says MISMATCH, so the test above is able to fail."""
    assert_catches(run_table(tmp_path, "exclude_rule", ("exclude_rule.h",) + DROPPED[name]))
