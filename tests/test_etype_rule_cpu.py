"""The rule of per-edge-type sampling (legion_amd/csrc/etype_rule.h) is constexpr text that the kernels run on the device and
operators.hip asks in front of the launches.  tests/cpu/etype_rule_test.cpp pins the draw, the slot count, the refusals in their order and
the scratch size over a literal table; the same draws are checked against tests/etype_ref.py here, and the last test says what the
reference itself means: its draw is uniform and Floyd's picks are distinct, uniform subsets.  Compiled on the host, no GPU, no HIP."""
import itertools

import numpy as np
import pytest

from tests import etype_ref as ref
from tests.rule_table import assert_passes, run_table

# the draws of the C++ table, (salt, row, t, k, R, draw): a negative salt, R = 1, R = 2^31 - 1 and row = 2^31 - 1 among them
DRAWS = [(0, 0, 0, 0, 5, 3), (1, 7, 3, 2, 100, 58), (-1, 12345, 63, 63, 4097, 2252), (-2 ** 63, 5, 1, 0, 2, 1), (99, 2 ** 31 - 1, 0, 1, 1000, 709),
         (3, 9, 2, 4, 1, 0), (3, 9, 2, 4, 2 ** 31 - 1, 1331445703), (12345, 70000, 17, 33, 70001, 18729), (2 ** 63 - 1, 1, 63, 0, 2 ** 32 - 1, 665727107)]


@pytest.mark.parametrize("salt, row, t, k, R, want", DRAWS)
def test_the_tables_draws_are_the_references(salt, row, t, k, R, want):
    assert int(ref.draw(salt, row, t, k, R)) == want


def test_the_rule_over_a_table(tmp_path):
    assert_passes(run_table(tmp_path, "etype_rule"))


@pytest.mark.parametrize("salt", [0, 1, -1])
def test_the_reference_draws_uniformly_and_floyd_picks_uniform_subsets(salt):
    """Over 200 000 row ids every frequency lies within five binomial standard deviations of its probability: a position of a segment
    of 5 drawn with replacement (1 / 5); without replacement at D = 7, f = 3 a position's inclusion (3 / 7) and each of the 35 subsets
    (1 / 35).  The picks of a pair are distinct."""
    n, D, f = 200_000, 7, 3
    rows = np.arange(n)
    sd = lambda p: np.sqrt(p * (1 - p) / n)
    freq = np.bincount(ref.draw(salt, rows, 2, 1, 5), minlength=5) / n
    assert np.abs(freq - 1 / 5).max() < 5 * sd(1 / 5), freq
    picks = np.zeros((n, f), dtype=np.int64)                           # Floyd over all rows at once: the reference's loop, a column a slot
    for k in range(f):
        c = ref.draw(salt, rows, 4, k, D - f + k + 1)
        picks[:, k] = np.where((picks[:, :k] == c[:, None]).any(axis=1), D - f + k, c)
    assert all(picks[r].tolist() == ref.pair_picks(salt, r, 4, D, f, False) for r in (0, 1, 77, n - 1))
    ordered = np.sort(picks, axis=1)
    assert np.all(ordered[:, 1:] > ordered[:, :-1]) and picks.min() >= 0 and picks.max() < D, "distinct positions of the segment"
    member = np.stack([(picks == x).any(axis=1) for x in range(D)], axis=1).mean(axis=0)
    assert np.abs(member - f / D).max() < 5 * sd(f / D), member
    freq = np.array([(ordered == s).all(axis=1).mean() for s in itertools.combinations(range(D), f)])
    assert freq.size == 35 and np.abs(freq - 1 / 35).max() < 5 * sd(1 / 35), freq
