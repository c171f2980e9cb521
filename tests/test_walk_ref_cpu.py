"""The fast forms of the walk references against their definitions, and the draw-free expectations of tests/functional_ref.py against
the references, without a GPU: walk_ref.draws (runs by doubling) against one pow per index, pinsage_ref.topk (one flat sort) against
the row loop, and -- on the graphs tests/test_gpu_pinsage_sort.py walks -- the iterated successor against pinsage_ref.neighbors and
walk_ref.walk, with every index those read inside its array."""
import numpy as np
import pytest

from tests import functional_ref as fn
from tests import pinsage_ref
from tests import walk_ref
from tests import weighted_ref

M31 = 2 ** 31 - 1


# ---- draws ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 2 ** 31], ids=["step", "restart"])
@pytest.mark.parametrize("base", [0, 40, 1234567890])
def test_fast_draws_are_the_slow_ones(base, offset):
    for count in (1, 2, 3, 1000, 65537):
        walk_ref._DRAWS.pop((base, offset), None)                  # each length from nothing, then grown from the one before
        fast = walk_ref.draws(base, count, offset)
        assert fast.dtype == np.uint64 and np.array_equal(fast, walk_ref.draws_slow(base, count, offset)), (base, count, offset)
    grown = walk_ref.draws(base, 70000, offset)                    # ... and a cached run extended
    assert np.array_equal(grown, walk_ref.draws_slow(base, 70000, offset))


@pytest.mark.parametrize("offset", [0, 2 ** 31], ids=["step", "restart"])
def test_fast_draws_at_the_largest_legal_base(offset):
    """The run's last exponent is 2^31 - 1 (offset 0) or 2^32 - 1 (the restart draw of draw index 2^31 - 2)."""
    base = M31 - 65537
    fast, slow = walk_ref.draws(base, 65537, offset), walk_ref.draws_slow(base, 65537, offset)
    assert np.array_equal(fast, slow)
    assert int(slow[-1]) == walk_ref.minstd(M31 + offset) and int(fast.max()) < M31 and int(fast.min()) >= 1


def test_fast_draws_at_the_bases_the_gpu_tests_use():
    """A prefix and the tail of every (base, count) run that tests/test_gpu_random_walk.py and tests/test_gpu_pinsage.py ask for."""
    runs = [(0, 5000 * 100), (40, 257 * 17), (5, 5000 * 17), (9, 5000 * 16), (977, 257 * 1024), (40, 257 * 1024),
            (M31 - 65 * 17, 65 * 17), (M31 - 65 * 5 * 13, 65 * 5 * 13), (M31 - 8 * 5 * 4, 8 * 5 * 4), (M31 - 8 * 4, 8 * 4)]
    for base, count in runs:
        for offset in (0, 2 ** 31):
            fast = walk_ref.draws(base, count, offset)
            head = min(count, 3000)
            assert np.array_equal(fast[:head], walk_ref.draws_slow(base, head, offset)), (base, count, offset)
            assert np.array_equal(fast[-head:], walk_ref.draws_slow(base + count - head, head, offset)), (base, count, offset)


def test_draws_of_no_length_are_empty():
    assert walk_ref.draws(123, 0).shape == (0,) and walk_ref.draws(123, 0).dtype == np.uint64


# ---- topk -------------------------------------------------------------------------------------------------------------------------
def _rows(seed):
    """Seeded visit rows of width 40: random ones over few and over many ids, all -1, one value, every count tied."""
    rng = np.random.RandomState(seed)
    few = rng.randint(-1, 7, (60, 40))
    many = rng.randint(-1, 5000, (60, 40))
    empty = np.full((3, 40), -1)
    one = np.repeat(rng.randint(0, 5000, (4, 1)), 40, axis=1)
    one[1, ::3] = -1                                               # one value among sentinels
    tied = np.stack([rng.permutation(np.repeat(rng.choice(5000, 10, replace=False), 4)) for _ in range(6)])      # ten ids, four times each
    distinct = np.stack([rng.choice(5000, 40, replace=False) for _ in range(4)])                                  # forty ids, once each
    rows = np.concatenate([few, many, empty, one, tied, distinct]).astype(np.int32)
    return rows[rng.permutation(rows.shape[0])]


@pytest.mark.parametrize("seed", range(4))
def test_fast_topk_is_the_loop(seed):
    vis = _rows(seed)
    for k in (1, 5, 6, 7, 9, 10, 11, 39, 40, 41, 1024):            # below, at and above the distinct values of the few / tied / distinct rows
        fast, loop = pinsage_ref.topk(vis, k), pinsage_ref.topk_loop(vis, k)
        for a, b in zip(fast, loop):
            assert a.dtype == np.int32 and a.shape == (vis.shape[0], k) and np.array_equal(a, b), (seed, k)


def test_fast_topk_at_the_cap_and_without_rows():
    rng = np.random.RandomState(9)
    vis = rng.randint(-1, 300, (7, 1024)).astype(np.int32)
    vis[0], vis[1] = -1, 5
    vis[2] = np.arange(1024)[::-1]                                 # 1 024 distinct ids
    for k in (1, 299, 300, 301, 1024):
        fast, loop = pinsage_ref.topk(vis, k), pinsage_ref.topk_loop(vis, k)
        assert np.array_equal(fast[0], loop[0]) and np.array_equal(fast[1], loop[1]), k
    nb, ct = pinsage_ref.topk(np.zeros((0, 8), np.int32), 3)
    assert nb.shape == ct.shape == (0, 3)


# ---- the draw-free expectations of tests/functional_ref.py --------------------------------------------------------------------------
def test_id_orders_are_permutations():
    for name in fn.ORDERS:
        for n in (1, 2, 97, 193, 1029):
            assert np.array_equal(np.sort(fn.id_order(name, n)), np.arange(n)), (name, n)
    assert fn.id_order("bit-reversed", 8).tolist() == [0, 4, 2, 6, 1, 5, 3, 7]
    assert fn.id_order("organ-pipe", 7).tolist() == [0, 2, 4, 6, 5, 3, 1]


def _both_modes(succ, zero_weight=()):
    """(graph arrays, [(table or None, successor as that mode sees it)])"""
    indptr, col, w = fn.graph_of(succ, zero_weight)
    assert int(np.diff(indptr).max()) <= 1
    return indptr, col, [(None, succ), (weighted_ref.cdf(indptr, w), fn.without(succ, zero_weight))]


def _check_neighbors(indptr, col, table, succ, seeds, R, T, ks, p, base, ctx):
    reads = {}
    vis = pinsage_ref.visits(indptr, col, seeds, R, T, table=table, termination_prob=p, base=base, reads=reads)
    walk_ref.assert_reads_in_bounds(reads, indptr.size - 1, col.size)
    for k in ks:
        want, ref = fn.expected_neighbors(succ, seeds, R, T, k), pinsage_ref.topk(vis, k)
        assert np.array_equal(want[0], ref[0]) and np.array_equal(want[1], ref[1]), (ctx, k)


@pytest.mark.parametrize("order", fn.ORDERS)
def test_path_expectations_are_the_references(order):
    """termination_prob = 0 (a walk ends only where the path does); every T at the first and last order, a class edge at the others."""
    for T in fn.PATH_T if order in ("ascending", "shuffled") else (33, 256):
        succ, seeds = fn.path_case(order, 1, T)
        indptr, col, modes = _both_modes(succ)
        for table, s in modes:
            _check_neighbors(indptr, col, table, s, seeds, 1, T, fn.ks_for(T), 0.0, 7, (order, T, table is not None))
        steps = fn.iterate(succ, seeds, T)
        assert (steps[0] >= 0).all() and (steps[-2] < 0).any() and seeds[-1] == -1      # a full row, a short one, the bad seed


def test_run_expectations_are_the_references():
    for R, T in fn.RUN_SHAPES:
        succ, seeds = fn.path_case("descending", R, T)
        indptr, col, modes = _both_modes(succ)
        for table, s in modes:
            _check_neighbors(indptr, col, table, s, seeds, R, T, fn.ks_for(T), 0.0, 0, (R, T, table is not None))


def test_misc_expectations_are_the_references():
    succ = fn.misc_succ()
    indptr, col, modes = _both_modes(succ, fn.MISC_ZERO)
    for table, s in modes:
        for R, T, k in fn.MISC_SHAPES:
            _check_neighbors(indptr, col, table, s, fn.MISC_SEEDS, R, T, [k], 0.0, 3, (R, T, k, table is not None))
    nb, ct = fn.expected_neighbors(succ, np.array([1, 0, 10, 20], np.int32), 1, 1024, 4)
    assert nb[0].tolist() == [9, 1, 5, -1] and ct[0].tolist() == [342, 341, 341, 0]     # the larger count at the largest id
    assert nb[1].tolist() == [0, -1, -1, -1] and ct[1, 0] == 1024                       # one run of the whole segment
    assert nb[2].tolist() == [12, 13, 14, 11] and ct[2].tolist() == [341, 341, 341, 1]  # the tail counts once
    assert ct[3].tolist() == [1, 1, 1, 1]
    weighted = fn.expected_neighbors(fn.without(succ, fn.MISC_ZERO), np.array([20], np.int32), 1, 1024, 4)
    assert weighted[0][0].tolist() == [21, 22, -1, -1]                                  # the walk ends at the edge of weight 0


@pytest.mark.parametrize("order", fn.ORDERS)
def test_walk_expectations_are_the_references(order):
    ids = fn.id_order(order, 1100)
    succ = fn.path_succ(ids)
    seeds = np.concatenate([ids[np.arange(256) * 4], [-1]]).astype(np.int32)      # some walks run their length, some off the end
    indptr, col, modes = _both_modes(succ)
    for length in (16, 17, 1024) if order == "descending" else (17,):
        for table, s in modes:
            reads = {}
            ref = walk_ref.walk(indptr, col, seeds, length, table=table, base=11, reads=reads)
            walk_ref.assert_reads_in_bounds(reads, indptr.size - 1, col.size)
            want = fn.expected_walk(s, indptr, seeds, length)
            assert np.array_equal(want[0], ref[0]) and np.array_equal(want[1], ref[1]), (order, length)
    succ = fn.misc_succ()
    indptr, col, modes = _both_modes(succ, fn.MISC_ZERO)
    for table, s in modes:
        ref = walk_ref.walk(indptr, col, fn.MISC_SEEDS, 17, table=table, base=11)
        want = fn.expected_walk(s, indptr, fn.MISC_SEEDS, 17)
        assert np.array_equal(want[0], ref[0]) and np.array_equal(want[1], ref[1])
