"""The link-prediction seed ops without a GPU: the entry points in the header, the ctypes table and the library, the arguments the Python
methods refuse before they touch a device, and the numpy restatement's (tests/link_ref.py) own properties on the symmetric graph the GPU
tests use: it is the brute-force loops' result, it reads inside its arrays, its counters are the figures the GPU tests rely on, and its
negatives are uniform over the non-neighbours."""
import os
import re
import subprocess

import numpy as np
import pytest

from legion_amd import engine, lib
from tests import link_ref as ref
from tests import node2vec_ref, walk_ref
# the inputs of the GPU files come from their own builders: what is proven here is what they launch
from tests import test_gpu_link_find_edges as gpu_find
from tests import test_gpu_link_fuzz as gpu_fuzz
from tests import test_gpu_link_negative as gpu_negative
from tests import test_gpu_link_stride as gpu_stride
from tests import test_gpu_link_table as gpu_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "legion_hip.h")
LIB = os.path.join(ROOT, "legion_amd", "liblegion_hip.so")
NAMES = ["legion_find_edges", "legion_negative_sample", "legion_unique_ids", "legion_unique_ids_scratch_bytes"]


@pytest.fixture(scope="module")
def world():
    indptr, col, _ = node2vec_ref.sym_graph()
    return {"indptr": indptr, "col": col}


# ---- the entry points -----------------------------------------------------------------------------------------------------------
def test_symbols_in_header_ctypes_table_and_library():
    text = open(HEADER).read()
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NAMES:
        assert re.search(r"\bint(32|64)_t\s+" + name + r"\s*\(", text), name
    assert re.search(r"#define\s+LEGION_NEGATIVE_MAX_TRIES\s+256\b", text) and re.search(r"#define\s+LEGION_UNIQUE_MAX_IDS\s+1048576\b", text)
    assert set(NAMES) <= exported
    c_p, c_i32, c_i64 = lib.c_p, lib.c_i32, lib.c_i64
    assert lib.SIGNATURES["legion_find_edges"] == (c_i32, [c_p, c_p, c_p, c_i32, c_p, c_p])
    assert lib.SIGNATURES["legion_negative_sample"] == (c_i32, [c_p, c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_i64, c_p])
    assert lib.SIGNATURES["legion_unique_ids"] == (c_i32, [c_p, c_p, c_i32, c_p, c_p, c_p, c_p, c_i64])
    assert lib.SIGNATURES["legion_unique_ids_scratch_bytes"] == (c_i64, [c_i32])


def test_the_python_side_has_the_methods():
    for name in ("find_edges", "negative_sample", "edge_prediction_seeds"):
        assert callable(getattr(engine.GraphStorage, name, None)), name
    assert callable(getattr(engine, "unique_ids", None))
    assert engine.GraphStorage.NEGATIVE_MAX_TRIES == ref.MAX_TRIES and engine.UNIQUE_MAX_IDS == ref.MAX_IDS


def test_null_pointers_are_refused_before_anything_else():
    L = lib.load()
    assert L.legion_find_edges(None, None, None, 1, None, None) == -1
    assert L.legion_negative_sample(None, None, None, 1, 1, 0, 1, 0, None) == -1
    assert L.legion_unique_ids(None, None, 1, None, None, None, None, 1 << 30) == -1


def test_the_scratch_size_is_the_references():
    L = lib.load()
    for m in (-1, 0, 1, 63, 64, 65, 128, 129, 256, 257, 1023, 1024, 1025, 3073, 70001, 2 ** 20, 2 ** 20 + 1):
        assert L.legion_unique_ids_scratch_bytes(m) == ref.scratch_bytes(m), m
    assert ref.table_slots(2 ** 20) == 2 ** 21 and all(ref.table_slots(m) >= 2 * m for m in (1, 128, 129, 70001))


def test_the_header_states_the_coincidence_and_what_is_not_offered():
    text = open(HEADER).read()
    assert "coincides with try 0 of the slot t * 2^23" in text and "255 * 2^23 + 2^31 < 2^32" in text
    assert "degree-biased negatives" in text and "a consumer masks by agg_edge_ids" in text
    assert 255 * 2 ** 23 + 2 ** 31 < 2 ** 32


# ---- ValueErrors, without a device ----------------------------------------------------------------------------------------------
def _bare_graph():
    g = engine.GraphStorage.__new__(engine.GraphStorage)      # (no handle: the checks come before the library call)
    g.node_num, g.edge_num = 10, 20
    return g


NEGATIVE_ERRORS = [
    (dict(k=0), "k must"), (dict(k=-2), "k must"), (dict(k=2.0), "k must"), (dict(k=True), "k must"), (dict(k=None), "k must"),
    (dict(max_tries=0), "max_tries"), (dict(max_tries=257), "max_tries"), (dict(max_tries=-1), "max_tries"), (dict(max_tries=2.0), "max_tries"),
    (dict(max_tries=True), "max_tries"), (dict(max_tries=None), "max_tries"),
    (dict(base=-1), "base"), (dict(base=1.5), "base"), (dict(base=2 ** 31 - 1 - 3 * 5 + 1), "draw index"), (dict(k=2 ** 30), "draw index"),
    (dict(exclude_self=1), "exclude_self"), (dict(exclude_self=None), "exclude_self"), (dict(exclude_edges=0), "exclude_edges"),
    (dict(exclude_edges="yes"), "exclude_edges"),
]


@pytest.mark.parametrize("kw, match", NEGATIVE_ERRORS)
def test_negative_sample_refuses_before_touching_a_device(kw, match):
    args = dict(k=5)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        _bare_graph().negative_sample(np.array([1, 2, 3], dtype=np.int32), **args)


@pytest.mark.parametrize("kw, match", NEGATIVE_ERRORS + [(dict(k=2 ** 20), "at most")])
def test_edge_prediction_seeds_refuses_before_touching_a_device(kw, match):
    args = dict(k=5)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        _bare_graph().edge_prediction_seeds(np.array([1, 2, 3], dtype=np.int64), **args)


def test_wrong_dtypes_and_shapes_are_refused():
    import torch
    g = _bare_graph()
    with pytest.raises(ValueError, match="int64"):
        g.find_edges(torch.tensor([1, 2], dtype=torch.int32))
    with pytest.raises(ValueError, match="one-dimensional"):
        g.find_edges(np.zeros((2, 2), dtype=np.int64))
    with pytest.raises(ValueError, match="int32"):
        g.negative_sample(torch.tensor([1, 2], dtype=torch.int64), 5)
    with pytest.raises(ValueError, match="one-dimensional"):
        g.negative_sample(np.zeros((2, 2), dtype=np.int32), 5)
    with pytest.raises(ValueError, match="int64"):
        g.edge_prediction_seeds(torch.tensor([1, 2], dtype=torch.int32), 5)
    with pytest.raises(ValueError, match="one-dimensional"):
        g.edge_prediction_seeds(np.zeros((2, 2), dtype=np.int64), 5)
    with pytest.raises(ValueError, match="int32"):
        engine.unique_ids(torch.tensor([1, 2], dtype=torch.int64))
    with pytest.raises(ValueError, match="one-dimensional"):
        engine.unique_ids(np.zeros((2, 2), dtype=np.int32))
    with pytest.raises(ValueError, match="at most"):
        engine.unique_ids(np.zeros(2 ** 20 + 1, dtype=np.int32))


def test_the_python_check_is_the_rule():
    ok = engine.GraphStorage._check_negative
    ok(3, 5, True, True, 256, 2 ** 31 - 1 - 15)
    ok(0, 1, False, False, 1, 2 ** 31 - 1)
    for n in (0, 3):
        for k in (-1, 0, 1, 5):
            for tries in (0, 1, 256, 257):
                for base in (-1, 0, 2 ** 31 - 1 - 15, 2 ** 31 - 15):
                    want = ref.negative_refused(n, k, 3, tries, base, 1)
                    try:
                        ok(n, k, True, True, tries, base)
                        got = False
                    except ValueError:
                        got = True
                    assert got == want, (n, k, tries, base)


def test_the_predicates():
    assert not ref.negative_refused(3, 5, 0, 256, 0, -1) and not ref.negative_refused(3, 5, 1, 256, 0, 0)
    assert ref.negative_refused(3, 5, 2, 256, 0, -1) and ref.negative_refused(3, 5, 3, 256, 0, 0) and not ref.negative_refused(3, 5, 3, 256, 0, 1)
    assert ref.negative_refused(3, 5, 4, 256, 0, 1) and ref.negative_refused(3, 5, -1, 256, 0, 1)
    assert ref.unique_refused(5, ref.scratch_bytes(5) - 1) and not ref.unique_refused(5, ref.scratch_bytes(5))
    assert ref.unique_refused(5, 1 << 20, ids=1000, unique=1016) and not ref.unique_refused(5, 1 << 20, ids=1000, unique=1020)
    assert ref.unique_refused(5, 1 << 20, ids=1000, count=1016) and not ref.unique_refused(5, 1 << 20, ids=1000, count=996)
    assert ref.find_edges_refused(-1) and not ref.find_edges_refused(0)


# ---- the reference against brute force ------------------------------------------------------------------------------------------
def test_find_edges_is_the_loop(world):
    indptr, col = world["indptr"], world["col"]
    E = col.size
    eids = ref.eids_for(indptr, col, 400)
    reads = {}
    row, c = ref.find_edges(indptr, col, eids, reads=reads)
    walk_ref.assert_reads_in_bounds(reads, node2vec_ref.NODE_NUM, E)
    owner = np.repeat(np.arange(node2vec_ref.NODE_NUM), np.diff(indptr))
    for i, e in enumerate(eids.tolist()):
        if e < 0 or e >= E or col[e] < 0:
            assert row[i] == -1 and c[i] == -1, (i, e)
        else:
            assert row[i] == owner[e] and c[i] == col[e] and indptr[row[i]] <= e < indptr[row[i] + 1], (i, e)
    live = row >= 0
    assert (~live).sum() >= 33 and live.sum() >= 300
    assert 42 in row and 8 in row and 40 not in row and 41 not in row      # the rows after the empty rows, never the empty rows


def test_the_edge_ids_contain_what_the_gpu_test_names(world):
    indptr, col = world["indptr"], world["col"]
    E = col.size
    e = set(ref.eids_for(indptr, col, 63).tolist())
    assert {-1, E, E + 5, E - 1} <= e and set(np.nonzero(col < 0)[0].tolist()) <= e and (col < 0).sum() == 30
    for h in node2vec_ref.HUBS:
        assert int(indptr[h]) in e and int(indptr[h + 1]) - 1 in e
    assert indptr[40] == indptr[41] == indptr[42] and int(indptr[42]) in e and int(indptr[8]) in e
    assert ref.eids_for(indptr, col, 1).tolist() == [E - 1]


@pytest.mark.parametrize("exclude", [0, 1, 2, 3])
@pytest.mark.parametrize("tries", [1, 3, 256])
def test_negative_sample_is_the_loop(world, exclude, tries):
    indptr, col = world["indptr"], world["col"]
    N = node2vec_ref.NODE_NUM
    rows = np.concatenate([node2vec_ref.seeds_for(5000)[:40], [-1, N, 6, 6]]).astype(np.int32)
    k, base = 5, 777
    reads = {}
    got = ref.negative_sample(indptr, col, rows, k, exclude, tries, base, reads=reads)
    walk_ref.assert_reads_in_bounds(reads, N, col.size)
    if not exclude & 2:
        assert not reads
    for i, r in enumerate(rows.tolist()):
        for j in range(k):
            want = -1
            if 0 <= r < N:
                nn = base + i * k + j
                row = set(col[indptr[r]:indptr[r + 1]].tolist())
                for t in range(tries):
                    x = walk_ref.minstd(((nn + 1) & 0xFFFFFFFF) + t * 2 ** 23)
                    u = int((x - 1) / 2147483646.0 * N)
                    if (exclude & 1 and u == r) or (exclude & 2 and u in row):
                        continue
                    want = u
                    break
            assert got[i, j] == want, (i, j, r)


def test_try_stepping_is_the_power(world):
    x = walk_ref.minstd(12345)
    assert x * walk_ref.minstd(2 ** 23) % walk_ref.M31 == walk_ref.minstd(12345 + 2 ** 23)


def test_the_figures_the_gpu_tests_rely_on(world):
    """seeds_for(5000)[:600], k = 5, both exclusions: 408 of 3 000 slots reject at least once, 272 are exhausted at max_tries = 2 and none
    at 256; a fifth of the rows are the 4 097-entry hub, which rejects 68 % of its candidates."""
    indptr, col = world["indptr"], world["col"]
    rows = node2vec_ref.seeds_for(5000)[:600]
    two, full = ref.new_stats(node2vec_ref.NODE_NUM), ref.new_stats(node2vec_ref.NODE_NUM)
    a = ref.negative_sample(indptr, col, rows, 5, 3, 2, 0, stats=two)
    b = ref.negative_sample(indptr, col, rows, 5, 3, 256, 0, stats=full)
    assert two["rejected_slots"] == full["rejected_slots"] == 408 and two["exhausted"] == 272 and full["exhausted"] == 0
    assert int((a < 0).sum()) == 272 and int((b < 0).sum()) == 0
    assert 0.19 < (rows == 6).mean() < 0.21
    assert 0.66 < full["hits_of_row"][6] / full["searches_of_row"][6] < 0.70


def test_small_graphs(world):
    ip, c = ref.complete_graph(8)
    rows = np.arange(8, dtype=np.int32).repeat(4)
    for tries in (1, 3, 256):
        assert np.all(ref.negative_sample(ip, c, rows, 5, 3, tries) == -1)
    assert np.array_equal(ref.negative_sample(ip, c, rows, 5, 2, 256), np.repeat(rows, 5).reshape(-1, 5))
    ip, c = ref.ring_graph(8)
    st = ref.new_stats(8)
    out = ref.negative_sample(ip, c, rows, 5, 1, 256, stats=st)
    assert st["self"] >= 10 and np.all(out != rows[:, None]) and np.all(out >= 0)


def test_unique_ids_is_the_loop():
    rng = np.random.RandomState(3)
    for ids in (rng.randint(-3, 40, 500), np.array([], dtype=np.int64), np.full(9, -1), np.full(9, 4), np.arange(20)[::-1]):
        ids = ids.astype(np.int32)
        unique, local, count = ref.unique_ids(ids)
        seen = {}
        for i, v in enumerate(ids.tolist()):
            if v < 0:
                assert local[i] == -1
                continue
            if v not in seen:
                seen[v] = len(seen)
            assert local[i] == seen[v], i
        assert count == len(seen) and unique[:count].tolist() == list(seen) and np.all(unique[count:] == -1)


def test_the_composite_gives_back_the_endpoints(world):
    indptr, col = world["indptr"], world["col"]
    eids = ref.eids_for(indptr, col, 257)
    out = ref.edge_prediction_seeds(indptr, col, eids, 5, base=9)
    seeds = np.concatenate([out["seeds"], [-1]])                   # (index -1: a -1)
    assert np.array_equal(seeds[out["pos_row"]], out["row"]) and np.array_equal(seeds[out["pos_col"]], out["col"])
    assert np.array_equal(seeds[out["neg_col"]], out["neg"])
    U = out["num_seeds"]
    assert len(set(out["seeds"][:U].tolist())) == U and out["seeds"][:U].min() >= 0 and (out["row"] < 0).sum() >= 33


# ---- frequencies ----------------------------------------------------------------------------------------------------------------
def test_negatives_are_uniform_over_the_non_neighbours(world):
    """360 000 negatives of vertex 1, the 64-entry row: every vertex that is neither 1 nor in its row is drawn about 60 times.  Every cell
    lies within five binomial standard deviations of uniform (the bound of test_node2vec_cpu.py's frequencies); no excluded vertex is
    drawn at all.  The sequence is fixed: this passes or it does not."""
    indptr, col = world["indptr"], world["col"]
    N = node2vec_ref.NODE_NUM
    assert node2vec_ref.HUBS[1] == 64
    n = 360000
    out = ref.negative_sample(indptr, col, np.full(n // 5, 1, dtype=np.int32), 5, 3, 256, 0).reshape(-1)
    assert np.all(out >= 0)
    banned = np.zeros(N, dtype=bool)
    banned[col[indptr[1]:indptr[2]][col[indptr[1]:indptr[2]] >= 0]] = True
    banned[1] = True
    counts = np.bincount(out, minlength=N)
    assert np.all(counts[banned] == 0)
    cells = int((~banned).sum())
    prob = 1.0 / cells
    sd = np.sqrt(n * prob * (1 - prob))
    worst = float(np.abs(counts[~banned] - n * prob).max() / sd)
    print(f"{cells} cells, expected {n * prob:.1f} each, worst {worst:.2f} sd")
    assert n * prob >= 50 and worst <= 5.0, worst


# ---- what the GPU tests of the second pass assert before they launch, and four wrong kernels that they catch ----------------------
def unique_without_wrap(ids, order):
    """Wrong kernel 1: a probe that stops at the table's last slot.  An id that finds no place there has no slot: local = -1, and it is
    no seed."""
    ids = np.asarray(ids, dtype=np.int32)
    slot = ref.probe_table(ids, ids.size, order, wrap=False)[0]
    return ref.unique_ids(np.where(slot < 0, -1, ids))


def unique_by_first_claimer(ids, order):
    """Wrong kernel 2: the slot remembers the index of the lane that claimed it, not the minimum over its lanes.  With `order` the
    arrival order, the claimer of an id is its first index in that order; the later launches are the library's: index i is a first
    touch if it is its id's remembered index, first touches are ranked in index order, local[i] is the rank of the remembered index."""
    ids = np.asarray(ids, dtype=np.int32)
    m = ids.size
    claimed = {}
    for i in np.asarray(order).tolist():
        if ids[i] >= 0:
            claimed.setdefault(int(ids[i]), i)
    flag = np.zeros(m, dtype=bool)
    flag[list(claimed.values())] = True
    rank = np.cumsum(flag) - 1
    unique, local = np.full(m, -1, dtype=np.int32), np.full(m, -1, dtype=np.int32)
    unique[:int(flag.sum())] = ids[flag]
    live = np.nonzero(ids >= 0)[0]
    local[live] = [rank[claimed[int(v)]] for v in ids[live]]
    return unique, local, int(flag.sum())


def _differs(a, b):
    return any(not np.array_equal(x, y) for x, y in zip(a[:2], b[:2])) or a[2] != b[2]


def test_ids_with_home_inverts_the_hash():
    assert ref.HASH * ref.HASH_INV % 2 ** 32 == 1
    for m, homes in ((2, [0, 255]), (1000, [2047]), (70001, range(262144 - 64, 262144)), (2 ** 20, [0, 2 ** 21 - 1])):
        ids = ref.ids_with_home(m, homes, 50)
        assert ids.dtype == np.int32 and ids.min() >= 0 and np.unique(ids).size == ids.size == 50 * len(homes)
        assert np.array_equal(ref.home_slots(ids, m), np.repeat(np.asarray(homes), 50))
    with pytest.raises(AssertionError):
        ref.ids_with_home(2 ** 20, [5], 2000)                      # a home of 2^21 slots has 2 048 values of y, half of them ids


def test_probe_table_is_linear_probing():
    """Against the loop over slots on a table small enough to fill by hand."""
    ids = np.array([5, -1, 9, 5, 14, 9, 3, 22], dtype=np.int32)
    homes = ref.home_slots(np.maximum(ids, 0), ids.size)
    for order in (np.arange(8), np.arange(8)[::-1]):
        table, want, longest, wraps = {}, np.full(8, -1), 0, 0
        for i in order:
            if ids[i] < 0:
                continue
            s, n = int(homes[i]), 1
            while s in table and table[s] != ids[i]:
                s, n = (s + 1) % 256, n + 1
            wraps += int(s not in table and s < homes[i])
            table[s] = ids[i]
            want[i], longest = s, max(longest, n)
        got = ref.probe_table(ids, 8, order)
        assert np.array_equal(got[0], want) and got[1:] == (longest, wraps)
    one = ref.ids_with_home(8, [255], 8)
    slot, longest, wraps = ref.probe_table(one, 8, np.arange(8))
    assert slot.tolist() == [255, 0, 1, 2, 3, 4, 5, 6] and (longest, wraps) == (8, 7)
    slot, longest, wraps = ref.probe_table(one, 8, np.arange(8), wrap=False)
    assert slot.tolist() == [255] + [-1] * 7 and wraps == 0


@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("m", gpu_table.ONE_HOME)
def test_one_home_inputs_wrap_and_probe_far(m, interleaved):
    ids = gpu_table.one_home(m, interleaved)
    gpu_table.one_home_conditions(ids, m)
    want = ref.unique_ids(ids)
    for order in gpu_table.orders(ids.size):
        wrong = unique_without_wrap(ids, order)
        assert wrong[2] == 1 and want[2] == m and _differs(wrong, want)
        assert int((wrong[1] == -1).sum()) - int((want[1] == -1).sum()) == (ids >= 0).sum() * (m - 1) // m      # every id but one: no slot
    if interleaved:                                                # descending arrival: the claimer is an id's LAST appearance
        wrong = unique_by_first_claimer(ids, np.arange(ids.size)[::-1])
        assert wrong[2] == want[2] and _differs(wrong, want)
        assert int((wrong[1] != want[1]).sum()) >= m and not np.array_equal(wrong[0], want[0])
        assert not _differs(unique_by_first_claimer(ids, np.arange(ids.size)), want)      # in index order the claimer IS the minimum


def test_cluster_inputs_wrap():
    for m in gpu_table.CLUSTERS:
        ids, at = gpu_table.cluster(m)
        least = gpu_table.cluster_conditions(ids, at, m)
        want = ref.unique_ids(ids)
        if m > 70001:                                              # (the pigeonhole alone: the model takes seconds at 2^20)
            continue
        for order in gpu_table.orders(m):
            _, longest, wraps = ref.probe_table(ids, m, order)
            print(f"m {m}: {wraps} ids wrap, longest run {longest}")
            assert wraps >= least and longest > gpu_table.CLUSTER_PER
        wrong = unique_without_wrap(ids, np.arange(m))
        assert want[2] - wrong[2] >= least and int((wrong[1] == -1).sum()) >= least


def test_the_hot_key():
    ids = gpu_table.hot_key()
    unique, local, count = ref.unique_ids(ids)
    assert ids.size == 2 ** 20 and count == 2 and np.all(local[:-1] == 0) and local[-1] == 1 and np.all(unique[2:] == -1)


def test_find_edges_stride_case_and_a_stale_second_trip():
    eids, want, named = gpu_stride.find_case()
    assert eids.size == 2048 * 1024 + 1024 + 1 and set(named) >= {"-1", "E", "E + 5", "dead entry", "after two empty rows"}
    for w in want:                                                 # wrong kernel 3
        stale = gpu_stride.stale_second_trip(w, gpu_stride.FIND_STRIDE)
        assert np.array_equal(stale[:gpu_stride.FIND_STRIDE], w[:gpu_stride.FIND_STRIDE]) and (stale != w).sum() >= 900
    indptr, col = gpu_stride.graph()                               # wrong kernel 4, on the id placed for it
    i = named["after two empty rows"][0]
    assert ref.find_edges_lower_bound(indptr, col, eids[i:i + 1])[0][0] == 40 and want[0][i] == 42


@pytest.mark.parametrize("shape", gpu_stride.NEG_SHAPES, ids=lambda s: f"{s['n']}x{s['k']}")
def test_negative_stride_cases_and_a_stale_second_trip(shape):
    rows, want, stats = gpu_stride.negative_case(shape)
    print({k: v for k, v in stats.items() if not hasattr(v, "shape")}, "second-trip -1s", int((want.reshape(-1)[gpu_stride.NEG_STRIDE:] < 0).sum()))
    stale = gpu_stride.stale_second_trip(want, gpu_stride.NEG_STRIDE)
    late = want.size - gpu_stride.NEG_STRIDE
    assert (stale != want).sum() * 2 >= late, "half of the second trip's slots at least"
    if shape["exclude"] == 3:
        assert shape["tries"] == 3 and (want.reshape(-1)[gpu_stride.NEG_STRIDE:] < 0).sum() == 128 + stats["exhausted"]


@pytest.mark.parametrize("kind", gpu_stride.UNIQUE_KINDS)
@pytest.mark.parametrize("m", gpu_stride.UNIQUE_COUNTS)
def test_unique_stride_cases_and_a_stale_second_trip(m, kind):
    ids = gpu_stride.stride_ids(kind, m)
    want, firsts, repeats = gpu_stride.unique_conditions(kind, ids)
    if (kind, m) == ("mix", 524545):
        assert (firsts, repeats, int((ids[gpu_stride.UNIQUE_STRIDE:] == -1).sum())) == (51, 155, 51)
    if m > gpu_stride.UNIQUE_STRIDE:
        stale = gpu_stride.stale_second_trip(want[1], gpu_stride.UNIQUE_STRIDE)
        assert not np.array_equal(stale, want[1])
        if kind == "mix":                                          # the model of the claimer on an input with repeats all over
            assert _differs(unique_by_first_claimer(ids, np.arange(m)[::-1]), want)
    else:                                                          # the scan: per = 1 at 256 tiles, 2 from 257 on; 2 050 tiles: runs of 9, the last of 7
        per = lambda tiles: (tiles + 255) // 256
        assert (per((m + 255) // 256), (m + 255) // 256) in ((1, 256), (2, 257))
        assert per(2050) == 9 and 2050 - 9 * (2050 // 9) == 7 and (524545 + 255) // 256 == 2050


@pytest.mark.parametrize("name", sorted(ref.small_graphs()))
def test_small_graphs_against_the_loop_and_a_lower_bound(name):
    indptr, col, eids, want = gpu_find.small_case(name)
    assert eids[0] == -2 and eids[-1] == col.size + 2
    for i, e in enumerate(eids.tolist()):                          # the definition: the row whose range holds e
        rows = [v for v in range(indptr.size - 1) if indptr[v] <= e < indptr[v + 1]] if 0 <= e < col.size and col[e] >= 0 else []
        assert (want[0][i], want[1][i]) == ((rows[0], col[e]) if rows else (-1, -1)), (name, e)


def test_the_small_graphs_are_what_they_are_called():
    g = ref.small_graphs()
    assert {ip.size - 1 for ip, _ in g.values()} >= {1, 2, 3, 254, 255, 256, 257, 64}
    assert g["loop"][1].tolist() == [0] and np.diff(g["ends-empty"][0])[:3].tolist() == [0, 0, 0] == np.diff(g["ends-empty"][0])[-3:].tolist()
    deg = np.diff(g["one-row"][0])
    assert deg[17] == deg.sum() == 40 and deg.size == 64
    for n in (254, 255, 256, 257):
        d = np.diff(g[f"degrees-{n}"][0])
        assert set(d.tolist()) == {0, 1, 2, 3} and (g[f"degrees-{n}"][1] < 0).sum() == 3
    wrong = sum(int((ref.find_edges_lower_bound(ip, c, np.arange(c.size))[0] != ref.find_edges(ip, c, np.arange(c.size))[0]).sum()) for ip, c in g.values())
    assert wrong >= 100                                            # wrong kernel 4 over all of them


def test_the_find_edges_counts_split_a_lanes_four_ids():
    """A lane's ids j = 0 .. 3 sit at lane + 256 j: id j is dead for every lane at n <= 256 j, for some at 256 j < n < 256 (j + 1)."""
    for j in (1, 2, 3):
        assert {256 * j, 256 * j + 1} <= set(gpu_find.COUNTS)
    assert {1023, 1024, 1025, 2049, 5000} <= set(gpu_find.COUNTS)


def test_one_vertex_and_the_big_draw():
    ip, c = np.array([0, 1], dtype=np.int64), np.array([0], dtype=np.int32)
    rows = np.zeros(50, dtype=np.int32)
    assert np.all(ref.negative_sample(ip, c, rows, 5, 1, 3) == -1) and np.all(ref.negative_sample(ip, c, rows, 5, 0, 3) == 0)
    indptr, col, rows, want = gpu_negative.big_case(gpu_negative.BIG[0])      # (its conditions are asserted inside)
    assert indptr.size == 2 ** 24 + 4 and col.size == 1000 and np.all(np.diff(col) > 0) and rows.size == 5000 and want[3].shape == (5000, 5)


def test_the_fuzz_seed_set_holds_its_conditions():
    made = {}
    gpu_fuzz.seed_set_conditions(lambda seed: made.setdefault(seed, gpu_fuzz.link_shape(seed)))
    assert len(made) == 24
