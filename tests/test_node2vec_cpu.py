"""node2vec walks without a GPU: the two new entry points in the header, the ctypes table and the library, the arguments
GraphStorage.node2vec_random_walk refuses before it touches a device, and the numpy restatement's (tests/node2vec_ref.py) own properties
on the symmetric graph the GPU tests walk: it is walk_ref's walk at p = q = 1 and at max_tries = 1, its transitions are edges, it reads
inside its arrays, its draws are the definition's, and its transition frequencies are node2vec's."""
import os
import re
import subprocess

import numpy as np
import pytest

from legion_amd import engine, lib
from tests import node2vec_ref as ref
from tests import walk_ref
from tests import weighted_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "legion_hip.h")
LIB = os.path.join(ROOT, "legion_amd", "liblegion_hip.so")
FREQ_BASE = 0                                                      # the fixed draw sequence of the frequency tests


@pytest.fixture(scope="module")
def world():
    indptr, col, w = ref.sym_graph()
    return {"indptr": indptr, "col": col, "w": w, "table": weighted_ref.cdf(indptr, w), "seeds": ref.seeds_for(600)}


# ---- the entry points -----------------------------------------------------------------------------------------------------------
def test_symbols_in_header_ctypes_table_and_library():
    text = open(HEADER).read()
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert re.search(r"\bint32_t\s+legion_node2vec_walk\s*\(", text) and re.search(r"\bint32_t\s+legion_graph_check_rows_sorted\s*\(", text)
    assert re.search(r"#define\s+LEGION_NODE2VEC_MAX_TRIES\s+256\b", text) and re.search(r"#define\s+LEGION_NODE2VEC_MAX_BIAS\s+16\b", text)
    assert {"legion_node2vec_walk", "legion_graph_check_rows_sorted"} <= exported
    assert lib.SIGNATURES["legion_node2vec_walk"] == (lib.c_i32, [lib.c_p, lib.c_p, lib.c_p, lib.c_i32, lib.c_i32, lib.ctypes.c_float,
                                                                   lib.ctypes.c_float, lib.c_i32, lib.c_i32, lib.c_i64, lib.c_p, lib.c_p])
    assert lib.SIGNATURES["legion_graph_check_rows_sorted"] == (lib.c_i32, [lib.c_p, lib.c_p])


def test_graph_storage_has_the_methods():
    assert callable(getattr(engine.GraphStorage, "node2vec_random_walk", None))
    assert callable(getattr(engine.GraphStorage, "rows_sorted", None))
    assert engine.GraphStorage.NODE2VEC_MAX_TRIES == ref.MAX_TRIES and engine.GraphStorage.NODE2VEC_MAX_BIAS == ref.MAX_BIAS


def test_null_pointers_are_refused_before_anything_else():
    L = lib.load()
    assert L.legion_node2vec_walk(None, None, None, 1, 1, 1.0, 1.0, 0, 256, 0, None, None) == -1
    assert L.legion_graph_check_rows_sorted(None, None) == -1


def test_the_random_walk_contract_points_to_the_new_entry():
    text = open(HEADER).read()
    assert "node2vec's p / q bias is legion_node2vec_walk" in text and "Not offered: metapaths, node2vec" not in text


def _bare_graph():
    g = engine.GraphStorage.__new__(engine.GraphStorage)      # (no handle: the checks come before the library call)
    g.node_num, g.edge_num = 10, 20
    return g


@pytest.mark.parametrize("kw, match", [
    (dict(length=0), "length"), (dict(length=-3), "length"), (dict(length=2.0), "length"), (dict(length=True), "length"),
    (dict(base=-1), "base"), (dict(base=1.5), "base"),
    (dict(base=2 ** 31 - 1 - 3 * 4 + 1), "draw index"), (dict(length=2 ** 30), "draw index"),
    (dict(weighted=1), "weighted"), (dict(weighted=None), "weighted"), (dict(return_eids=0), "return_eids"),
    (dict(max_tries=0), "max_tries"), (dict(max_tries=257), "max_tries"), (dict(max_tries=-1), "max_tries"), (dict(max_tries=2.0), "max_tries"),
    (dict(max_tries=True), "max_tries"), (dict(max_tries=None), "max_tries"),
    (dict(p=0), "p must"), (dict(p=-1.0), "p must"), (dict(p=float("nan")), "p must"), (dict(p=float("inf")), "p must"),
    (dict(p="1"), "p must"), (dict(p=None), "p must"), (dict(p=True), "p must"), (dict(p=1e39), "p must"), (dict(p=1e-46), "p must"),
    (dict(q=0), "q must"), (dict(q=-0.5), "q must"), (dict(q=float("nan")), "q must"), (dict(q=float("inf")), "q must"),
    (dict(p=16.5), "too strong"), (dict(q=17), "too strong"), (dict(p=0.06), "too strong"), (dict(p=8, q=0.25), "too strong"),
    (dict(p=100, q=100), "too strong"), (dict(p=0.01, q=0.01), "too strong"),
])
def test_engine_refuses_before_touching_a_device(kw, match):
    args = dict(p=1.0, q=1.0, length=4)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        _bare_graph().node2vec_random_walk(np.array([1, 2, 3], dtype=np.int32), **args)


def test_engine_refuses_seeds_of_a_wrong_dtype_or_shape():
    import torch
    with pytest.raises(ValueError, match="int32"):
        _bare_graph().node2vec_random_walk(torch.tensor([1, 2], dtype=torch.int64), 1.0, 1.0, 3)
    with pytest.raises(ValueError, match="one-dimensional"):
        _bare_graph().node2vec_random_walk(np.zeros((2, 2), dtype=np.int32), 1.0, 1.0, 3)


def test_the_python_check_is_the_rule():
    """The edges of the rule are accepted on their legal side, and the check agrees with the reference's predicate over a grid."""
    ok = engine.GraphStorage._check_node2vec
    ok(3, 16.0, 1.0, 4, False, False, 256, 2 ** 31 - 1 - 12)
    ok(0, 1.0, 0.0625, 4, True, True, 1, 2 ** 31 - 1)
    ok(3, 4, 0.25, 4, False, False, 2, 0)
    for p in (0.0, -1.0, 0.05, 0.0625, 0.25, 1.0, 3.0, 16.0, 16.5, float("nan"), float("inf")):
        for q in (0.0, 0.0625, 0.25, 1.0, 4.0, 16.0, 20.0, float("nan")):
            for tries in (0, 1, 256, 257):
                want = ref.refused(3, 4, p, q, 0, tries, 0, False, 1)
                try:
                    ok(3, p, q, 4, False, False, tries, 0)
                    got = False
                except ValueError:
                    got = True
                assert got == want, (p, q, tries)


def test_the_predicate_knows_tables_and_sorted_rows():
    assert not ref.refused(3, 4, 1, 1, 1, 256, 0, True, 1) and ref.refused(3, 4, 1, 1, 1, 256, 0, False, 1)
    assert ref.refused(3, 4, 1, 1, 0, 256, 0, False, 0) and ref.refused(3, 4, 1, 1, 0, 256, 0, False, -1)
    assert not ref.refused(3, 4, 1, 1, 0, 256, 2 ** 31 - 1 - 12, False, 1) and ref.refused(3, 4, 1, 1, 0, 256, 2 ** 31 - 12, False, 1)


# ---- the graph ------------------------------------------------------------------------------------------------------------------
def test_the_graph_is_what_the_tests_need(world):
    indptr, col = world["indptr"], world["col"]
    deg = np.diff(indptr)
    assert indptr.size - 1 == ref.NODE_NUM and all(deg[h] == d for h, d in ref.HUBS.items()) and all(deg[v] == 0 for v in ref.EMPTY)
    assert ref.rows_sorted(indptr, col) and (col == -1).sum() >= 20 and col.min() == -1
    rows = np.repeat(np.arange(ref.NODE_NUM), deg)
    live = col >= 0
    fwd = set(zip(rows[live].tolist(), col[live].tolist()))
    back = sum((u, v) in fwd for v, u in fwd)
    assert back >= 0.99 * len(fwd)                                  # symmetric but for the entries made dead
    assert (rows[live] == col[live]).sum() >= 100                   # self-loops
    assert ((col[1:] == col[:-1]) & (rows[1:] == rows[:-1]) & live[1:]).sum() >= 100       # parallel edges
    w = world["w"]
    assert np.all(w[indptr[ref.ZERO_ROW]:indptr[ref.ZERO_ROW + 1]] == 0) and (w == 0).mean() > 0.1


def test_rows_sorted_is_about_rows_only():
    indptr = np.array([0, 2, 2, 4, 4, 5], dtype=np.int64)
    assert ref.rows_sorted(indptr, np.array([5, 9, 1, 3, 0], dtype=np.int32))              # decreases across row boundaries only
    assert not ref.rows_sorted(indptr, np.array([5, 9, 3, 1, 0], dtype=np.int32))
    assert not ref.rows_sorted(indptr, np.array([9, 5, 1, 3, 0], dtype=np.int32))
    assert ref.rows_sorted(indptr, np.array([-1, -1, 1, 1, 0], dtype=np.int32))
    assert ref.rows_sorted(np.zeros(4, np.int64), np.zeros(0, np.int32))


# ---- the reference's own properties ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "weighted"])
@pytest.mark.parametrize("p, q, tries", [(1.0, 1.0, 256), (1.0, 1.0, 3), (0.5, 2.0, 1), (4.0, 0.25, 1)])
def test_unbiased_and_single_try_walks_are_the_random_walk(world, weighted, p, q, tries):
    table = world["table"] if weighted else None
    want = walk_ref.walk(world["indptr"], world["col"], world["seeds"], 17, table=table, base=77)
    got = ref.walk(world["indptr"], world["col"], world["seeds"], 17, p, q, table=table, max_tries=tries, base=77)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "weighted"])
@pytest.mark.parametrize("p, q, tries", [(0.5, 2.0, 256), (4.0, 0.25, 256), (0.25, 4.0, 2), (16.0, 1.0, 3)])
def test_every_transition_is_an_edge_and_reads_stay_inside(world, weighted, p, q, tries):
    reads, stats = {}, ref.new_stats()
    traces, eids = ref.walk(world["indptr"], world["col"], world["seeds"], 17, p, q, table=world["table"] if weighted else None,
                            max_tries=tries, base=5, reads=reads, stats=stats)
    walk_ref.check(world["indptr"], world["col"], world["seeds"], traces, eids)
    walk_ref.assert_reads_in_bounds(reads, ref.NODE_NUM, world["col"].size)
    assert (traces[:, 5] >= 0).any() and (traces[:, 1] < 0).any()        # some walks go on, some end at once
    assert stats["steps"] == int((traces[:, 1:] >= 0).sum()) and stats["tries"] >= stats["steps"]
    assert all(stats["accepted"][c] > 0 for c in range(3))
    if weighted:
        live = eids >= 0
        assert np.all(weighted_ref.sanitise(world["w"])[eids[live]] > 0)  # an entry of weight zero is never a candidate
        assert np.all(traces[world["seeds"] == ref.ZERO_ROW, 1] == -1)    # the all-zero row yields no step


def test_seeds_outside_the_graph_read_nothing(world):
    reads = {}
    seeds = np.array([-1, ref.NODE_NUM, -7, 2 ** 31 - 1], dtype=np.int32)
    traces, eids = ref.walk(world["indptr"], world["col"], seeds, 5, 0.5, 2.0, table=world["table"], reads=reads)
    assert np.array_equal(traces[:, 0], seeds) and np.all(traces[:, 1:] == -1) and np.all(eids == -1)
    assert all(i.size == 0 for chunks in reads.values() for i in chunks)


def test_the_draws_of_a_step_are_the_definitions(world):
    """One walk from the long row, two steps, followed by hand with pow(48271, k, 2^31 - 1) at the indices the contract names."""
    indptr, col = world["indptr"], world["col"]
    p, q, base, length = 0.25, 4.0, 123456, 2
    a, b, mx = ref.bias(p, q)
    for w in range(40):
        seeds = np.full(w + 1, 6, dtype=np.int32)
        traces, eids = ref.walk(indptr, col, seeds, length, p, q, base=base)
        n = base + w * length
        s, D = int(indptr[6]), int(indptr[7] - indptr[6])
        pick = int((walk_ref.minstd(n + 1) - 1) / 2147483646.0 * D)
        assert eids[w, 0] == s + pick                                    # step 1: taken as drawn
        t, v = 6, int(col[s + pick])
        n, s, D = n + 1, int(indptr[v]), int(indptr[v + 1] - indptr[v])
        for i in range(ref.MAX_TRIES):
            x = walk_ref.minstd(n + 1 + i * 2 ** 23)
            pick = int((x - 1) / 2147483646.0 * D)
            u = int(col[s + pick])
            if u < 0:
                assert traces[w, 2] == -1
                break
            wt = a if u == t else 1.0 if u in col[indptr[t]:indptr[t + 1]] else b
            y = walk_ref.minstd(n + 1 + i * 2 ** 23 + 2 ** 22)
            if (y - 1) / 2147483646.0 * mx < wt:
                assert traces[w, 2] == u and eids[w, 1] == s + pick, (w, i)
                break
        else:
            raise AssertionError("256 rejections")


def test_draw_indices_of_a_step_are_distinct():
    assert 255 * 2 ** 23 + 2 ** 22 < 2 ** 31 - 2                          # inside one period of 48271: no two of a step's 512 coincide
    assert walk_ref.minstd(2 ** 31 - 2) == 1 and walk_ref.minstd(2 ** 30 - 1) != 1


# ---- frequencies ----------------------------------------------------------------------------------------------------------------
FREQ_SEEDS = [100, 101, 102, 2000, 2001, 4500, 4501, 0]              # lattice vertices and the 63-entry hub


def _frequencies(world, p, q, weighted):
    """240 000 walks of two steps from FREQ_SEEDS: the second step of every walk is a node2vec transition out of (t, v) = (seed, first
    step).  Returns the worst deviation in binomial standard deviations over the (t, v, u) cells with an expected count >= 50, and
    their number; rows with a dead entry (a walk that draws it ends: not a transition) are left out."""
    indptr, col = world["indptr"], world["col"]
    ws = weighted_ref.sanitise(world["w"]).astype(np.float64) if weighted else np.ones(col.size)
    a, b, mx = ref.bias(p, q)
    n = 240000
    seeds = np.array(FREQ_SEEDS, dtype=np.int32)[np.arange(n) % len(FREQ_SEEDS)]
    traces, eids = ref.walk(indptr, col, seeds, 2, p, q, table=world["table"] if weighted else None, base=FREQ_BASE)
    walk_ref.check(indptr, col, seeds, traces, eids)
    worst, cells = 0.0, 0
    pairs = np.unique(traces[traces[:, 1] >= 0][:, :2], axis=0)
    for t, v in pairs:
        row = col[indptr[v]:indptr[v + 1]]
        if row.size == 0 or row.min() < 0:
            continue
        trow = col[indptr[t]:indptr[t + 1]]
        wt = np.array([a if u == t else 1.0 if u in trow else b for u in row]) * ws[indptr[v]:indptr[v + 1]]
        if wt.sum() == 0:
            continue
        here = (traces[:, 0] == t) & (traces[:, 1] == v)
        visits = int(here.sum())
        assert np.all(traces[here, 2] >= 0)
        for u in np.unique(row):
            prob = wt[row == u].sum() / wt.sum()
            if visits * prob < 50:
                continue
            got = int((traces[here, 2] == u).sum())
            sd = np.sqrt(visits * prob * (1 - prob)) if prob < 1 else 1.0
            worst, cells = max(worst, abs(got - visits * prob) / sd), cells + 1
    return worst, cells


@pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "weighted"])
@pytest.mark.parametrize("p, q", [(4.0, 0.25), (0.5, 2.0)])
def test_transition_frequencies_are_node2vecs(world, p, q, weighted):
    """Every (t, v, u) cell with an expected count of at least 50 lies within five binomial standard deviations of wt / sum wt (weighted:
    w wt / sum w wt).  The sequence is fixed: this passes or it does not."""
    worst, cells = _frequencies(world, p, q, weighted)
    print(f"p {p} q {q} weighted {weighted}: {cells} cells, worst {worst:.2f} sd")
    assert cells >= 150 and worst <= 5.0, (cells, worst)
