"""PinSAGE's neighbour sampler without a GPU: the entry point in the header, the ctypes table and the library, the arguments
GraphStorage.pinsage_neighbors refuses before it touches a device, the numpy restatement's (tests/pinsage_ref.py) own properties on the
hand-built graph of the walk tests, and that the inputs of the GPU tests exercise what they claim to."""
import os
import re
import subprocess

import numpy as np
import pytest

from legion_amd import engine, lib
from tests import pinsage_ref as ref
from tests import walk_ref
from tests import weighted_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "legion_hip.h")
LIB = os.path.join(ROOT, "legion_amd", "liblegion_hip.so")
M31 = 2 ** 31 - 1


@pytest.fixture(scope="module")
def world():
    indptr, col, w = walk_ref.hand_graph()
    return {"indptr": indptr, "col": col, "w": w, "table": weighted_ref.cdf(indptr, w), "seeds": walk_ref.seeds_for(257)}


# ---- the entry point ------------------------------------------------------------------------------------------------------------
def test_symbol_in_header_ctypes_table_and_library():
    text = open(HEADER).read()
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert re.search(r"\bint32_t\s+legion_pinsage_neighbors\s*\(", text)
    assert re.search(r"#define\s+LEGION_PINSAGE_MAX_VISITS\s+1024\b", text)
    assert "legion_pinsage_neighbors" in exported
    assert lib.SIGNATURES["legion_pinsage_neighbors"] == (lib.c_i32, [lib.c_p, lib.c_p, lib.c_p, lib.c_i32, lib.c_i32, lib.c_i32,
                                                                       lib.c_i32, lib.c_i32, lib.ctypes.c_float, lib.c_i64, lib.c_p,
                                                                       lib.c_p])
    assert engine.GraphStorage.PINSAGE_MAX_VISITS == ref.MAX_VISITS == 1024


def test_graph_storage_has_the_method():
    assert callable(getattr(engine.GraphStorage, "pinsage_neighbors", None))


def test_null_pointers_are_refused_before_anything_else():
    L = lib.load()
    assert L.legion_pinsage_neighbors(None, None, None, 1, 1, 1, 1, 0, 0.0, 0, None, None) == -1


def _bare_graph():
    g = engine.GraphStorage.__new__(engine.GraphStorage)      # (no handle: the checks come before the library call)
    g.node_num, g.edge_num = 10, 20
    return g


@pytest.mark.parametrize("kw, match", [
    (dict(num_random_walks=0), "num_random_walks"), (dict(num_random_walks=-2), "num_random_walks"),
    (dict(num_random_walks=2.0), "num_random_walks"), (dict(num_random_walks=True), "num_random_walks"),
    (dict(walk_length=0), "walk_length"), (dict(walk_length=-1), "walk_length"), (dict(walk_length=1.5), "walk_length"),
    (dict(num_neighbors=0), "num_neighbors"), (dict(num_neighbors=-4), "num_neighbors"), (dict(num_neighbors=None), "num_neighbors"),
    (dict(num_random_walks=41, walk_length=25), "visits per seed"), (dict(num_random_walks=1025, walk_length=1), "visits per seed"),
    (dict(num_random_walks=1, walk_length=1025), "visits per seed"),
    (dict(num_neighbors=1025), "num_neighbors"),
    (dict(base=-1), "base"), (dict(base=1.5), "base"),
    (dict(base=M31 - 3 * 5 * 4 + 1), "draw index"), (dict(base=2 ** 40), "draw index"),
    (dict(weighted=1), "weighted"), (dict(weighted=None), "weighted"),
    (dict(termination_prob=-0.1), "termination_prob"), (dict(termination_prob=1.5), "termination_prob"),
    (dict(termination_prob=float("nan")), "termination_prob"), (dict(termination_prob="0.5"), "termination_prob"),
    (dict(termination_prob=None), "termination_prob"),
])
def test_engine_refuses_before_touching_a_device(kw, match):
    args = dict(num_random_walks=5, walk_length=4, num_neighbors=3)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        _bare_graph().pinsage_neighbors(np.array([1, 2, 3], dtype=np.int32), **args)


def test_engine_refuses_seeds_of_a_wrong_dtype_or_shape():
    import torch
    with pytest.raises(ValueError, match="int32"):
        _bare_graph().pinsage_neighbors(torch.tensor([1, 2], dtype=torch.int64), 3, 2, 1)
    with pytest.raises(ValueError, match="one-dimensional"):
        _bare_graph().pinsage_neighbors(np.zeros((2, 2), dtype=np.int32), 3, 2, 1)


def test_the_largest_legal_values_are_accepted_by_the_python_check():
    check = engine.GraphStorage._check_pinsage
    check(3, 5, 4, 3, 0.5, False, M31 - 60)
    check(0, 64, 16, 1024, 1.0, True, M31)
    check(1, 1024, 1, 1, 0.0, False, 0)
    check(1, 1, 1024, 1, 0, False, 0)
    assert not ref.refused(3, 5, 4, 3, 0, 0.5, M31 - 60, False) and ref.refused(3, 5, 4, 3, 0, 0.5, M31 - 59, False)
    assert not ref.refused(1, 64, 16, 1024, 0, 0.5, 0, False)
    assert ref.refused(1, 41, 25, 3, 0, 0.5, 0, False) and ref.refused(1, 5, 4, 1025, 0, 0.5, 0, False)
    assert ref.refused(1, 5, 4, 3, 1, 0.5, 0, False) and not ref.refused(1, 5, 4, 3, 1, 0.5, 0, True)


# ---- the reference's own properties ---------------------------------------------------------------------------------------------
def _reachable(world, seeds):
    """Per seed the set of vertices some path of live column entries reaches from it (any length >= 1), for the few seeds asked for."""
    indptr, col = world["indptr"], world["col"]
    out = []
    for s in seeds:
        seen, frontier = set(), [int(s)] if 0 <= s < walk_ref.NODE_NUM else []
        while frontier:
            nxt = []
            for v in frontier:
                for u in col[indptr[v]:indptr[v + 1]]:
                    if u >= 0 and int(u) not in seen:
                        seen.add(int(u))
                        nxt.append(int(u))
            frontier = nxt
        out.append(seen)
    return out


@pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "weighted"])
@pytest.mark.parametrize("shape", [(10, 2, 3), (7, 9, 5), (65, 3, 200)])
def test_rows_are_ordered_bounded_and_reachable(world, weighted, shape):
    R, T, k = shape
    seeds = world["seeds"][:40]
    reads = {}
    vis = ref.visits(world["indptr"], world["col"], seeds, R, T, table=world["table"] if weighted else None, termination_prob=0.3,
                     base=40, reads=reads)
    walk_ref.assert_reads_in_bounds(reads, walk_ref.NODE_NUM, world["col"].size)
    nb, ct = ref.topk(vis, k)
    assert nb.shape == ct.shape == (40, k) and nb.dtype == ct.dtype == np.int32
    assert np.all(ct.sum(axis=1) <= R * T) and np.all((nb >= 0) == (ct > 0)) and np.all(nb[ct == 0] == -1)
    reach = _reachable(world, seeds[:12])
    for i in range(40):
        m = int((ct[i] > 0).sum())
        assert np.all(ct[i, m:] == 0)                                          # the filled slots come first
        key = list(zip((-ct[i, :m]).tolist(), nb[i, :m].tolist()))
        assert all(a < b for a, b in zip(key, key[1:])), (i, key)              # strictly ordered by (-count, id)
        for u, c in zip(nb[i, :m], ct[i, :m]):
            assert int((vis[i] == u).sum()) == c
        if i < 12:
            assert set(nb[i, :m].tolist()) <= reach[i], i
        if m < k:                                                              # a short row holds every distinct visit
            assert m == np.unique(vis[i][vis[i] >= 0]).size


def test_termination_one_leaves_exactly_the_first_steps(world):
    R, T = 6, 5
    vis = ref.visits(world["indptr"], world["col"], world["seeds"], R, T, termination_prob=1.0, base=7).reshape(-1, T)
    first = walk_ref.walk(world["indptr"], world["col"], np.repeat(world["seeds"], R), T, base=7)[0][:, 1]
    assert np.array_equal(vis[:, 0], first) and np.all(vis[:, 1:] == -1) and (first >= 0).any()


@pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "weighted"])
def test_termination_zero_is_the_walk_over_repeated_seeds(world, weighted):
    R, T, table = 5, 13, world["table"] if weighted else None
    vis = ref.visits(world["indptr"], world["col"], world["seeds"], R, T, table=table, termination_prob=0.0, base=123)
    traces = walk_ref.walk(world["indptr"], world["col"], np.repeat(world["seeds"], R), T, table=table, base=123)[0]
    assert np.array_equal(vis.reshape(-1, T), traces[:, 1:])


def test_later_steps_take_the_walks_restart_draw(world):
    """From the second step on the visits are those of the walk with restart_prob = termination_prob, given where the first step went."""
    R, T, p = 4, 6, 0.3
    vis = ref.visits(world["indptr"], world["col"], world["seeds"], R, T, termination_prob=p, base=11).reshape(-1, T)
    full = walk_ref.walk(world["indptr"], world["col"], np.repeat(world["seeds"], R), T, restart_prob=p, base=11)[0]
    same_first = full[:, 1] == vis[:, 0]
    assert np.array_equal(vis[same_first], full[same_first, 1:])
    assert (~same_first).any() and np.all(full[~same_first, 1] == -1)        # the walk's own first step may end on its restart draw


def test_unit_weights_are_the_unweighted_sampler(world):
    unit = weighted_ref.cdf(world["indptr"], np.ones(world["col"].size, np.float32))
    a = ref.neighbors(world["indptr"], world["col"], world["seeds"], 10, 2, 3, base=1000)
    b = ref.neighbors(world["indptr"], world["col"], world["seeds"], 10, 2, 3, table=unit, base=1000)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_seeds_outside_the_graph_read_nothing(world):
    reads = {}
    seeds = np.array([-1, walk_ref.NODE_NUM, -7, 2 ** 31 - 1], dtype=np.int32)
    nb, ct = ref.neighbors(world["indptr"], world["col"], seeds, 10, 2, 3, table=world["table"], reads=reads)
    assert np.all(nb == -1) and np.all(ct == 0)
    assert all(i.size == 0 for chunks in reads.values() for i in chunks)


# ---- the inputs of the GPU tests exercise what they claim to ------------------------------------------------------------------------
def test_the_gpu_inputs_have_ties_repeats_short_and_empty_rows(world):
    """seeds_for(257), base 40 on the hand graph.  (10, 2, 3) at 0.5: rows with more than k distinct vertices, ties across the k
    boundary, counts above 1 and empty rows; (65, 3, 200) weighted at 0: rows shorter than k."""
    seeds = world["seeds"]
    vis = ref.visits(world["indptr"], world["col"], seeds, 10, 2, termination_prob=0.5, base=40)
    nb, ct = ref.topk(vis, 3)
    more, tie = 0, 0
    for i in range(seeds.size):
        ids, c = np.unique(vis[i][vis[i] >= 0], return_counts=True)
        if ids.size > 3:
            more += 1
            c = np.sort(c)[::-1]
            tie += int(c[2] == c[3])
    many = int((ct.max(axis=1) > 1).sum())
    empty = int((ct[:, 0] == 0).sum())
    print("more than k:", more, "tie at the boundary:", tie, "a count > 1:", many, "empty:", empty)
    assert more > 0 and tie > 0 and many > 0 and empty > 0
    nb, ct = ref.neighbors(world["indptr"], world["col"], seeds, 65, 3, 200, table=world["table"], termination_prob=0.0, base=40)
    short = int(((ct[:, -1] == 0) & (ct[:, 0] > 0)).sum())
    print("short rows:", short, "with every slot filled:", int((ct[:, -1] > 0).sum()))
    assert short > 0
