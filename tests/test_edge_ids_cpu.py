"""The edge-id mode without a GPU: the numpy restatement (tests/edge_ids_ref.py) against a slot-by-slot statement in plain Python
and against the oracle's batch, the arguments engine.MemoryPool / engine.Pipeline refuse before they touch a device, and the new
C entry points in the header, the ctypes table and the library."""
import os
import re
import subprocess

import numpy as np
import pytest

from legion_amd import engine, lib
from oracle import ffi
from tests import edge_ids_ref as ref
from tests.helpers import Workload, compare_batches
from tests.test_oracle_sampler import oracle_batch, tiny_graph
from tests.test_sample_distinct_cpu import py_picks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "legion_hip.h")
LIB = os.path.join(ROOT, "legion_amd", "liblegion_hip.so")
NEW_SYMBOLS = ("legion_pool_set_edge_ids", "legion_pool_edge_ids", "legion_pipeline_set_edge_ids")


def py_edges(indptr, col, seeds, fanout, replace):
    """(vertex sampled for, neighbour, position in col) of every edge, hop after hop, slot by slot."""
    L = ffi.load()
    out, frontier = [], list(seeds)
    for f in fanout:
        hop = []
        for q, s in enumerate(frontier):
            D = int(indptr[s + 1] - indptr[s]) if s >= 0 else 0
            pk = [int(L.lgo_draw(q * f + k, D)) for k in range(min(f, D))] if replace else py_picks(q, f, D)
            for p in pk:
                at = int(indptr[s]) + p
                if col[at] >= 0:
                    hop.append((s, int(col[at]), at))
        out += hop
        frontier = [e[1] for e in hop]
    return out


def dead_and_parallel_graph():
    """tiny_graph with parallel edges (v0 lists 1, 2, 3 twice already; v3 lists 4 three times) and dead column entries (-1)."""
    adj = {0: [1, 2, 3, 4, 5, 6, 1, 2, 3], 1: [0, -1, 2], 2: [0, 1, 3, -1], 3: [4, 0, 4, 2, 4, 5], 4: [0, 3],
           5: [-1, 0, 3, 6], 6: [5, 5], 7: []}
    indptr = np.zeros(9, dtype=np.int64)
    col = []
    for v in range(8):
        col += adj[v]
        indptr[v + 1] = len(col)
    return indptr, np.array(col, dtype=np.int32)


@pytest.mark.parametrize("replace", [True, False], ids=["replace", "distinct"])
@pytest.mark.parametrize("fanout", [[3, 2], [25, 10], [2, 2, 2], [1], [4, 1, 3]])
@pytest.mark.parametrize("graph", [tiny_graph, dead_and_parallel_graph], ids=["tiny", "dead-and-parallel"])
def test_helper_against_the_slot_by_slot_statement(graph, fanout, replace):
    indptr, col = graph()
    seeds = np.array([0, 6, 7, 3], dtype=np.int32)
    got = ref.run_batch(indptr, col, seeds, np.zeros_like(seeds), 4, 0, fanout, replace)
    want = py_edges(indptr, col, seeds.tolist(), fanout, replace)
    assert got["agg_dst_ids"].tolist() == [e[0] for e in want]
    assert got["agg_src_ids"].tolist() == [e[1] for e in want]
    assert got["agg_edge_ids"].tolist() == [e[2] for e in want] and got["agg_edge_ids"].dtype == np.int64
    ref.check_edge_ids(indptr, col, got)
    assert got["edge_counter"][9 + len(fanout)] == len(want)


@pytest.mark.parametrize("fanout", [[3, 2], [25, 10], [2, 2, 2]])
def test_helper_with_replacement_is_the_oracle_batch(fanout):
    """Everything but the edge ids is what the existing oracle computes: the helper adds a key, nothing else."""
    indptr, col = tiny_graph()
    seeds = np.array([0, 6, 7, 3, 1], dtype=np.int32)
    compare_batches(ref.run_batch(indptr, col, seeds, np.zeros_like(seeds), 4, 0, fanout, True),
                    oracle_batch(indptr, col, seeds, fanout, 4), f"{fanout}: ")
    wl = Workload(scale=9, edge_factor=8, dim=0, n_seeds=100)
    ids, labels = wl.sets[(0, 0)]
    got = ref.run_batch(wl.indptr, wl.col, ids, labels, 32, 3, fanout, True)      # the clamped last batch
    want = oracle_batch(wl.indptr, wl.col, ids, fanout, 32, counter=3, mode=0)
    for k in ("node_counter", "edge_counter", "sampled_ids", "agg_src_ids", "agg_dst_ids", "agg_src_off", "agg_dst_off"):
        assert np.array_equal(got[k], want[k]), k
    ref.check_edge_ids(wl.indptr, wl.col, got)


def test_distinct_rows_list_their_edges_in_order():
    """replace=False with f >= D: a row's ids are indptr[s] .. indptr[s+1]-1 in order minus the dead entries; parallel edges get
    ids of their own."""
    indptr, col = dead_and_parallel_graph()
    seeds = np.array([3, 0, 5, 7, 1], dtype=np.int32)
    got = ref.run_batch(indptr, col, seeds, np.zeros_like(seeds), 5, 0, [9], False)
    want = [e for s in seeds.tolist() for e in range(int(indptr[s]), int(indptr[s + 1])) if col[e] >= 0]
    assert got["agg_edge_ids"].tolist() == want
    three = got["agg_edge_ids"][(got["agg_dst_ids"] == 3) & (got["agg_src_ids"] == 4)]
    assert three.size == 3 and np.unique(three).size == 3


@pytest.mark.parametrize("bad", [1, 0, "yes", None, 1.0])
def test_engine_refuses_a_non_bool_before_touching_a_device(bad):
    with pytest.raises(ValueError, match="edge_ids"):
        engine.MemoryPool(0, 100, 8, [2], 4, edge_ids=bad)
    with pytest.raises(ValueError, match="edge_ids"):
        engine.Pipeline(None, None, None, 0, 8, [2], 2, 16, edge_ids=bad)
    pool = engine.MemoryPool.__new__(engine.MemoryPool)       # (no handle: the check comes before the library call)
    with pytest.raises(ValueError, match="edge_ids"):
        pool.set_edge_ids(bad)
    pipe = engine.Pipeline.__new__(engine.Pipeline)
    with pytest.raises(ValueError, match="edge_ids"):
        pipe.set_edge_ids(bad)


def test_engine_names_the_buffer():
    assert engine.MemoryPool._BUF["agg_edge_ids"][0] == 14
    import torch
    assert engine.MemoryPool._BUF["agg_edge_ids"][1] == torch.int64


def test_new_symbols_in_header_ctypes_table_and_library():
    text = open(HEADER).read()
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in lib.SIGNATURES and name in exported, name
    assert lib.SIGNATURES["legion_pool_set_edge_ids"] == (lib.c_i32, [lib.c_p, lib.c_i32])
    assert lib.SIGNATURES["legion_pool_edge_ids"] == (lib.c_i32, [lib.c_p])
    assert lib.SIGNATURES["legion_pipeline_set_edge_ids"] == (lib.c_i32, [lib.c_p, lib.c_i32])


def test_null_handles_are_refused():
    L = lib.load()
    assert L.legion_pool_set_edge_ids(None, 1) == -1
    assert L.legion_pool_edge_ids(None) == -1
    assert L.legion_pipeline_set_edge_ids(None, 1) == -1
