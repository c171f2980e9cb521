"""Weighted sampling without a GPU: the numpy restatement (tests/weighted_ref.py) against the existing oracle under unit weights, the
pick rule's frequencies over a hand-made row, the arguments engine refuses before it touches a device, and the new C entry points in
the header, the ctypes table and the library."""
import os
import re
import subprocess

import numpy as np
import pytest

from legion_amd import engine, lib
from tests import weighted_ref as ref
from tests.helpers import KEYS_EXACT, Workload
from tests.test_oracle_sampler import oracle_batch, tiny_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "legion_hip.h")
LIB = os.path.join(ROOT, "legion_amd", "liblegion_hip.so")
NEW_SYMBOLS = ("legion_graph_set_edge_weights", "legion_graph_edge_cdf", "legion_pool_set_sample_weighted", "legion_pool_sample_weighted",
               "legion_pipeline_set_sample_weighted", "legion_draw_weighted_batch")


@pytest.mark.parametrize("fanout", [[3], [3, 2], [25, 10], [2, 2, 2]])
def test_unit_weights_are_the_oracle_batch(fanout):
    """All weights 1.0f: the table is 1, 2, .. D per row and the pick is floor(r * D), the uniform draw -- the whole batch is the
    existing oracle's."""
    indptr, col = tiny_graph()
    seeds = np.array([0, 6, 7, 3, 1], dtype=np.int32)
    table = ref.cdf(indptr, np.ones(col.size, np.float32))
    got = ref.run_batch(indptr, col, table, seeds, np.zeros_like(seeds), 4, 0, fanout)
    want = oracle_batch(indptr, col, seeds, fanout, 4)
    for k in KEYS_EXACT:
        assert np.array_equal(got[k], want[k]), k
    wl = Workload(scale=9, edge_factor=8, dim=0, n_seeds=100)
    ids, labels = wl.sets[(0, 0)]
    table = ref.cdf(wl.indptr, np.ones(wl.E, np.float32))
    for counter in (0, 3):                                                        # 3: the clamped last batch
        got = ref.run_batch(wl.indptr, wl.col, table, ids, labels, 32, counter, fanout)
        want = oracle_batch(wl.indptr, wl.col, ids, fanout, 32, counter=counter, mode=0)
        for k in ("node_counter", "edge_counter", "sampled_ids", "agg_src_ids", "agg_dst_ids", "agg_src_off", "agg_dst_off"):
            assert np.array_equal(got[k], want[k]), (counter, k)
        ref.check_edges(wl.indptr, wl.col, np.ones(wl.E, np.float32), got)


def test_table_sanitises_and_repeats_over_zero_weights():
    indptr = np.array([0, 0, 3, 8, 9], dtype=np.int64)
    w = np.array([1, -2, np.nan, np.inf, 0.5, -0.0, -np.inf, 0.25, 0], dtype=np.float32)
    assert ref.sanitise(w).tolist() == [1, 0, 0, 0, 0.5, 0, 0, 0.25, 0]
    assert ref.cdf(indptr, w).tolist() == [1, 1, 1, 0, 0.5, 0.5, 0.5, 0.75, 0]
    assert ref.cdf(indptr, w).dtype == np.float32
    # a slot of the all-zero row and of the empty row has no pick; a zero-weight entry is never picked
    p = ref.picks(np.array([0, 4, 8, 12]), indptr[:4], np.diff(indptr), 4, ref.cdf(indptr, w))
    assert p[0].tolist() == [-1] * 4 and p[3].tolist() == [-1] * 4
    assert p[1].tolist() == [0, 0, 0, -1] and set(p[2].tolist()) <= {1, 4}      # (row 1 has three entries)


def test_frequencies_follow_the_weights():
    """A row of D = 8 with weights [0, 1, 0, 3, 4, 0, 8, 0] / 8 over 200 000 consecutive slots: each position's count within five
    binomial standard deviations of n w / T, zero-weight positions never.  The sequence is fixed: this passes or it does not."""
    w = (np.array([0, 1, 0, 3, 4, 0, 8, 0], dtype=np.float32) / np.float32(8))
    indptr = np.array([0, 8], dtype=np.int64)
    table = ref.cdf(indptr, w)
    n = 200000
    p = ref.pick_slots(np.arange(n), np.zeros(n, np.int64), np.full(n, 8), table)
    counts = np.bincount(p, minlength=8)
    assert counts.sum() == n and p.min() >= 0
    prob = w.astype(np.float64) / float(w.sum())
    for i in range(8):
        if w[i] == 0:
            assert counts[i] == 0, i
        else:
            sd = np.sqrt(n * prob[i] * (1 - prob[i]))
            assert abs(counts[i] - n * prob[i]) <= 5 * sd, (i, counts[i], n * prob[i], sd)


def test_pick_is_the_count_of_entries_at_or_below_the_target():
    """pick_slots against the definition written out slot by slot, on rows with ties, zeros and one entry."""
    rng = np.random.RandomState(3)
    deg = np.array([1, 2, 5, 17, 64, 0, 3], dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    w = (rng.randint(0, 5, int(indptr[-1])) / 8).astype(np.float32)
    w[indptr[6]:indptr[7]] = 0
    table = ref.cdf(indptr, w)
    for v in range(deg.size):
        idx = np.arange(100) + 1000 * v
        got = ref.pick_slots(idx, np.full(100, indptr[v]), np.full(100, deg[v]), table)
        row = table[indptr[v]:indptr[v + 1]].astype(np.float64)
        for i, r in zip(got.tolist(), ref.unit_r(idx).tolist()):
            if deg[v] == 0 or row[-1] == 0:
                assert i == -1
            else:
                assert i == int((row <= r * row[-1]).sum()) and w[indptr[v] + i] > 0


@pytest.mark.parametrize("bad", [1, 0, "yes", None, 1.0])
def test_engine_refuses_a_non_bool_before_touching_a_device(bad):
    with pytest.raises(ValueError, match="weighted"):
        engine.MemoryPool(0, 100, 8, [2], 4, weighted=bad)
    with pytest.raises(ValueError, match="weighted"):
        engine.Pipeline(None, None, None, 0, 8, [2], 2, 16, weighted=bad)
    pool = engine.MemoryPool.__new__(engine.MemoryPool)       # (no handle: the check comes before the library call)
    with pytest.raises(ValueError, match="weighted"):
        pool.set_weighted(bad)
    pipe = engine.Pipeline.__new__(engine.Pipeline)
    with pytest.raises(ValueError, match="weighted"):
        pipe.set_weighted(bad)


def test_engine_refuses_weights_of_a_wrong_size_or_dtype():
    g = engine.GraphStorage.__new__(engine.GraphStorage)      # (no handle: the checks come before the library call)
    g.edge_num = 10
    with pytest.raises(ValueError, match="float32"):
        g.set_edge_weights(np.ones(10, np.float64))
    with pytest.raises(ValueError, match="float32"):
        g.set_edge_weights(np.ones(10, np.int32))
    with pytest.raises(ValueError, match="one entry per edge"):
        g.set_edge_weights(np.ones(9, np.float32))
    with pytest.raises(ValueError, match="one entry per edge"):
        g.set_edge_weights(np.ones((5, 2), np.float32))
    with pytest.raises(ValueError, match="tensor or array"):
        g.set_edge_weights([1.0] * 10)


def test_new_symbols_in_header_ctypes_table_and_library():
    text = open(HEADER).read()
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in lib.SIGNATURES and name in exported, name
    assert lib.SIGNATURES["legion_graph_set_edge_weights"] == (lib.c_i32, [lib.c_p, lib.c_p, lib.c_p])
    assert lib.SIGNATURES["legion_graph_edge_cdf"] == (lib.c_p, [lib.c_p])
    assert lib.SIGNATURES["legion_pool_set_sample_weighted"] == (lib.c_i32, [lib.c_p, lib.c_i32])
    assert lib.SIGNATURES["legion_pool_sample_weighted"] == (lib.c_i32, [lib.c_p])
    assert lib.SIGNATURES["legion_pipeline_set_sample_weighted"] == (lib.c_i32, [lib.c_p, lib.c_i32])
    assert lib.SIGNATURES["legion_draw_weighted_batch"] == (None, [lib.c_p] * 6 + [lib.c_i32])


def test_null_handles_and_bad_values_are_refused():
    L = lib.load()
    assert L.legion_graph_set_edge_weights(None, None, None) == -1
    assert not L.legion_graph_edge_cdf(None)
    assert L.legion_pool_set_sample_weighted(None, 1) == -1
    assert L.legion_pool_set_sample_weighted(None, 2) == -1
    assert L.legion_pool_sample_weighted(None) == -1
    assert L.legion_pipeline_set_sample_weighted(None, 1) == -1
    assert L.legion_pipeline_set_sample_weighted(None, 7) == -1
