"""Weighted sampling on the GPU (GraphStorage.set_edge_weights, MemoryPool / Pipeline weighted=True): the prefix-sum table and the
pick rule bit for bit against the numpy restatement in tests/weighted_ref.py, whole batches bit for bit in every sampler class, with
and without edge ids, from the full CSR and from a cached topology -- and, under unit weights, bit for bit the existing oracle's."""
import ctypes

import numpy as np
import pytest
import torch

from tests import weighted_ref as ref
from tests.gpu_harness import CpuSide, GpuSide
from tests.helpers import KEYS_EXACT, Workload, compare_batches

pytestmark = pytest.mark.gpu

EIDS = pytest.mark.parametrize("edge_ids", [False, True], ids=["plain", "edge-ids"])
DEV = "cuda:0"


# ---- helpers ------------------------------------------------------------------------------------------------------------
def _weighted(wl, batch, fanout, w, edge_ids=False):
    """A GpuSide whose graph has the weights w and whose pools sample weighted."""
    gpu = GpuSide(wl, batch, fanout, edge_ids=edge_ids)
    assert gpu.graph.edge_cdf() is None
    gpu.graph.set_edge_weights(w)
    for pool in gpu.pools:
        pool.set_weighted(True)
        assert pool.weighted is True and pool.replace is True and pool.edge_ids is edge_ids
    return gpu


def _want(wl, table, it, mode, batch, fanout, **kw):
    ids, labels = wl.sets[(0, mode)]
    return ref.run_batch(wl.indptr, wl.col, table, ids, labels, batch, it, fanout, **kw)


def _check(got, want, wl, w, ctx, edge_ids):
    compare_batches(got, want, ctx)
    if edge_ids:
        assert "agg_edge_ids" in got and got["agg_edge_ids"].dtype == np.int64, f"{ctx}no agg_edge_ids"
        assert np.array_equal(got["agg_edge_ids"], want["agg_edge_ids"]), f"{ctx}agg_edge_ids"
        ref.check_edges(wl.indptr, wl.col, w, got)
    else:
        assert "agg_edge_ids" not in got
    if "float_features" in got and wl.D > 0:
        rows = got["float_features"][:want["sampled_ids"].size]
        assert np.array_equal(rows.view(np.uint32), wl.features[want["sampled_ids"]].view(np.uint32)), f"{ctx}gathered rows"


def _table_of(gpu, wl, w):
    """The GPU's table, which for these weights (multiples of 1/8, small totals) must be the reference's bit for bit."""
    table = ref.cdf(wl.indptr, w)
    torch.cuda.synchronize()
    assert np.array_equal(gpu.graph.edge_cdf().cpu().numpy().view(np.uint32), table.view(np.uint32)), "edge_cdf"
    return table


# ---- 1. the table and the pick rule on their own --------------------------------------------------------------------------
ROW_DEGREES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 70001, 300, 0, 5]      # (row 14: all weights zero)
ZERO_ROW = 14


@pytest.fixture(scope="module")
def rows():
    """A hand-built CSR over every row length at which the table build changes its path (a wave's 64 entries, a step's 1024 of the
    long-row workgroup, the 4096 above which a row gets a workgroup) and one row of 70 001."""
    from legion_amd import engine
    deg = np.array(ROW_DEGREES, dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    E = int(indptr[-1])
    col = (np.arange(E, dtype=np.int64) % deg.size).astype(np.int32)
    graph = engine.GraphStorage(1, torch.from_numpy(indptr).to(DEV), torch.from_numpy(col).to(DEV))
    rng = np.random.RandomState(7)
    w = (rng.randint(1, 33, E) / 8).astype(np.float32)                            # multiples of 1/8; the longest row totals < 2^21
    for v in range(deg.size):
        s, D = int(indptr[v]), int(deg[v])
        if D >= 2 and v % 2 == 0:
            w[s:s + max(D // 5, 1)] = 0                                           # a leading run of zeros
        if D >= 2 and v % 3 == 0:
            w[s + D - max(D // 7, 1):s + D] = 0                                   # a trailing run
        if D >= 60:
            w[s + D // 2:s + D // 2 + D // 9] = 0                                 # an inner run (across a wave's / a step's boundary)
    w[indptr[ZERO_ROW]:indptr[ZERO_ROW + 1]] = 0
    yield {"graph": graph, "indptr": indptr, "deg": deg, "w": w, "E": E}
    graph.close()


def test_table_is_the_reference_bit_for_bit(hip, rows):
    g = rows["graph"]
    g.set_edge_weights(rows["w"])
    torch.cuda.synchronize()
    got = g.edge_cdf().cpu().numpy()
    want = ref.cdf(rows["indptr"], rows["w"])
    assert got.dtype == np.float32 and got.shape == (rows["E"],)
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert bad.size == 0, f"{bad.size} entries differ, first at {bad[:5]}: got {got[bad[:5]]} want {want[bad[:5]]}"
    s = int(rows["indptr"][ZERO_ROW])
    assert not got[s:s + ROW_DEGREES[ZERO_ROW]].any()
    g.set_edge_weights(torch.ones(rows["E"], dtype=torch.float32, device=DEV))    # a second call replaces the table
    torch.cuda.synchronize()
    assert np.array_equal(g.edge_cdf().cpu().numpy(), ref.cdf(rows["indptr"], np.ones(rows["E"], np.float32)))


def test_table_properties_with_arbitrary_floats(hip, rows):
    """Negative values, NaN, +-inf, -0, denormals and ordinary floats over eleven orders of magnitude: the table is non-decreasing
    in a row, repeats over a sanitised zero, and is within 2^-23 (relative) of the exact sum."""
    g, indptr, E = rows["graph"], rows["indptr"], rows["E"]
    rng = np.random.RandomState(11)
    w = (rng.rand(E) * 10.0 ** rng.randint(-6, 6, E)).astype(np.float32)
    special = np.array([-1.5, np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-42, 3e-39, -1e-42], dtype=np.float32)
    at = rng.rand(E) < 0.3
    w[at] = special[rng.randint(0, special.size, int(at.sum()))]
    g.set_edge_weights(w)
    torch.cuda.synchronize()
    got = g.edge_cdf().cpu().numpy()
    ws = ref.sanitise(w)
    assert np.isfinite(got).all()
    for v in range(indptr.size - 1):
        s, e = int(indptr[v]), int(indptr[v + 1])
        if e == s:
            continue
        row, x = got[s:e], ws[s:e]
        prev = np.concatenate([[np.float32(0)], row[:-1]])
        assert np.all(row >= prev), f"row {v}: decreasing"
        assert np.all(row[x == 0] == prev[x == 0]), f"row {v}: a zero weight moved the table"
        exact = np.cumsum(x.astype(np.longdouble))
        assert np.all(np.abs(row.astype(np.longdouble) - exact) <= np.longdouble(2.0 ** -23) * exact), f"row {v}: off the exact sum"


def test_picks_are_the_reference_bit_for_bit(hip, rows):
    """legion_draw_weighted_batch over every row, 4096 slot indices each -- low ones, and a run that ends at 2^31 - 2."""
    g, indptr, deg = rows["graph"], rows["indptr"], rows["deg"]
    g.set_edge_weights(rows["w"])
    table = ref.cdf(indptr, rows["w"])
    n_rows, per = deg.size, 4096
    idx = np.empty((n_rows, per), dtype=np.int64)
    for v in range(n_rows):
        idx[v, :per // 2] = np.arange(per // 2) + 5000 * v
        idx[v, per // 2:] = (2 ** 31 - 1) - per // 2 + np.arange(per // 2) - 3 * v
    assert idx.max() == 2 ** 31 - 2
    row_start = np.repeat(indptr[:-1], per)
    d = np.repeat(deg, per).astype(np.int32)
    flat = idx.reshape(-1).astype(np.int32)
    t_idx, t_rs, t_d = (torch.from_numpy(a).to(DEV) for a in (flat, row_start, d))
    out = torch.full((flat.size,), -7, dtype=torch.int32, device=DEV)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    hip.legion_draw_weighted_batch(s, ctypes.c_void_p(t_idx.data_ptr()), ctypes.c_void_p(t_rs.data_ptr()), ctypes.c_void_p(t_d.data_ptr()),
                                   ctypes.c_void_p(g.edge_cdf().data_ptr()), ctypes.c_void_p(out.data_ptr()), flat.size)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    want = ref.pick_slots(flat, row_start, d, table)
    assert np.array_equal(got, want), f"{int((got != want).sum())} picks differ"
    got = got.reshape(n_rows, per)
    for v in (0, ZERO_ROW, 15):
        assert np.all(got[v] == -1)                                               # empty rows and the all-zero row
    for v in range(n_rows):
        if deg[v] > 0 and v != ZERO_ROW:
            assert got[v].min() >= 0 and got[v].max() < deg[v]
            assert np.all(rows["w"][indptr[v] + got[v]] > 0)                      # a zero weight is never drawn


# ---- 2. unit weights: the existing oracle pins the kernel -----------------------------------------------------------------
@pytest.mark.parametrize("fanout", [[25, 10], [3], [4, 3, 2]])
def test_unit_weights_are_the_oracle_batch(hip, fanout):
    wl = Workload(scale=11, edge_factor=8, dim=16, n_seeds=700)
    batch = 64
    w = np.ones(wl.E, np.float32)
    gpu = _weighted(wl, batch, fanout, w)
    cpu = CpuSide(wl, batch, fanout)
    n_train = (wl.sets[(0, 0)][0].size + batch - 1) // batch                      # the last batch is clamped
    for it, mode in [(0, 0), (1, 0), (n_train - 1, 0), (0, 1), (0, 2)]:
        compare_batches(gpu.run(0, it, mode), cpu.run(0, it, mode), f"{fanout} mode {mode} batch {it}: ")
    assert gpu.pools[0].error() == 0
    gpu.close()
    cpu.close()


# ---- 3. whole batches against the restatement -----------------------------------------------------------------------------
@EIDS
@pytest.mark.parametrize("fanout", [[5], [25, 10], [2, 2, 2]])
def test_exact_batches(hip, fanout, edge_ids):
    wl = Workload(scale=11, edge_factor=8, dim=16, n_seeds=700)
    batch = 64
    w = ref.hash_weights(wl.E, seed=len(fanout))
    gpu = _weighted(wl, batch, fanout, w, edge_ids)
    table = _table_of(gpu, wl, w)
    n_train = (wl.sets[(0, 0)][0].size + batch - 1) // batch
    first = None
    for it, mode in [(0, 0), (1, 0), (n_train - 1, 0), (0, 1), (0, 2)]:
        got = gpu.run(0, it, mode)
        _check(got, _want(wl, table, it, mode, batch, fanout), wl, w, f"{fanout} mode {mode} batch {it}: ", edge_ids)
        first = got if first is None else first
    # (the weights matter: the same batch under unit weights is another one)
    ids, labels = wl.sets[(0, 0)]
    other = ref.run_batch(wl.indptr, wl.col, ref.cdf(wl.indptr, np.ones(wl.E, np.float32)), ids, labels, batch, 0, fanout)
    assert not np.array_equal(other["agg_src_ids"], first["agg_src_ids"])
    assert gpu.pools[0].error() == 0
    gpu.close()


def test_presc_hotness_then_topology_cache(hip, col_slots):
    """PreSC in weighted mode: the hotness arrays are the restatement's; then rows served from the cached topology (with and without
    column slots) pick by the FULL CSR's positions of the table."""
    wl = Workload(scale=11, edge_factor=8, dim=32, n_seeds=700)
    fanout, batch = [6, 3], 64
    w = ref.hash_weights(wl.E, seed=9)
    gpu = _weighted(wl, batch, fanout, w, edge_ids=True)
    table = _table_of(gpu, wl, w)
    ea, na = np.zeros(wl.N, np.uint64), np.zeros(wl.N, np.uint64)
    steps = (wl.sets[(0, 0)][0].size - 1) // batch
    for it in range(steps):
        got = gpu.run(0, it, 0, is_presc=True)
        compare_batches(got, _want(wl, table, it, 0, batch, fanout, serve=False, edge_access=ea, node_access=na), f"presc {it}: ")
    assert np.array_equal(gpu.cache.array("edge_access_time", 0).cpu().numpy().view(np.uint64), ea)
    assert np.array_equal(gpu.cache.array("node_access_time", 0).cpu().numpy().view(np.uint64), na)
    gpu.cache.candidate_selection(0, gpu.graph)
    gpu.cache.set_capacity(150, 80)                     # rows served from the cached topology and the full CSR
    gpu.cache.fill_up(gpu.feature, gpu.graph)
    topo = 0
    for it in range(3):
        want = _want(wl, table, it, 0, batch, fanout)
        _check(gpu.run(0, it, 0), want, wl, w, f"cached topology {it}: ", True)
        ec = want["edge_counter"]
        tp = gpu.pools[0].buffer("tmp_part_ind")[:int(ec[10] - ec[9])].cpu().numpy()      # the last hop's frontier
        topo += int((tp >= 0).sum())
    assert topo > 0                                     # some rows did come from the cached topology
    assert gpu.graph.column_slots(0) == col_slots
    assert gpu.pools[0].error() == 0
    gpu.close()


# ---- 4. every bucket class and its overflow paths -------------------------------------------------------------------------
@EIDS
@pytest.mark.parametrize("buckets,claim_cap,known_cap", [("8", "1", None), ("8", "40", "3"), ("8", None, None), ("16", "1", "3"), ("16", "40", None),
                                                         ("16", None, None)])
def test_small_classes_with_list_overflow(hip, monkeypatch, buckets, claim_cap, known_cap, edge_ids):
    monkeypatch.setenv("LEGION_LDS_SMALL_BUCKETS", buckets)
    if claim_cap is not None:
        monkeypatch.setenv("LEGION_LDS_CLAIM_CAP", claim_cap)
    if known_cap is not None:
        monkeypatch.setenv("LEGION_LDS_KNOWN_CAP", known_cap)
    wl = Workload(scale=12, edge_factor=8, dim=4, n_seeds=600)
    fanout, batch = [4, 3, 3], 48
    w = ref.hash_weights(wl.E, seed=4)
    gpu = _weighted(wl, batch, fanout, w, edge_ids)
    table = _table_of(gpu, wl, w)
    assert gpu.pools[0].lds_buckets() == int(buckets)
    for it in range(3):
        _check(gpu.run(0, it, 0), _want(wl, table, it, 0, batch, fanout), wl, w, f"{buckets} buckets caps {claim_cap} {known_cap} batch {it}: ",
               edge_ids)
    assert gpu.pools[0].error() == 0
    gpu.close()


@pytest.fixture(scope="module")
def large():
    """The workload of the two large classes, its weights, table and expected batches (computed once per fan-out)."""
    wl = Workload(scale=15, edge_factor=16, dim=4, n_seeds=13000)
    w = ref.hash_weights(wl.E, seed=2)
    return {"wl": wl, "w": w, "table": ref.cdf(wl.indptr, w), "want": {}}


@EIDS
@pytest.mark.parametrize("fanout,n_buckets", [([10, 10], 64), ([10, 10, 8], 256)], ids=["64buckets", "256buckets"])
def test_large_classes(hip, large, fanout, n_buckets, edge_ids):
    wl, w, batch = large["wl"], large["w"], 6000
    gpu = _weighted(wl, batch, fanout, w, edge_ids)
    assert gpu.pools[0].lds_buckets() == n_buckets
    key = tuple(fanout)
    if key not in large["want"]:
        large["want"][key] = _want(wl, large["table"], 1, 0, batch, fanout)
    got = gpu.run(0, 1, 0)
    assert np.array_equal(gpu.graph.edge_cdf().cpu().numpy().view(np.uint32), large["table"].view(np.uint32))
    _check(got, large["want"][key], wl, w, f"{batch} {fanout}: ", edge_ids)
    assert gpu.pools[0].error() == 0
    gpu.close()


# ---- 5. lane groups, graph replay, the weave ------------------------------------------------------------------------------
@EIDS
@pytest.mark.parametrize("group,slots,use_graph,weave", [(4, 2, True, False), (3, 2, True, True), (2, 2, False, False)])
def test_pipeline_graph_replay_and_weave(hip, group, slots, use_graph, weave, edge_ids):
    from legion_amd import engine
    wl = Workload(scale=11, edge_factor=8, dim=32, n_seeds=700)
    fanout, batch = [6, 3], 64
    w = ref.hash_weights(wl.E, seed=6)
    gpu = GpuSide(wl, batch, fanout)
    gpu.graph.set_edge_weights(w)
    table = _table_of(gpu, wl, w)
    gpu.cache.candidate_selection(0, gpu.graph)
    gpu.cache.set_capacity(150, 80)
    gpu.cache.fill_up(gpu.feature, gpu.graph)
    pipe = engine.Pipeline(gpu.graph, gpu.feature, gpu.cache, 0, batch, fanout, group, gpu.pools[0].num_ids, use_graph, slots,
                           weave=weave, edge_ids=edge_ids, weighted=True)
    assert pipe.weighted is True
    n_batches = (wl.sets[(0, 0)][0].size + batch - 1) // batch
    n_groups = min((n_batches + group - 1) // group, 2 * slots)          # two passes over the slots: every graph is replayed
    for gi in range(n_groups):
        sl = pipe.submit(gi * group, 0)
        pipe.wait(sl)
        for lane in range(group):
            b = gi * group + lane
            _check(engine.read_batch(pipe.pools[sl][lane]), _want(wl, table, b, 0, batch, fanout), wl, w, f"group {gi} lane {lane}: ", edge_ids)
    with pytest.raises(RuntimeError):
        pipe.set_weighted(False)                        # the captured graphs never mix modes
    with pytest.raises(RuntimeError):
        gpu.graph.set_edge_weights(w)                   # ... and the table they read stays
    assert all(pool.error() == 0 for lanes in pipe.pools for pool in lanes)
    pipe.close()
    gpu.close()


# ---- 6. parallel edges, dead column entries, all-zero rows ----------------------------------------------------------------
def _hand_built_csr(n=40, seed=5):
    """A few dozen vertices of degree 0..8; rows list a neighbour two or three times, and some column entries are -1."""
    rng = np.random.RandomState(seed)
    indptr, col = [0], []
    for v in range(n):
        row = rng.randint(0, n, rng.randint(0, 6)).tolist()
        if v % 3 == 0 and row:
            row += [row[0]] * (1 + v % 2)            # the same neighbour two or three times
        if v % 4 == 1:
            row.insert(rng.randint(0, len(row) + 1), -1)
        col += row
        indptr.append(len(col))
    return np.array(indptr, dtype=np.int64), np.array(col, dtype=np.int32)


@EIDS
@pytest.mark.parametrize("fanout", [[8], [5, 4]])
def test_parallel_edges_dead_columns_and_zero_rows(hip, fanout, edge_ids):
    indptr, col = _hand_built_csr()
    assert (col < 0).sum() >= 5
    wl = Workload(dim=4, indptr=indptr, col=col, n_seeds=24, n_valid=8, n_test=8)
    w = ref.hash_weights(wl.E, seed=8)
    zero_rows = [v for v in range(wl.N) if v % 5 == 2 and indptr[v + 1] > indptr[v]]
    w[col < 0] = 2.0                                  # dead entries keep a weight: drawn, and then no edge
    for v in zero_rows:
        w[indptr[v]:indptr[v + 1]] = 0
    batch = 24
    gpu = _weighted(wl, batch, fanout, w, edge_ids)
    table = _table_of(gpu, wl, w)
    got = gpu.run(0, 0, 0)
    _check(got, _want(wl, table, 0, 0, batch, fanout), wl, w, f"{fanout}: ", edge_ids)
    assert zero_rows and not np.isin(got["agg_dst_ids"], zero_rows).any()         # an all-zero row yields no edge
    assert np.isin(wl.sets[(0, 0)][0][:batch], zero_rows).any()                   # ... though such rows were sampled for
    assert gpu.pools[0].error() == 0
    gpu.close()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------
def test_switch_default_and_refusals(hip):
    from legion_amd import engine
    wl = Workload(scale=10, edge_factor=8, dim=4, n_seeds=200)
    fanout, batch = [4, 2], 32
    gpu = GpuSide(wl, batch, fanout)
    pool = gpu.pools[0]
    L = pool._lib
    assert pool.weighted is False and int(L.legion_pool_sample_weighted(pool.handle)) == 0      # off by default
    assert L.legion_pool_set_sample_weighted(pool.handle, 2) == -1 and L.legion_pool_set_sample_weighted(pool.handle, -1) == -1
    # weighted and replace=False, in both orders
    pool.set_replace(False)
    with pytest.raises(RuntimeError):
        pool.set_weighted(True)
    assert pool.weighted is False
    pool.set_replace(True)
    pool.set_weighted(True)
    with pytest.raises(RuntimeError):
        pool.set_replace(False)
    assert pool.replace is True and pool.weighted is True
    with pytest.raises(RuntimeError):
        engine.MemoryPool(0, wl.N, batch, fanout, wl.D, replace=False, weighted=True)
    # a weighted hop against a graph without a table: error bit 8, buffers untouched, and the mode is still free
    pool.buffer("edge_counter").fill_(-5)
    pool.buffer("sampled_ids").fill_(-9)
    engine.enqueue_batch(None, gpu.graph, gpu.feature, gpu.cache, pool, batch, 0, 0, 0, False, fanout)
    torch.cuda.synchronize()
    assert pool.error() & 8
    assert bool((pool.buffer("edge_counter") == -5).all()) and bool((pool.buffer("sampled_ids") == -9).all())
    pool.set_weighted(False)
    off = gpu.run(0, 0, 0)
    with pytest.raises(RuntimeError):
        pool.set_weighted(True)                         # refused after the first sampled hop
    with pytest.raises(RuntimeError):
        pool.set_weighted(False)                        # (whatever the value: the mode is fixed)
    # weights may be set and replaced while no weighted hop has run against the graph -- an unweighted batch is not one
    gpu.graph.set_edge_weights(np.ones(wl.E, np.float32))
    w = ref.hash_weights(wl.E, seed=3)
    gpu.graph.set_edge_weights(torch.from_numpy(w))
    assert L.legion_graph_set_edge_weights(gpu.graph.handle, None, None) == -1
    table = _table_of(gpu, wl, w)
    on = engine.MemoryPool(0, wl.N, batch, fanout, wl.D, weighted=True)
    on.alloc_features(on.num_ids)
    on.set_weighted(False)
    on.set_weighted(True)                               # free to change before the first hop
    engine.enqueue_batch(None, gpu.graph, gpu.feature, gpu.cache, on, batch, 0, 0, 0, False, fanout)
    torch.cuda.synchronize()
    got = engine.read_batch(on)
    _check(got, _want(wl, table, 0, 0, batch, fanout), wl, w, "on: ", False)
    assert not np.array_equal(got["agg_src_ids"], off["agg_src_ids"])
    with pytest.raises(RuntimeError):
        on.set_weighted(False)
    with pytest.raises(RuntimeError):
        gpu.graph.set_edge_weights(w)                   # refused once a weighted hop has been enqueued
    assert np.array_equal(gpu.graph.edge_cdf().cpu().numpy().view(np.uint32), table.view(np.uint32))
    again = gpu.run(0, 0, 0)                            # the unweighted pool of the same graph is not touched by any of this
    for k in KEYS_EXACT:
        assert np.array_equal(again[k], off[k]), k
    assert on.error() == 0
    on.close()
    gpu.close()


def test_pipeline_refusals(hip):
    from legion_amd import engine
    wl = Workload(scale=10, edge_factor=8, dim=4, n_seeds=200)
    fanout, batch = [4, 2], 32
    gpu = GpuSide(wl, batch, fanout)
    gpu.graph.set_edge_weights(np.ones(wl.E, np.float32))
    torch.cuda.synchronize()                            # (the pipeline samples on streams of its own)
    with pytest.raises(RuntimeError):
        engine.Pipeline(gpu.graph, gpu.feature, gpu.cache, 0, batch, fanout, 2, gpu.pools[0].num_ids, False, 2, replace=False, weighted=True)
    pipe = engine.Pipeline(gpu.graph, gpu.feature, gpu.cache, 0, batch, fanout, 2, gpu.pools[0].num_ids, False, 2, weighted=True)
    with pytest.raises(RuntimeError):
        pipe.set_replace(False)                         # the other order
    assert pipe.weighted is True and all(pl.replace for lanes in pipe.pools for pl in lanes)
    assert pipe._lib.legion_pipeline_set_sample_weighted(pipe.handle, 3) == -1
    pipe.set_weighted(False)
    pipe.set_weighted(True)
    pipe.wait(pipe.submit(0, 0))
    with pytest.raises(RuntimeError):
        pipe.set_weighted(False)                        # refused after the first submit
    assert all(pool.error() == 0 for lanes in pipe.pools for pool in lanes)
    pipe.close()
    gpu.close()


def test_group_lanes_share_one_mode_and_need_a_table(hip):
    """A group whose lanes disagree on the mode, and a weighted group against a graph without a table, are refused: nothing is
    sampled, LG_ERR_SAMPLE_MODE = 8."""
    from legion_amd import engine, lib
    L = lib.load()
    wl = Workload(scale=10, edge_factor=8, dim=4, n_seeds=200)
    fanout, batch = [4, 2], 32
    gpu = GpuSide(wl, batch, fanout)
    fo = (ctypes.c_int32 * 2)(*fanout)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def refused(pools):
        for pl in pools:
            pl.alloc_features(pl.num_ids)
            pl.buffer("edge_counter").fill_(-5)
        grp = L.legion_group_create((ctypes.c_void_p * 2)(*[pl.handle for pl in pools]), 2)
        L.legion_enqueue_group(s, gpu.graph.handle, gpu.feature.handle, gpu.cache.handle, grp, batch, 0, 0, 0, fo, 2)
        torch.cuda.synchronize()
        assert all(pl.error() & 8 for pl in pools)
        assert all(bool((pl.buffer("edge_counter") == -5).all()) for pl in pools)        # nothing was sampled
        L.legion_group_destroy(grp)
        for pl in pools:
            pl.close()

    refused([engine.MemoryPool(0, wl.N, batch, fanout, wl.D, weighted=True) for _ in range(2)])      # no table yet
    gpu.graph.set_edge_weights(np.ones(wl.E, np.float32))
    refused([engine.MemoryPool(0, wl.N, batch, fanout, wl.D, weighted=(i == 1)) for i in range(2)])   # lanes disagree
    gpu.graph.set_edge_weights(np.ones(wl.E, np.float32))        # (neither attempt enqueued a weighted hop: the table is still free)
    gpu.close()


# ---- 8. a seeded fuzz -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(20))
def test_fuzz(hip, seed):
    rng = np.random.RandomState(1000 + seed)
    n = int(rng.randint(30, 400))
    deg = np.minimum(rng.geometric(0.15, n) - 1, 60).astype(np.int64)
    deg[rng.randint(0, n, 2)] = rng.randint(100, 700, 2)                          # a few long rows
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    E = int(indptr[-1])
    col = rng.randint(0, n, E).astype(np.int32)
    col[rng.rand(E) < 0.03] = -1
    w = (rng.randint(0, 40, E) / 8).astype(np.float32)
    odd = rng.rand(E) < 0.2
    w[odd] = rng.choice(np.array([0.0, -1.0, np.nan, np.inf, -0.0], dtype=np.float32), int(odd.sum()))
    for v in rng.randint(0, n, 3):
        w[indptr[v]:indptr[v + 1]] = 0
    hops = int(rng.randint(1, 4))
    fanout = [int(f) for f in rng.randint(1, 9, hops)]
    edge_ids = bool(rng.randint(0, 2))
    n_seeds = int(rng.randint(8, max(n // 2, 9)))
    wl = Workload(dim=4, indptr=indptr, col=col, n_seeds=n_seeds, n_valid=4, n_test=4)
    batch = int(rng.randint(4, n_seeds + 1))
    gpu = _weighted(wl, batch, fanout, w, edge_ids)
    table = _table_of(gpu, wl, w)
    n_train = (wl.sets[(0, 0)][0].size + batch - 1) // batch
    ctx = f"seed {seed} (N {n}, E {E}, batch {batch}, fanout {fanout}, edge_ids {edge_ids}) "
    for it in sorted({0, n_train - 1}):
        _check(gpu.run(0, it, 0), _want(wl, table, it, 0, batch, fanout), wl, w, ctx + f"batch {it}: ", edge_ids)
    assert gpu.pools[0].error() == 0
    gpu.close()
