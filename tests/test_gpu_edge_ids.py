"""The edge-id mode on the GPU (MemoryPool / Pipeline edge_ids=True): agg_edge_ids bit for bit against the numpy restatement in
tests/edge_ids_ref.py, in both sampling modes and every sampler class, and everything else a batch holds bit for bit what it is
with the mode off (the existing oracle with replacement, tests/distinct_ref.py without)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import distinct_ref
from tests import edge_ids_ref as ref
from tests.gpu_harness import CpuSide, GpuSide
from tests.helpers import KEYS_EXACT, Workload, compare_batches

pytestmark = pytest.mark.gpu

BOTH = pytest.mark.parametrize("replace", [True, False], ids=["replace", "distinct"])


def _on(gpu, replace):
    for pool in gpu.pools:
        pool.set_replace(replace)
        pool.set_edge_ids(True)
        assert pool.edge_ids is True and pool.replace is replace
    return gpu


def _want(wl, it, mode, batch, fanout, replace):
    ids, labels = wl.sets[(0, mode)]
    return ref.run_batch(wl.indptr, wl.col, ids, labels, batch, it, fanout, replace)


def _check(got, want, wl, ctx):
    """The edge ids are the helper's and obey the contract; every other key and the gathered rows are the helper's too."""
    assert "agg_edge_ids" in got, f"{ctx}no agg_edge_ids"
    assert got["agg_edge_ids"].dtype == np.int64
    compare_batches(got, want, ctx)
    assert np.array_equal(got["agg_edge_ids"], want["agg_edge_ids"]), f"{ctx}agg_edge_ids"
    ref.check_edge_ids(wl.indptr, wl.col, got)
    if "float_features" in got and wl.D > 0:
        rows = got["float_features"][:want["sampled_ids"].size]
        assert np.array_equal(rows.view(np.uint32), wl.features[want["sampled_ids"]].view(np.uint32)), f"{ctx}gathered rows"


# ---- 1. exact, and nothing else changes ---------------------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("fanout", [[25, 10], [3], [2, 2, 2], [40, 3], [2, 2, 2, 2, 2, 2]])
def test_exact_and_invariant(hip, fanout, replace):
    wl = Workload(scale=11, edge_factor=8, dim=16, n_seeds=700)
    batch = 64
    gpu = _on(GpuSide(wl, batch, fanout), replace)
    cpu = CpuSide(wl, batch, fanout) if replace else None            # the existing oracle: the mode changes nothing it computes
    n_train = (wl.sets[(0, 0)][0].size + batch - 1) // batch          # the last batch is clamped
    for it, mode in [(0, 0), (1, 0), (2, 0), (n_train - 1, 0), (0, 1), (0, 2)]:
        ctx = f"{fanout} mode {mode} batch {it}: "
        got = gpu.run(0, it, mode)
        _check(got, _want(wl, it, mode, batch, fanout, replace), wl, ctx)
        if replace:
            compare_batches(got, cpu.run(0, it, mode), ctx + "oracle: ")
        else:
            ids, labels = wl.sets[(0, mode)]
            compare_batches(got, distinct_ref.run_batch(wl.indptr, wl.col, ids, labels, batch, it, fanout), ctx + "distinct_ref: ")
    assert gpu.pools[0].error() == 0
    gpu.close()
    if cpu:
        cpu.close()


# ---- 2. parallel edges and dead column entries --------------------------------------------------------------------------
def _hand_built_csr(n=40, seed=5):
    """A few dozen vertices of degree 0..7; rows list a neighbour two or three times, and some column entries are -1."""
    rng = np.random.RandomState(seed)
    indptr, col = [0], []
    for v in range(n):
        row = rng.randint(0, n, rng.randint(0, 5)).tolist()
        if v % 3 == 0 and row:
            row += [row[0]] * (1 + v % 2)            # the same neighbour two or three times
        if v % 4 == 1:
            row.insert(rng.randint(0, len(row) + 1), -1)
        col += row
        indptr.append(len(col))
    return np.array(indptr, dtype=np.int64), np.array(col, dtype=np.int32)


@pytest.mark.parametrize("fanout", [[8], [8, 8]])
def test_parallel_edges_and_dead_columns(hip, fanout):
    indptr, col = _hand_built_csr()
    assert (col < 0).sum() >= 5 and int(np.diff(indptr).max()) <= 8
    wl = Workload(dim=4, indptr=indptr, col=col, n_seeds=24, n_valid=8, n_test=8)
    batch = 24
    gpu = _on(GpuSide(wl, batch, fanout), False)
    got = gpu.run(0, 0, 0)
    _check(got, _want(wl, 0, 0, batch, fanout, False), wl, f"{fanout}: ")
    # f >= D everywhere: every frontier entry lists its row's live entries, in CSR order
    ec, lo, frontier = got["edge_counter"], 0, got["sampled_ids"][:batch]
    for h in range(len(fanout)):
        hi = int(ec[9 + h + 1])
        want = [e for s in frontier.tolist() for e in range(int(indptr[s]), int(indptr[s + 1])) if col[e] >= 0]
        assert got["agg_edge_ids"][lo:hi].tolist() == want, f"hop {h}"
        frontier, lo = got["agg_src_ids"][lo:hi], hi
    n0 = int(ec[10])                                 # hop 1: the seeds are distinct, so a repeated (vertex, neighbour) pair is one row's
    pairs = got["agg_dst_ids"][:n0].astype(np.int64) * wl.N + got["agg_src_ids"][:n0]
    _, inv, cnt = np.unique(pairs, return_inverse=True, return_counts=True)
    assert cnt.max() >= 2                            # parallel edges were sampled ...
    for g in np.nonzero(cnt > 1)[0]:                 # ... and each got an id of its own
        assert np.unique(got["agg_edge_ids"][:n0][inv == g]).size == cnt[g]
    # with replacement on the same graph: dead entries yield no edge and no id
    gpu2 = _on(GpuSide(wl, batch, [3, 2]), True)
    _check(gpu2.run(0, 0, 0), _want(wl, 0, 0, batch, [3, 2], True), wl, "with replacement: ")
    assert gpu.pools[0].error() == 0 and gpu2.pools[0].error() == 0
    gpu2.close()
    gpu.close()


# ---- 3. rows served from the cached topology ----------------------------------------------------------------------------
@BOTH
def test_cached_topology_keeps_full_csr_positions(hip, col_slots, replace):
    wl = Workload(scale=11, edge_factor=8, dim=32, n_seeds=700)
    fanout, batch = [6, 3], 64
    gpu = _on(GpuSide(wl, batch, fanout), replace)
    steps = (wl.sets[(0, 0)][0].size - 1) // batch
    for it in range(steps):
        gpu.run(0, it, 0, is_presc=True)
    gpu.cache.candidate_selection(0, gpu.graph)
    gpu.cache.set_capacity(150, 80)                     # rows served from the cached topology and the full CSR
    gpu.cache.fill_up(gpu.feature, gpu.graph)
    topo = 0
    for it in range(3):
        got = gpu.run(0, it, 0)
        want = _want(wl, it, 0, batch, fanout, replace)
        _check(got, want, wl, f"cached topology {it}: ")
        ec = want["edge_counter"]
        tp = gpu.pools[0].buffer("tmp_part_ind")[:int(ec[10] - ec[9])].cpu().numpy()      # the last hop's frontier
        topo += int((tp >= 0).sum())
    assert topo > 0                                     # some rows did come from the cached topology
    assert gpu.graph.column_slots(0) == col_slots
    assert gpu.pools[0].error() == 0
    gpu.close()


# ---- 4. every bucket class and its overflow paths -----------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("buckets,claim_cap", [("8", "1"), ("8", "40"), ("8", None), ("16", "1"), ("16", "40"), ("16", None)])
def test_small_classes_with_claim_list_overflow(hip, monkeypatch, buckets, claim_cap, replace):
    monkeypatch.setenv("LEGION_LDS_SMALL_BUCKETS", buckets)
    if claim_cap is not None:
        monkeypatch.setenv("LEGION_LDS_CLAIM_CAP", claim_cap)
    wl = Workload(scale=12, edge_factor=8, dim=4, n_seeds=600)
    fanout, batch = [4, 3, 3], 48
    gpu = _on(GpuSide(wl, batch, fanout), replace)
    assert gpu.pools[0].lds_buckets() == int(buckets)
    for it in range(3):
        _check(gpu.run(0, it, 0), _want(wl, it, 0, batch, fanout, replace), wl, f"{buckets} buckets cap {claim_cap} batch {it}: ")
    assert gpu.pools[0].error() == 0
    gpu.close()


@pytest.fixture(scope="module")
def large_wl():
    return Workload(scale=15, edge_factor=16, dim=4, n_seeds=13000)


@BOTH
@pytest.mark.parametrize("fanout,n_buckets", [([10, 10], 64), ([10, 10, 8], 256)], ids=["64buckets", "256buckets"])
def test_large_classes(hip, large_wl, fanout, n_buckets, replace):
    wl, batch = large_wl, 6000
    gpu = _on(GpuSide(wl, batch, fanout), replace)
    assert gpu.pools[0].lds_buckets() == n_buckets
    _check(gpu.run(0, 1, 0), _want(wl, 1, 0, batch, fanout, replace), wl, f"{batch} {fanout}: ")
    assert gpu.pools[0].error() == 0
    gpu.close()


# ---- 5. lane groups, graph replay, the weave ----------------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("group,slots,use_graph,weave", [(4, 2, True, False), (3, 2, True, True), (2, 2, False, False)])
def test_pipeline_graph_replay_and_weave(hip, group, slots, use_graph, weave, replace):
    from legion_amd import engine
    wl = Workload(scale=11, edge_factor=8, dim=32, n_seeds=700)
    fanout, batch = [6, 3], 64
    gpu = GpuSide(wl, batch, fanout)
    gpu.cache.candidate_selection(0, gpu.graph)
    gpu.cache.set_capacity(150, 80)
    gpu.cache.fill_up(gpu.feature, gpu.graph)
    pipe = engine.Pipeline(gpu.graph, gpu.feature, gpu.cache, 0, batch, fanout, group, gpu.pools[0].num_ids, use_graph, slots,
                           weave=weave, replace=replace, edge_ids=True)
    assert pipe.edge_ids is True
    n_batches = (wl.sets[(0, 0)][0].size + batch - 1) // batch
    n_groups = min((n_batches + group - 1) // group, 2 * slots)          # two passes over the slots: every graph is replayed
    want = {}
    for gi in range(n_groups):
        sl = pipe.submit(gi * group, 0)
        pipe.wait(sl)
        for lane in range(group):
            b = gi * group + lane
            want[b] = _want(wl, b, 0, batch, fanout, replace)
            _check(engine.read_batch(pipe.pools[sl][lane]), want[b], wl, f"group {gi} lane {lane}: ")
    with pytest.raises(RuntimeError):
        pipe.set_edge_ids(False)                        # the captured graphs never mix modes
    assert all(pool.error() == 0 for lanes in pipe.pools for pool in lanes)
    pipe.close()
    gpu.close()


# ---- 6. the switch ------------------------------------------------------------------------------------------------------
def test_switch_default_and_refusals(hip):
    from legion_amd import engine
    wl = Workload(scale=10, edge_factor=8, dim=4, n_seeds=200)
    gpu = GpuSide(wl, 32, [4, 2])
    pool = gpu.pools[0]
    assert pool.edge_ids is False and int(pool._lib.legion_pool_edge_ids(pool.handle)) == 0      # off by default
    with pytest.raises(RuntimeError):
        pool.buffer("agg_edge_ids")
    assert not pool._lib.legion_pool_buffer(pool.handle, 14)
    assert pool._lib.legion_pool_set_edge_ids(pool.handle, 2) == -1
    off = gpu.run(0, 0, 0)
    assert "agg_edge_ids" not in off
    with pytest.raises(RuntimeError):
        pool.set_edge_ids(True)                         # refused after the first sampled hop
    assert pool.edge_ids is False
    with pytest.raises(RuntimeError):
        pool.set_edge_ids(False)                        # (whatever the value: the mode is fixed)
    with pytest.raises(RuntimeError):
        pool.buffer("agg_edge_ids")
    on = engine.MemoryPool(0, wl.N, 32, [4, 2], wl.D, edge_ids=True)
    on.alloc_features(on.num_ids)
    on.set_edge_ids(False)
    on.set_edge_ids(True)                               # free to change before the first hop
    t = on.buffer("agg_edge_ids")
    assert t.dtype == torch.int64 and t.shape == (on.num_ids,)
    engine.enqueue_batch(None, gpu.graph, gpu.feature, gpu.cache, on, 32, 0, 0, 0, False, [4, 2])
    torch.cuda.synchronize()
    got = engine.read_batch(on)
    for k in KEYS_EXACT:                                # the mode changes nothing else
        assert np.array_equal(got[k], off[k]), k
    assert np.array_equal(got["float_features"], off["float_features"])
    _check(got, _want(wl, 0, 0, 32, [4, 2], True), wl, "on: ")
    with pytest.raises(RuntimeError):
        on.set_edge_ids(False)
    assert on.edge_ids is True
    on.close()
    gpu.close()


def test_group_lanes_share_one_mode(hip):
    """A group whose lanes disagree on the mode is refused (nothing sampled, LG_ERR_SAMPLE_MODE = 8); a group that was made before
    its lanes took the mode still writes every lane's ids."""
    from legion_amd import engine, lib
    L = lib.load()
    wl = Workload(scale=10, edge_factor=8, dim=4, n_seeds=200)
    fanout, batch = [4, 2], 32
    gpu = GpuSide(wl, batch, fanout)
    fo = (ctypes.c_int32 * 2)(*fanout)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def group_of(pools):
        for pl in pools:
            pl.alloc_features(pl.num_ids)
        return L.legion_group_create((ctypes.c_void_p * 2)(*[pl.handle for pl in pools]), 2)

    pools = [engine.MemoryPool(0, wl.N, batch, fanout, wl.D) for _ in range(2)]
    grp = group_of(pools)
    pools[1].set_edge_ids(True)                          # lanes disagree: refused
    for pl in pools:
        pl.buffer("edge_counter").fill_(-5)
    L.legion_enqueue_group(s, gpu.graph.handle, gpu.feature.handle, gpu.cache.handle, grp, batch, 0, 0, 0, fo, 2)
    torch.cuda.synchronize()
    assert all(pl.error() & 8 for pl in pools)
    assert all(bool((pl.buffer("edge_counter") == -5).all()) for pl in pools)        # nothing was sampled
    L.legion_group_destroy(grp)
    for pl in pools:
        pl.close()

    pools = [engine.MemoryPool(0, wl.N, batch, fanout, wl.D) for _ in range(2)]
    grp = group_of(pools)
    for pl in pools:
        pl.set_edge_ids(True)                            # after the group was made
    L.legion_enqueue_group(s, gpu.graph.handle, gpu.feature.handle, gpu.cache.handle, grp, batch, 0, 0, 0, fo, 2)
    torch.cuda.synchronize()
    for lane, pl in enumerate(pools):
        assert pl.error() == 0
        _check(engine.read_batch(pl), _want(wl, lane, 0, batch, fanout, True), wl, f"group lane {lane}: ")
        with pytest.raises(RuntimeError):
            pl.set_edge_ids(False)                       # lane 1 as well as lane 0
    L.legion_group_destroy(grp)
    for pl in pools:
        pl.close()
    gpu.close()
