"""The cache set-up chain (kernels_cache.hip: the row headers, the hotness count and the find included) past every capped grid, against the C oracle and the numpy
statements of tests/setup_ref.py, integer for integer and bit for bit.

One world: N = 2^20 + 2^16 + 777 vertices of degree 2 and 3 alternating (E about 2.8 M: the later rows' edges lie past the 2 097 152 of one
column-slot pass), a few dead columns, two logical GPUs as one clique.  The access counters are written directly -- heavy-tailed, mostly
zero, different for the two members -- so the chain runs from known inputs; only the hotness case presamples.

    aggregate_access, iota, sort, the scans, edge_mem, fill_kernel, init_row_hdr              N > 4096 x 256
    init_node_map / init_edge_maps                                                            cap * Kg = 1 114 000, between 2^20 and N
    feat_fill_up, feat_fill_up_bf16, topo_fill_up                                             557 000 cached rows > 8192 x 4 waves
    convert_f32_to_bf16                                                                       N rows of pitch 32: 4.46 M chunks > 16384 x 256
    build_column_slots                                                                        E > 8192 x 256, read by the served batches
    topo_neighbor_count, cache_row_hdr                                                        ONE member's capacity > 4096 x 256: the cliques
                                                                                              of one with capacity 1 100 000 (below)
    find_kernel                                                                               N keys > 2048 x 256
    hotness_measure                                                                           one op of more than 1024 x 256 ids

topo_neighbor_count and cache_row_hdr run over one member's capacity, not over N or cap * Kg: with 557 000 rows a member their grids make
one pass.  test_cliques_of_one_with_a_capacity_past_one_pass gives every member 1 100 000 rows (Kg = 1), compares the whole cached CSR
(the neighbour counts) and serves batches whose rows sit at cached offsets at or above 2^20 (the cached row headers).
The oracle defines capacities with cap * Kg > N (ranks at or beyond N are skipped), so that case is here too."""
import numpy as np
import pytest
import torch

from legion_amd import engine
from oracle import ffi
from tests import setup_ref as ref
from tests.gpu_harness import CpuSide, GpuSide
from tests.helpers import Workload, compare_batches
from tests.mode_ref import bf16_bits, rounded

DEV = "cuda:0"
N = (1 << 20) + (1 << 16) + 777
P = KG = 2
CAP = 557_000
CAP_BEYOND = 600_000
CAP_ONE = 1_100_000                              # one member's capacity in a clique of one: what topo_neighbor_count and cache_row_hdr run over
HYBRID = (500_000, 600_000)                      # (cpu_cap, gpu_cap)
N_SEEDS = 400_000
SERVE_BATCH, SERVE_FANOUT = 4096, [3, 2]
PRESC_BATCH, PRESC_FANOUT = 150_000, [3]
BUDGETS = [4_000_000, 12_000_000]                # cache bytes per GPU: below and above what the whole feature table takes
PEER_MAX_IDS, TRAIN_STEP, COUNTERS = [300_000, 250_000], 5, (123_456, 7_890)
FILLS = [("float32", 4, CAP), ("float32", 7, CAP), ("bfloat16", 25, CAP), ("float32", 4, CAP_BEYOND)]
FILL_IDS = ["f32-D4", "f32-D7", "bf16-D25", "f32-D4-beyond-N"]


# ---- the world and the reference side -------------------------------------------------------------------------------------------------
def _csr():
    rng = np.random.RandomState(29)
    deg = 2 + (np.arange(N, dtype=np.int64) & 1)
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    E = int(indptr[-1])
    col = rng.randint(0, N, E).astype(np.int32)
    col[rng.randint(0, E, 200)] = -1
    col[rng.randint(int(indptr[N - 800]), E, 60)] = -1          # the coldest vertices' rows: served from the full CSR
    return indptr, col


def _counters():
    rng = np.random.RandomState(31)
    out = [np.floor(rng.pareto(1.1, N) * 0.35).astype(np.uint64) for _ in range(4)]
    for a in out:
        a[rng.randint(0, N, 500)] = rng.randint(1 << 20, 1 << 40, 500).astype(np.uint64)
    return out[:2], out[2:]


class World:
    def __init__(self):
        self.indptr, self.col = _csr()
        self.E = int(self.col.size)
        self.na, self.ea = _counters()
        self._wl = {}
        self.QF, self.AF = ref.hotness_order(self.na)
        self.QT, self.AT = ref.hotness_order(self.ea)

    def workload(self, D):
        if D not in self._wl:
            self._wl[D] = Workload(dim=D, n_seeds=N_SEEDS, partition_count=P, indptr=self.indptr, col=self.col)
        return self._wl[D]

    def oracle_cache(self, D):
        """A fresh OracleCache of the clique after candidate selection over the written counters."""
        oc = ffi.OracleCache(N, D, KG, 0)
        oc.candidate_selection(self.na, self.ea)
        return oc

    def gpu(self, D, batch, fanout, feature_dtype="float32", cache_memory=0):
        wl = self.workload(D)
        gpu = GpuSide(wl, batch, fanout, cache_memory=cache_memory, feature_dtype=feature_dtype)
        for p in range(P):
            gpu.cache.array("node_access_time", p).copy_(torch.from_numpy(self.na[p].view(np.int64)).to(DEV))
            gpu.cache.array("edge_access_time", p).copy_(torch.from_numpy(self.ea[p].view(np.int64)).to(DEV))
        torch.cuda.synchronize()
        return gpu, wl

    def cpu(self, wl, batch, fanout):
        cpu = CpuSide(wl, batch, fanout)
        for p in range(P):
            cpu.node_access[p][:] = self.na[p]
            cpu.edge_access[p][:] = self.ea[p]
        return cpu


@pytest.fixture(scope="module")
def world():
    return World()


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype}{got.shape} != {want.dtype}{want.shape}"
    if not np.array_equal(got, want):
        bad = np.nonzero((got != want).reshape(got.shape[0], -1).any(axis=1))[0]
        raise AssertionError(f"{what}: {bad.size} entries differ, first at {bad[:5]}: got {got[bad[:3]]} want {want[bad[:3]]}")


def test_inputs_cross_every_cap(world):
    """From the reference side alone, before any launch."""
    assert N > ref.PASS_ELEMENTWISE and N > ref.PASS_FIND
    assert world.E > ref.PASS_COLUMN_SLOTS and world.indptr[N - 900] > ref.PASS_COLUMN_SLOTS
    dead = np.nonzero(world.col < 0)[0]
    assert 100 < dead.size < 300 and dead.min() < ref.PASS_COLUMN_SLOTS < dead.max()
    assert set(np.diff(world.indptr).tolist()) == {2, 3}
    assert (1 << 20) == ref.PASS_ELEMENTWISE < CAP * KG < N < CAP_BEYOND * KG and CAP > ref.PASS_ROW_WAVES
    assert ref.PASS_ELEMENTWISE < sum(HYBRID) < N and min(HYBRID) > ref.PASS_ROW_WAVES
    # the kernels that run over ONE member's capacity make a single pass at CAP, and more than one only in the cliques of one
    assert CAP < CAP_BEYOND < ref.PASS_ELEMENTWISE < CAP_ONE < N
    for p in range(P):
        QT, _ = ref.hotness_order([world.ea[p]])
        counts = np.diff(world.indptr)[QT[ref.PASS_ELEMENTWISE:CAP_ONE]]
        assert set(counts.tolist()) == {2, 3}, "the second pass of the neighbour counts is not all one value"
    assert engine.bf16_pitch(25) == 32 and N * (32 // 8) > ref.PASS_BF16_CHUNKS
    assert [d % 4 == 0 for _, d, _ in FILLS[:3]] == [True, False, False]
    assert PRESC_BATCH * (1 + PRESC_FANOUT[0]) > ref.PASS_HOTNESS and N_SEEDS // P > PRESC_BATCH
    for a, b in ((world.na[0], world.na[1]), (world.ea[0], world.ea[1]), (world.na[0], world.ea[0])):
        assert (a == 0).mean() > 0.6 and (b == 0).mean() > 0.6 and (a != b).mean() > 0.2
    assert np.unique(world.AF).size > 200 and (world.AF == 0).sum() > N // 3            # ties: the stable order decides most of QF
    # a set-up that stopped after one pass, or that dropped the `% Kg` term, is another map
    nmap = ref.node_map(world.QF, N, CAP, KG)
    assert (nmap[world.QF[ref.PASS_ELEMENTWISE:CAP * KG]] >= 0).all() and (nmap[world.QF[CAP * KG:]] == ref.MISS).all()
    assert (nmap[world.QF[1:CAP * KG:2]] >= CAP).all() and (nmap[world.QF[0:CAP * KG:2]] < CAP).all()


def test_numpy_statements_equal_the_oracle_at_this_size(world, oracle):
    oc = world.oracle_cache(4)
    for name, want, dtype in (("QF", world.QF, np.int32), ("QT", world.QT, np.int32), ("AF", world.AF, np.uint64), ("AT", world.AT, np.uint64)):
        _same(oc.arr(name, dtype), want, name)
    wl = world.workload(4)
    for cap in (CAP, CAP_BEYOND):
        oc.set_capacity(cap, cap)
        oc.fill_up(wl.features, world.indptr, world.col)
        _same(oc.arr("node_map", np.int32), ref.node_map(world.QF, N, cap, KG), "node_map")
        index_map, offset_map = ref.edge_maps(world.QT, N, cap, KG, 0)
        _same(oc.arr("edge_index_map", np.int8), index_map, "edge_index_map")
        _same(oc.arr("edge_offset_map", np.int32), offset_map, "edge_offset_map")
        c = oc.c.contents
        for j in range(KG):
            rows, r = ref.cached_rows(wl.features, world.QF, cap, KG, j)
            got = np.ctypeslib.as_array(c.feat_cache[j], shape=(cap, 4))
            _same(got[r].view(np.uint32), rows.view(np.uint32), f"member {j} rows")
            index, dst = ref.cached_csr(world.indptr, world.col, world.QT, cap, KG, j)
            _same(np.ctypeslib.as_array(c.topo_indptr[j], shape=(cap + 1,)), index, f"member {j} cached index")
            _same(np.ctypeslib.as_array(c.topo_col[j], shape=(int(index[-1]),)), dst, f"member {j} cached columns")
    oc.close()


# ---- the device ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_candidate_selection_one_clique_of_two(hip, world):
    gpu, wl = world.gpu(4, 8, [2])
    try:
        gpu.cache.candidate_selection(1, gpu.graph)
        torch.cuda.synchronize()
        assert gpu.cache.hotness_reduce_path(0) == "p2p"
        oc = world.oracle_cache(4)
        for p in range(P):
            for name, want, dtype in (("QF", world.QF, np.int32), ("QT", world.QT, np.int32), ("AF", world.AF, np.uint64),
                                      ("AT", world.AT, np.uint64)):
                got = gpu.cache.array(name, p).cpu().numpy().view(dtype)
                _same(got, want, f"gpu {p} {name} against numpy")
                _same(got, oc.arr(name, dtype), f"gpu {p} {name} against the oracle")
            _same(gpu.cache.array("node_access_time", p).cpu().numpy().view(np.uint64), world.na[p], "the counters survive")
        oc.close()
    finally:
        gpu.close()


@pytest.mark.gpu
def test_cost_model_two_budgets(hip, world):
    split = []
    for cache_memory in BUDGETS:
        gpu, wl = world.gpu(4, 8, [2], cache_memory=cache_memory)
        try:
            gpu.cache.set_peer_max_ids(PEER_MAX_IDS)
            gpu.cache.candidate_selection(1, gpu.graph)
            gpu.cache.cost_model(gpu.feature, gpu.graph, COUNTERS, TRAIN_STEP)
            oc = world.oracle_cache(4)
            alpha, _ = oc.cost_model(cache_memory, world.indptr, COUNTERS, PEER_MAX_IDS, TRAIN_STEP)
            want = (oc.node_capacity, oc.edge_capacity)
            oc.close()
            print(f"cache_memory {cache_memory}: oracle alpha {alpha} capacities {want}")
            assert min(want) > 1
            for p in range(P):
                assert (gpu.cache.node_capacity(p), gpu.cache.edge_capacity(p)) == want
            split.append((alpha, want))
        finally:
            gpu.close()
    assert split[0][0] != split[1][0] and split[0][1][0] != split[1][1][0] and split[0][1][1] != split[1][1][1], "the two budgets split differently"


def _dense_edge_counters(world):
    """Edge counters that are small and positive everywhere, different for the two members: the saved topology transactions then grow
    step by step up to the last vertex, and with no feature transactions the model gives the topology all it can take."""
    ids = np.arange(N, dtype=np.uint64)
    return [np.uint64(1) + (ids * np.uint64(2654435761) + np.uint64(7 * p)) % np.uint64(5) for p in range(P)]


@pytest.mark.gpu
def test_cost_model_split_past_one_pass(hip, world):
    """With the heavy-tailed counters the best split caches a few hundred thousand vertices' adjacency: the model never looks at the prefix
    of edge_mem_in_order beyond rank 2^20.  Here it does: the split point is a lower bound in that prefix past 2^20 ranks."""
    cache_memory, dense = BUDGETS[1], _dense_edge_counters(world)
    oc = ffi.OracleCache(N, 4, KG, 0)
    oc.candidate_selection(world.na, dense)
    oc.cost_model(cache_memory, world.indptr, COUNTERS, [0, 0], TRAIN_STEP)
    want = (oc.node_capacity, oc.edge_capacity)
    QT, _ = ref.hotness_order(dense)
    _same(oc.arr("QT", np.int32), QT, "QT")
    oc.close()
    print(f"dense edge counters, cache_memory {cache_memory}: oracle capacities {want}")
    assert ref.PASS_ELEMENTWISE < (want[1] - 1) * KG < N and want[0] > 1, "from the oracle alone: the topology's share ends past 2^20 ranks"
    gpu, wl = world.gpu(4, 8, [2], cache_memory=cache_memory)
    try:
        for p in range(P):
            gpu.cache.array("edge_access_time", p).copy_(torch.from_numpy(dense[p].view(np.int64)).to(DEV))
        gpu.cache.set_peer_max_ids([0, 0])
        gpu.cache.candidate_selection(1, gpu.graph)
        gpu.cache.cost_model(gpu.feature, gpu.graph, COUNTERS, TRAIN_STEP)
        for p in range(P):
            assert (gpu.cache.node_capacity(p), gpu.cache.edge_capacity(p)) == want
    finally:
        gpu.close()


def _feature_cache(hip, gpu, p, cap, D, dtype):
    ptr = hip.legion_cache_feature_cache(gpu.cache.handle, p)
    assert ptr
    if dtype == "bfloat16":
        return engine.device_view(ptr, (cap, engine.bf16_pitch(D)), torch.int16, torch.device(DEV)).cpu().numpy().view(np.uint16)
    return engine.device_view(ptr, (cap, D), torch.float32, torch.device(DEV)).cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,D,cap", FILLS, ids=FILL_IDS)
def test_fill_maps_rows_and_cached_csr(hip, world, dtype, D, cap):
    gpu, wl = world.gpu(D, 8, [2], feature_dtype=dtype)
    try:
        gpu.cache.candidate_selection(1, gpu.graph)
        gpu.cache.set_capacity(cap, cap)
        gpu.cache.fill_up(gpu.feature, gpu.graph)
        torch.cuda.synchronize()
        served = rounded(wl.features) if dtype == "bfloat16" else wl.features
        oc = world.oracle_cache(D)
        oc.set_capacity(cap, cap)
        oc.fill_up(served, world.indptr, world.col)
        c = oc.c.contents
        nmap = ref.node_map(world.QF, N, cap, KG)
        index_map, offset_map = ref.edge_maps(world.QT, N, cap, KG, 0)
        for p in range(P):
            for name, want, dt in (("node_map", nmap, np.int32), ("edge_index_map", index_map, np.int8), ("edge_offset_map", offset_map, np.int32)):
                got = gpu.cache.array(name, p).cpu().numpy()
                _same(got, want, f"gpu {p} {name} against numpy")
                _same(got, oc.arr(name, dt), f"gpu {p} {name} against the oracle")
            # every cached feature row of this member
            rows, r = ref.cached_rows(wl.features, world.QF, cap, KG, p)
            assert r.size == (cap if cap * KG <= N else len(range(p, N, KG)))
            got = _feature_cache(hip, gpu, p, cap, D, dtype)[r]
            o_rows = np.ctypeslib.as_array(c.feat_cache[p], shape=(cap, D))[r]
            if dtype == "bfloat16":
                want = np.zeros((r.size, engine.bf16_pitch(D)), dtype=np.uint16)
                want[:, :D] = bf16_bits(rows)
                _same(got, want, f"gpu {p} cached bf16 rows against torch's conversion")
                _same((got[:, :D].astype(np.uint32) << 16), o_rows.view(np.uint32), f"gpu {p} cached bf16 rows against the oracle")
            else:
                _same(got.view(np.uint32), rows.view(np.uint32), f"gpu {p} cached rows against numpy")
                _same(got.view(np.uint32), o_rows.view(np.uint32), f"gpu {p} cached rows against the oracle")
            # the whole cached CSR of this member
            index, dst = ref.cached_csr(world.indptr, world.col, world.QT, cap, KG, p)
            g_index, g_dst = gpu.graph.cached_csr(p, cap)
            g_index, g_dst = g_index.cpu().numpy(), g_dst.cpu().numpy()
            _same(g_index, index, f"gpu {p} cached index against numpy")
            _same(g_dst, dst, f"gpu {p} cached columns against numpy")
            _same(g_index, np.ctypeslib.as_array(c.topo_indptr[p], shape=(cap + 1,)), f"gpu {p} cached index against the oracle")
            _same(g_dst, np.ctypeslib.as_array(c.topo_col[p], shape=(int(index[-1]),)), f"gpu {p} cached columns against the oracle")
        oc.close()
    finally:
        gpu.close()


@pytest.mark.gpu
def test_hybrid_tier(hip, world):
    cpu_cap, gpu_cap = HYBRID
    gpu, wl = world.gpu(4, 8, [2])
    try:
        gpu.cache.hybrid_init(gpu.feature, gpu.graph, cpu_cap, gpu_cap)
        torch.cuda.synchronize()
        for p in range(P):
            oc = ffi.OracleCache(N, 4, 1, p)
            oc.hybrid_init(world.na[p], wl.features, cpu_cap, gpu_cap)
            QF, AF = ref.hotness_order([world.na[p]])
            _same(gpu.cache.array("QF", p).cpu().numpy(), QF, f"gpu {p} QF against numpy")
            _same(gpu.cache.array("QF", p).cpu().numpy(), oc.arr("QF", np.int32), f"gpu {p} QF against the oracle")
            _same(gpu.cache.array("AF", p).cpu().numpy().view(np.uint64), AF, f"gpu {p} AF")
            got = gpu.cache.array("node_map", p).cpu().numpy()
            _same(got, ref.hybrid_map(QF, N, cpu_cap, gpu_cap), f"gpu {p} node_map against numpy")
            _same(got, oc.arr("node_map", np.int32), f"gpu {p} node_map against the oracle")
            assert (gpu.cache.array("edge_index_map", p).cpu().numpy() == ref.MISS).all()
            assert (gpu.cache.array("edge_offset_map", p).cpu().numpy() == ref.MISS).all()
            cpu_rows, gpu_rows = gpu.cache.hybrid_caches(p)
            c = oc.c.contents
            _same(gpu_rows.cpu().numpy().view(np.uint32), wl.features[QF[:gpu_cap]].view(np.uint32), f"gpu {p} GPU cache against numpy")
            _same(cpu_rows.cpu().numpy().view(np.uint32), wl.features[QF[gpu_cap:gpu_cap + cpu_cap]].view(np.uint32), f"gpu {p} CPU cache against numpy")
            _same(gpu_rows.cpu().numpy().view(np.uint32), np.ctypeslib.as_array(c.feat_cache[0], shape=(gpu_cap, 4)).view(np.uint32), f"gpu {p} GPU cache against the oracle")
            _same(cpu_rows.cpu().numpy().view(np.uint32), np.ctypeslib.as_array(c.cpu_cache, shape=(cpu_cap, 4)).view(np.uint32), f"gpu {p} CPU cache against the oracle")
            oc.close()
    finally:
        gpu.close()


@pytest.mark.gpu
def test_serving_after_the_fill(hip, world, col_slots):
    """What reads the row headers (both kernels), the column-slot pairs and the maps past their caps."""
    gpu, wl = world.gpu(4, SERVE_BATCH, SERVE_FANOUT)
    cpu = world.cpu(wl, SERVE_BATCH, SERVE_FANOUT)
    try:
        gpu.cache.candidate_selection(1, gpu.graph)
        gpu.cache.set_capacity(CAP, CAP)
        gpu.cache.fill_up(gpu.feature, gpu.graph)
        assert all(gpu.graph.column_slots(p) == col_slots for p in range(P))
        (oc,) = cpu.build_cache(1, capacity=(CAP, CAP))
        o_nmap, o_off = oc.arr("node_map", np.int32), oc.arr("edge_offset_map", np.int32)
        wants = {(p, it): cpu.run(p, it, 0) for p in range(P) for it in range(2)}
        # from the oracle's batches alone
        ids = np.concatenate([w["sampled_ids"] for w in wants.values()])
        seeds = np.concatenate([w["sampled_ids"][:SERVE_BATCH] for w in wants.values()])
        nbrs = np.concatenate([w["agg_src_ids"] for w in wants.values()])
        rows = np.unique(np.concatenate([w["agg_dst_ids"] for w in wants.values()]))
        assert (seeds > (1 << 20)).any() and (nbrs > (1 << 20)).any()
        slots = o_nmap[ids[ids >= 0]]
        assert (slots >= 0).any() and (slots < 0).any() and (slots >= CAP).any()
        assert (world.indptr[rows] > ref.PASS_COLUMN_SLOTS).any()
        full = rows[o_off[rows] == ref.MISS]                    # served from the full CSR: its headers, and the pairs when they are on
        assert (world.indptr[full] > ref.PASS_COLUMN_SLOTS).any() and (o_off[rows] >= ref.PASS_ELEMENTWISE // KG).any()
        assert (full >= ref.PASS_ELEMENTWISE).any(), "a full-CSR header that init_row_hdr wrote in its second pass"
        for (p, it), want in wants.items():
            got = gpu.run(p, it, 0)
            compare_batches(got, want, f"gpu {p} batch {it}: ")
            _same(got["cache_search_buffer"], want["cache_search_buffer"], f"gpu {p} batch {it} cache_search_buffer")
    finally:
        gpu.close(); cpu.close()


@pytest.mark.gpu
def test_cliques_of_one_with_a_capacity_past_one_pass(hip, world, col_slots):
    """topo_neighbor_count and cache_row_hdr run over one member's capacity.  Two cliques of one (Kg = 1), each from its own counters, with
    1 100 000 rows a member: the whole cached CSR is compared (its index is the scan of the neighbour counts, both passes), then batches
    are served whose rows sit at cached offsets at or above 2^20 -- headers that cache_row_hdr wrote in its second pass.  (A header that
    pass mis-computed sends the sampler to another row of the cached CSR and shows in the batch; one it never wrote stays on the full CSR,
    which holds the same adjacency: no result can show that, and the library has no call that reads the headers back.)"""
    gpu, wl = world.gpu(4, SERVE_BATCH, SERVE_FANOUT)
    cpu = world.cpu(wl, SERVE_BATCH, SERVE_FANOUT)
    try:
        gpu.cache.candidate_selection(0, gpu.graph)
        gpu.cache.set_capacity(CAP_ONE, CAP_ONE)
        gpu.cache.fill_up(gpu.feature, gpu.graph)
        torch.cuda.synchronize()
        assert all(gpu.graph.column_slots(p) == col_slots for p in range(P))
        caches = cpu.build_cache(0, capacity=(CAP_ONE, CAP_ONE))
        assert len(caches) == P
        for p, oc in enumerate(caches):
            QF, _ = ref.hotness_order([world.na[p]])
            QT, _ = ref.hotness_order([world.ea[p]])
            _same(gpu.cache.array("QT", p).cpu().numpy(), QT, f"gpu {p} QT against numpy")
            _same(gpu.cache.array("QT", p).cpu().numpy(), oc.arr("QT", np.int32), f"gpu {p} QT against the oracle")
            index_map, offset_map = ref.edge_maps(QT, N, CAP_ONE, 1, p)
            for name, want, dt in (("node_map", ref.node_map(QF, N, CAP_ONE, 1), np.int32), ("edge_index_map", index_map, np.int8),
                                   ("edge_offset_map", offset_map, np.int32)):
                got = gpu.cache.array(name, p).cpu().numpy()
                _same(got, want, f"gpu {p} {name} against numpy")
                _same(got, oc.arr(name, dt), f"gpu {p} {name} against the oracle")
            index, dst = ref.cached_csr(world.indptr, world.col, QT, CAP_ONE, 1, 0)
            assert not np.array_equal(np.diff(index)[:ref.PASS_ELEMENTWISE][:CAP_ONE - ref.PASS_ELEMENTWISE], np.diff(index)[ref.PASS_ELEMENTWISE:])
            g_index, g_dst = gpu.graph.cached_csr(p, CAP_ONE)
            g_index, g_dst = g_index.cpu().numpy(), g_dst.cpu().numpy()
            c = oc.c.contents
            _same(g_index, index, f"gpu {p} cached index against numpy")
            _same(g_dst, dst, f"gpu {p} cached columns against numpy")
            _same(g_index, np.ctypeslib.as_array(c.topo_indptr[0], shape=(CAP_ONE + 1,)), f"gpu {p} cached index against the oracle")
            _same(g_dst, np.ctypeslib.as_array(c.topo_col[0], shape=(int(index[-1]),)), f"gpu {p} cached columns against the oracle")
            rows_f, r = ref.cached_rows(wl.features, QF, CAP_ONE, 1, 0)
            got = _feature_cache(hip, gpu, p, CAP_ONE, 4, "float32")
            _same(got.view(np.uint32), rows_f.view(np.uint32), f"gpu {p} cached rows against numpy")
            # served batches, judged from the oracle's side first
            o_off = oc.arr("edge_offset_map", np.int32)
            wants = [cpu.run(p, it, 0) for it in range(2)]
            rows = np.unique(np.concatenate([w["agg_dst_ids"] for w in wants]))
            assert (o_off[rows] >= ref.PASS_ELEMENTWISE).any(), "rows whose cached header cache_row_hdr wrote in its second pass"
            assert (o_off[rows] == ref.MISS).any() and ((o_off[rows] >= 0) & (o_off[rows] < ref.PASS_ELEMENTWISE)).any()
            for it, want in enumerate(wants):
                got = gpu.run(p, it, 0)
                compare_batches(got, want, f"gpu {p} batch {it}: ")
                _same(got["cache_search_buffer"], want["cache_search_buffer"], f"gpu {p} batch {it} cache_search_buffer")
    finally:
        gpu.close(); cpu.close()


@pytest.mark.gpu
def test_find_topo_over_every_id(hip, world):
    gpu, wl = world.gpu(4, 8, [2])
    try:
        gpu.cache.candidate_selection(1, gpu.graph)
        gpu.cache.set_capacity(CAP, CAP)
        gpu.cache.fill_up(gpu.feature, gpu.graph)
        rng = np.random.RandomState(37)
        ids = rng.permutation(N).astype(np.int32)
        neg = rng.choice(N, N // 100, replace=False)
        ids[neg] = -1 - rng.randint(0, 1 << 30, neg.size)
        ids[[0, ref.PASS_FIND - 1, ref.PASS_FIND, N - 1]] = [-1, -2, -(1 << 31), -3]
        assert ids.size > 2 * ref.PASS_FIND and (ids < 0).sum() >= N // 100
        index_map, offset_map = ref.edge_maps(world.QT, N, CAP, KG, 0)
        want_ind, want_off = ref.find_topo(index_map, offset_map, ids)
        assert (want_off[ref.PASS_FIND:] >= 0).sum() > 100_000 and (want_off == ref.MISS).sum() > N // 100
        for p in range(P):
            ind, off = gpu.cache.find_topo(p, torch.from_numpy(ids).to(DEV))
            torch.cuda.synchronize()
            _same(ind.cpu().numpy(), want_ind, f"gpu {p} partition index")
            _same(off.cpu().numpy(), want_off, f"gpu {p} partition offset")
    finally:
        gpu.close()


@pytest.mark.gpu
def test_hotness_measure_over_one_long_op(hip, world):
    wl = world.workload(4)
    gpu = GpuSide(wl, PRESC_BATCH, PRESC_FANOUT)
    cpu = CpuSide(wl, PRESC_BATCH, PRESC_FANOUT)
    try:
        for p in range(P):
            want = cpu.run(p, 0, 0, is_presc=True)
            assert int(want["node_counter"][7]) > ref.PASS_HOTNESS, "the op's id list is longer than one pass of the grid"
            compare_batches(gpu.run(p, 0, 0, is_presc=True), want, f"presc gpu {p}: ")
        for p in range(P):
            assert int(cpu.node_access[p].sum()) > ref.PASS_HOTNESS and int(cpu.edge_access[p].sum()) > 0
            _same(gpu.cache.array("node_access_time", p).cpu().numpy().view(np.uint64), cpu.node_access[p], f"gpu {p} node access")
            _same(gpu.cache.array("edge_access_time", p).cpu().numpy().view(np.uint64), cpu.edge_access[p], f"gpu {p} edge access")
    finally:
        gpu.close(); cpu.close()
