"""tests/setup_ref.py against the C oracle (oracle/legion_oracle.c) at a small size, Kg in {1, 2}, with capacities below and beyond N:
after this the large GPU cases may use the numpy statements and the oracle side by side.  The prefix-sum table's vectorised form is
held against weighted_ref.cdf, which loops over rows."""
import numpy as np
import pytest

from oracle import ffi
from tests import setup_ref as ref
from tests import weighted_ref

N, D, P = 3001, 5, 2


def small_world():
    rng = np.random.RandomState(19)
    deg = rng.randint(0, 6, N).astype(np.int64)
    deg[rng.randint(0, N, 20)] = 40
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = rng.randint(0, N, int(indptr[-1])).astype(np.int32)
    col[rng.randint(0, col.size, 30)] = -1
    table = rng.rand(N, D).astype(np.float32)
    access = [np.floor(rng.pareto(1.1, N) * 0.35).astype(np.uint64) for _ in range(4)]      # most zero: ties everywhere
    return indptr, col, table, access


def from_ptr(ptr, shape, dtype):
    return np.ctypeslib.as_array(ptr, shape=shape).astype(dtype, copy=True) if int(np.prod(shape)) else np.zeros(shape, dtype)


CASES = [(1, 0, 700, 400), (2, 0, 700, 400), (2, 1, 301, 1200), (1, 0, N + 50, N + 9), (2, 0, 1600, 1501), (2, 0, 1, 1)]


@pytest.mark.parametrize("Kg,Ki,ncap,ecap", CASES)
def test_clique_fill_statements_match_the_oracle(oracle, Kg, Ki, ncap, ecap):
    indptr, col, table, access = small_world()
    oc = ffi.OracleCache(N, D, Kg, Ki)
    oc.candidate_selection(access[:Kg], access[2:2 + Kg])
    QF, AF = ref.hotness_order(access[:Kg])
    QT, AT = ref.hotness_order(access[2:2 + Kg])
    for name, want, dtype in (("QF", QF, np.int32), ("QT", QT, np.int32), ("AF", AF, np.uint64), ("AT", AT, np.uint64)):
        assert np.array_equal(oc.arr(name, dtype), want), name
    assert (AF == 0).mean() > 0.5 and not np.array_equal(QF, QT)
    oc.set_capacity(ncap, ecap)
    oc.fill_up(table, indptr, col)
    nmap = ref.node_map(QF, N, ncap, Kg)
    index_map, offset_map = ref.edge_maps(QT, N, ecap, Kg, Ki)
    assert np.array_equal(oc.arr("node_map", np.int32), nmap)
    assert np.array_equal(oc.arr("edge_index_map", np.int8), index_map)
    assert np.array_equal(oc.arr("edge_offset_map", np.int32), offset_map)
    assert int((nmap >= 0).sum()) == min(ncap * Kg, N) and int((offset_map >= 0).sum()) == min(ecap * Kg, N)
    c = oc.c.contents
    csrs = []
    for j in range(Kg):
        rows, r = ref.cached_rows(table, QF, ncap, Kg, j)
        got = from_ptr(c.feat_cache[j], (ncap, D), np.float32)
        assert np.array_equal(got[r].view(np.uint32), rows.view(np.uint32)), f"member {j}: cached rows"
        assert r.size == len(range(j, min(ncap * Kg, N), Kg)) and not got[r.size:].any()
        index, dst = ref.cached_csr(indptr, col, QT, ecap, Kg, j)
        assert np.array_equal(from_ptr(c.topo_indptr[j], (ecap + 1,), np.int64), index), f"member {j}: cached index"
        assert np.array_equal(from_ptr(c.topo_col[j], (int(index[-1]),), np.int32), dst), f"member {j}: cached columns"
        csrs.append(index)
    # the column-slot pairs: what lgo_find_feat answers for every column entry
    pairs = ref.column_slots(col, nmap)
    o_map = oc.arr("node_map", np.int32)
    assert np.array_equal(pairs[:, 0], col)
    assert np.array_equal(pairs[:, 1], np.array([o_map[v] if v >= 0 else -2 for v in col], dtype=np.int32))
    assert (pairs[col < 0, 1] == ref.MISS).all() and (col < 0).sum() >= 20
    # the row headers: where lgo_find_topo sends a vertex, and the row of that member's CSR it names
    ids = np.arange(N, dtype=np.int32)
    ind, off = np.zeros(N, dtype=np.int8), np.zeros(N, dtype=np.int32)
    oracle.lgo_find_topo(oc.c, ids.ctypes.data_as(ffi.P_I32), ind.ctypes.data_as(ffi.P_I8), off.ctypes.data_as(ffi.P_I32), N)
    f_ind, f_off = ref.find_topo(index_map, offset_map, ids)
    assert np.array_equal(ind, f_ind) and np.array_equal(off, f_off)
    start, deg, slot = ref.row_headers(indptr, QT, ecap, Kg, Ki, P)
    for v in range(N):
        if ind[v] == ref.MISS:
            want = (int(indptr[v]), int(indptr[v + 1] - indptr[v]), P)
        else:
            index = csrs[int(ind[v]) - Ki * Kg]
            want = (int(index[off[v]]), int(index[off[v] + 1] - index[off[v]]), int(ind[v]))
        assert (int(start[v]), int(deg[v]), int(slot[v])) == want, f"vertex {v}"
    assert np.array_equal(deg, np.diff(indptr)), "a cached row has the vertex's own degree"
    neg = np.array([5, -1, 0, -7, N - 1], dtype=np.int32)
    f_ind, f_off = ref.find_topo(index_map, offset_map, neg)
    assert f_ind[1] == f_ind[3] == ref.MISS and f_off[1] == f_off[3] == ref.MISS and f_off[0] == offset_map[5]
    oc.close()


@pytest.mark.parametrize("cpu_cap,gpu_cap", [(300, 200), (0, 250), (250, 0), (2000, 1500)])
def test_hybrid_statements_match_the_oracle(oracle, cpu_cap, gpu_cap):
    indptr, col, table, access = small_world()
    oc = ffi.OracleCache(N, D, 1, 0)
    oc.hybrid_init(access[1], table, cpu_cap, gpu_cap)
    QF, AF = ref.hotness_order([access[1]])
    assert np.array_equal(oc.arr("QF", np.int32), QF) and np.array_equal(oc.arr("AF", np.uint64), AF)
    assert np.array_equal(oc.arr("node_map", np.int32), ref.hybrid_map(QF, N, cpu_cap, gpu_cap))
    c = oc.c.contents
    n_gpu, n_cpu = min(gpu_cap, N), max(min(cpu_cap, N - gpu_cap), 0)
    rows, r = ref.cached_rows(table, QF[:n_gpu], n_gpu, 1, 0)
    assert np.array_equal(from_ptr(c.feat_cache[0], (max(gpu_cap, 1), D), np.float32)[:n_gpu].view(np.uint32), rows.view(np.uint32))
    rows, r = ref.cached_rows(table, QF[gpu_cap:], n_cpu, 1, 0)
    assert np.array_equal(from_ptr(c.cpu_cache, (max(cpu_cap, 1), D), np.float32)[:n_cpu].view(np.uint32), rows.view(np.uint32))
    oc.close()


def small_rows():
    """The rows of tests/test_gpu_sample_weighted.py's fixture: every length at which the table build changes its path."""
    from tests.test_gpu_sample_weighted import ROW_DEGREES, ZERO_ROW
    deg = np.array(ROW_DEGREES, dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    E = int(indptr[-1])
    rng = np.random.RandomState(7)
    w = (rng.randint(1, 33, E) / 8).astype(np.float32)
    for v in range(deg.size):
        s, n = int(indptr[v]), int(deg[v])
        if n >= 2 and v % 2 == 0:
            w[s:s + max(n // 5, 1)] = 0
        if n >= 2 and v % 3 == 0:
            w[s + n - max(n // 7, 1):s + n] = 0
        if n >= 60:
            w[s + n // 2:s + n // 2 + n // 9] = 0
    w[indptr[ZERO_ROW]:indptr[ZERO_ROW + 1]] = 0
    return indptr, w


def test_segmented_table_is_the_row_loop_bit_for_bit():
    indptr, w = small_rows()
    assert np.array_equal(ref.cdf_segmented(indptr, w).view(np.uint32), weighted_ref.cdf(indptr, w).view(np.uint32))
    rng = np.random.RandomState(23)
    deg = rng.randint(0, 200, 400).astype(np.int64)
    deg[rng.randint(0, 400, 40)] = 0
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    E = int(indptr[-1])
    w = (rng.rand(E) * 10.0 ** rng.randint(-6, 6, E)).astype(np.float32)          # sums that round: the order of the additions shows
    special = np.array([-1.5, np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-42, 3e-39], dtype=np.float32)
    at = rng.rand(E) < 0.2
    w[at] = special[rng.randint(0, special.size, int(at.sum()))]
    got, want = ref.cdf_segmented(indptr, w), weighted_ref.cdf(indptr, w)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.unique(want).size > E // 4
    assert ref.cdf_segmented(np.zeros(5, dtype=np.int64), np.zeros(0, np.float32)).size == 0
