"""What the one-time set-up kernels (kernels_cache.hip, kernels_weights.hip) build, stated in plain numpy
over whole arrays: the hotness order, the id -> slot maps of a clique fill and of the hybrid tier, a member's cached feature rows and cached
CSR, the column-slot pairs, the row headers, and the per-row prefix-sum table.  tests/test_setup_ref_cpu.py holds every statement against
the C oracle at a small size; the large GPU cases (tests/test_gpu_setup_stride.py, tests/test_gpu_weights_stride.py) then use both.
A helper of the tests, not a test file."""
import numpy as np

from tests import weighted_ref

MISS = -2                                  # LEGION_CACHEMISS_FLAG

# threads (waves, rows) of one pass of each capped grid, as the launches in the sources state them
PASS_ELEMENTWISE = 4096 * 256              # grid_for() and the row-header launches: over N (aggregate_access, iota, edge_mem, fill, init_row_hdr),
                                           # over cap * Kg ranks (the maps), over ONE member's capacity (topo_neighbor_count, cache_row_hdr)
PASS_ROW_WAVES = 8192 * 4                  # feat_fill_up, feat_fill_up_bf16, topo_fill_up: one wave per cached row
PASS_COLUMN_SLOTS = 8192 * 256
PASS_BF16_CHUNKS = 16384 * 256             # convert_f32_to_bf16: one thread per 8 elements of the padded row
PASS_FIND = 2048 * 256
PASS_HOTNESS = 1024 * 256
CDF_BLOCK = 64                             # edge_cdf_rows_kernel: a wave takes 64 consecutive rows
PASS_CDF_ROWS = 8192 * 4 * CDF_BLOCK
CDF_LONG = 4096                            # rows above this many entries get a workgroup
PASS_CDF_LONG_ROWS = 512


def hotness_order(access_list):
    """(order int32[N], sorted sums uint64[N]): stable descending over the members' summed counters -- ties keep ascending id."""
    keys = np.zeros(np.asarray(access_list[0]).size, dtype=np.uint64)
    for a in access_list:
        keys = keys + np.asarray(a, dtype=np.uint64)
    order = np.argsort(np.uint64(0xFFFFFFFFFFFFFFFF) - keys, kind="stable").astype(np.int32)
    return order, keys[order]


def _ranks(N, cap, Kg):
    return np.arange(min(int(cap) * int(Kg), int(N)), dtype=np.int64)


def node_map(QF, N, cap, Kg):
    """node_map[QF[t]] = (t % Kg) * cap + t // Kg for t < min(cap * Kg, N); every other id misses."""
    m = np.full(N, MISS, dtype=np.int32)
    t = _ranks(N, cap, Kg)
    m[QF[t]] = ((t % Kg) * cap + t // Kg).astype(np.int32)
    return m


def edge_maps(QT, N, cap, Kg, Ki):
    """(edge_index_map int8[N], edge_offset_map int32[N]) of clique Ki: the caching GPU t % Kg + Ki * Kg and its row t // Kg."""
    index = np.full(N, MISS, dtype=np.int8)
    offset = np.full(N, MISS, dtype=np.int32)
    t = _ranks(N, cap, Kg)
    index[QT[t]] = (t % Kg + Ki * Kg).astype(np.int8)
    offset[QT[t]] = (t // Kg).astype(np.int32)
    return index, offset


def hybrid_map(QF, N, cpu_cap, gpu_cap):
    """The gpu_cap hottest ids -> slots cpu_cap + t (the GPU cache), the next cpu_cap ids -> slots t - gpu_cap (the CPU cache)."""
    m = np.full(N, MISS, dtype=np.int32)
    t = np.arange(min(int(cpu_cap) + int(gpu_cap), int(N)), dtype=np.int64)
    m[QF[t]] = np.where(t < gpu_cap, cpu_cap + t, t - gpu_cap).astype(np.int32)
    return m


def member_ranks(N, cap, Kg, Ki):
    """(rows r, ranks t = r * Kg + Ki) of the cache rows of member Ki that hold a vertex: t < N."""
    r = np.arange(int(cap), dtype=np.int64)
    t = r * Kg + Ki
    live = t < N
    return r[live], t[live]


def cached_rows(table, QF, cap, Kg, Ki):
    """(rows, r): row r[i] of member Ki's feature cache is rows[i] = table[QF[r * Kg + Ki]]; rows whose rank is past N are not written."""
    r, t = member_ranks(QF.size, cap, Kg, Ki)
    return table[QF[t]], r


def cached_csr(indptr, col, QT, cap, Kg, Ki):
    """(index int64[cap + 1], dst int32[index[cap]]): row r of member Ki's CSR is the adjacency of QT[r * Kg + Ki], empty past N."""
    indptr = np.asarray(indptr, dtype=np.int64)
    r, t = member_ranks(QT.size, cap, Kg, Ki)
    ids = QT[t].astype(np.int64)
    counts = np.zeros(int(cap), dtype=np.int64)
    counts[r] = indptr[ids + 1] - indptr[ids]
    index = np.zeros(int(cap) + 1, dtype=np.int64)
    np.cumsum(counts, out=index[1:])
    total = int(index[-1])
    within = np.arange(total, dtype=np.int64) - np.repeat(index[:-1], counts)
    begin = np.zeros(int(cap), dtype=np.int64)
    begin[r] = indptr[ids]
    return index, np.asarray(col)[np.repeat(begin, counts) + within].astype(np.int32)


def column_slots(col, nmap):
    """int32[E, 2]: {col[e], node_map[col[e]]}, or a miss for a dead column (col[e] < 0)."""
    col = np.asarray(col, dtype=np.int32)
    slot = np.where(col >= 0, nmap[np.maximum(col, 0)], MISS).astype(np.int32)
    return np.stack([col, slot], axis=1)


def row_headers(indptr, QT, cap, Kg, Ki, P):
    """(start int64[N], deg int32[N], slot int32[N]) as a member of clique Ki sees them: every vertex in the full CSR (slot P) first, then
    the rows each member j of the clique caches point into that member's CSR (slot Ki * Kg + j)."""
    indptr = np.asarray(indptr, dtype=np.int64)
    N = indptr.size - 1
    start, deg, slot = indptr[:-1].copy(), np.diff(indptr).astype(np.int32), np.full(N, P, dtype=np.int32)
    for j in range(Kg):
        r, t = member_ranks(N, cap, Kg, j)
        ids = QT[t]
        counts = np.zeros(int(cap), dtype=np.int64)
        counts[r] = indptr[ids.astype(np.int64) + 1] - indptr[ids]
        index = np.concatenate([[0], np.cumsum(counts)])
        start[ids], deg[ids], slot[ids] = index[r], (index[r + 1] - index[r]).astype(np.int32), Ki * Kg + j
    return start, deg, slot


def find_topo(index_map, offset_map, ids):
    """legion_cache_find_topo: the two maps at ids, a miss for a negative id."""
    ids = np.asarray(ids, dtype=np.int64)
    at = np.maximum(ids, 0)
    return (np.where(ids >= 0, index_map[at], MISS).astype(np.int8), np.where(ids >= 0, offset_map[at], MISS).astype(np.int32))


def cdf_segmented(indptr, w):
    """weighted_ref.cdf with the loop over positions inside a row instead of over rows: entry i of every row that has one takes the row's
    running float64 sum, in the order np.cumsum adds, so the two agree bit for bit for any weights.  The rows are ordered by length, so
    step i works on a prefix of them; a graph of two million rows with a longest row of a few thousand entries takes a second."""
    indptr = np.asarray(indptr, dtype=np.int64)
    ws = weighted_ref.sanitise(w).astype(np.float64)
    out = np.zeros(ws.size, dtype=np.float32)
    deg = np.diff(indptr)
    rows = np.nonzero(deg > 0)[0]
    if rows.size == 0:
        return out
    rows = rows[np.argsort(-deg[rows], kind="stable")]
    d, start = deg[rows], indptr[rows]
    acc = np.zeros(rows.size, dtype=np.float64)
    for i in range(int(d[0])):
        k = int(np.searchsorted(-d, -i, side="left"))            # the rows with more than i entries
        at = start[:k] + i
        acc[:k] += ws[at]
        out[at] = acc[:k]
    return out
