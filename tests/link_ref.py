"""The seeds of a link-prediction batch (GraphStorage.find_edges / negative_sample / edge_prediction_seeds, engine.unique_ids; the C ABI's
legion_find_edges, legion_negative_sample, legion_unique_ids) restated in numpy on the CPU as the contracts in include/legion_hip.h
write them, over tests/walk_ref's draws and unit_of: the row of an edge is np.searchsorted(side="right") over the row pointers, every
try of a negative forms its candidate and both rejections, the distinct list is np.unique's first occurrences put in index order.
A helper of the tests, not a test file."""
import numpy as np

from tests import node2vec_ref, walk_ref

M31 = walk_ref.M31
MAX_TRIES = 256                                                    # LEGION_NEGATIVE_MAX_TRIES
MAX_IDS = 2 ** 20                                                  # LEGION_UNIQUE_MAX_IDS
SELF, EDGES = 1, 2                                                 # the bits of `exclude`


# ---- the refusals (null pointers aside) ---------------------------------------------------------------------------------------------
def find_edges_refused(n):
    return n < 0


def negative_refused(n, k, exclude, max_tries, base, rows_sorted):
    """rows_sorted: 1, 0, or -1 (never checked)."""
    if n < 0 or k < 1 or base < 0 or base + n * k > M31:
        return True
    if exclude not in (0, 1, 2, 3) or not 1 <= max_tries <= MAX_TRIES:
        return True
    return bool(exclude & EDGES) and rows_sorted != 1


def table_slots(m):
    s = 256
    while s < 2 * m:
        s *= 2
    return s


def home_slots(ids, m):
    """The slot at which the table of m ids starts probing for each (non-negative) id: (id * 2654435769 mod 2^32) >> (32 - log2 slots),
    the multiplicative hash of kernels_link.hip.  Only the probe lengths depend on it, no result."""
    bits = table_slots(m).bit_length() - 1
    return ((np.asarray(ids, dtype=np.int64) * 2654435769) & 0xFFFFFFFF) >> (32 - bits)


def scratch_bytes(m):
    """legion_unique_ids_scratch_bytes: two int32 per table slot, two per id, one per tile of 256 ids; -1 for an illegal m."""
    if m < 0 or m > MAX_IDS:
        return -1
    return 4 * (2 * table_slots(m) + 2 * m + (m + 255) // 256)


def unique_refused(m, scratch, ids=0, unique=None, local=None, count=None):
    """ids, unique, local, count: addresses (None: far away)."""
    if m < 0 or m > MAX_IDS or scratch < scratch_bytes(m):
        return True
    over = lambda a, na: a is not None and ids < a + na and a < ids + 4 * m
    return over(unique, 4 * m) or over(local, 4 * m) or over(count, 4)


# ---- find_edges -------------------------------------------------------------------------------------------------------------------
def find_edges(indptr, col, eids, reads=None):
    """(row int32 [n], col int32 [n]); reads, if a dict, collects the positions of col that are read."""
    indptr, col = np.asarray(indptr, dtype=np.int64), np.asarray(col, dtype=np.int32)
    e = np.asarray(eids, dtype=np.int64)
    row = np.full(e.size, -1, dtype=np.int32)
    c = np.full(e.size, -1, dtype=np.int32)
    at = np.nonzero((e >= 0) & (e < col.size))[0]                  # 1. before any load
    if reads is not None:
        reads.setdefault("col", []).append(e[at].copy())
    got = col[e[at]]
    at, got = at[got >= 0], got[got >= 0]                          # 2. a dead entry: both -1
    row[at] = np.searchsorted(indptr, e[at], side="right") - 1     # 3. #{v : indptr[v] <= e} - 1
    c[at] = got
    return row, c


# ---- negative_sample --------------------------------------------------------------------------------------------------------------
def new_stats(node_num):
    """tries: candidates formed; self, hit: rejections by either rule; rejected_slots: slots that rejected at least once; exhausted:
    slots whose every try was rejected; searches_of_row / hits_of_row: per vertex r, the searches of its row and those that found u."""
    return {"tries": 0, "self": 0, "hit": 0, "rejected_slots": 0, "exhausted": 0, "slots": 0,
            "searches_of_row": np.zeros(node_num, dtype=np.int64), "hits_of_row": np.zeros(node_num, dtype=np.int64)}


def negative_sample(indptr, col, rows, k, exclude, max_tries=MAX_TRIES, base=0, reads=None, stats=None):
    """neg int32 [n, k].  reads, if a dict: the row pointers read (with exclude & 2 only) and, per search, the first and last position
    of the row searched.  stats, if a new_stats(node_num)."""
    indptr, col = np.asarray(indptr, dtype=np.int64), np.asarray(col, dtype=np.int32)
    rows = np.asarray(rows, dtype=np.int32)
    n, node_num = rows.size, indptr.size - 1
    r = np.repeat(rows.astype(np.int64), k)                        # slot m = i * k + j
    out = np.full(n * k, -1, dtype=np.int32)
    at = np.nonzero((r >= 0) & (r < node_num))[0]                  # 1. before any load
    keys = node2vec_ref._keys(indptr, col) if exclude & EDGES else None
    if exclude & EDGES:
        s, e = indptr[r[at]], indptr[r[at] + 1]                    # the pair, once per slot
        if reads is not None:
            reads.setdefault("indptr", []).extend([r[at].copy(), r[at] + 1])
    x = walk_ref.draws(base, n * k)[at]                            # try 0 of slot m: minstd(base + m + 1)
    rejected = np.zeros(n * k, dtype=bool)
    if stats is not None:
        stats["slots"] += int(at.size)
    for t in range(max_tries):                                     # 2. the slots in `at` are those still without a value
        if at.size == 0:
            break
        xt = x * np.uint64(walk_ref.minstd(t << 23)) % np.uint64(M31)      # minstd((nn + 1) + t 2^23)
        u = (walk_ref.unit_of(xt) * np.float64(node_num)).astype(np.int64)
        rr = r[at]
        own = (u == rr) if exclude & SELF else np.zeros(at.size, dtype=bool)
        hit = np.zeros(at.size, dtype=bool)
        if exclude & EDGES:
            look = ~own                                            # a candidate rejected as the row itself is not searched for
            key = (rr[look] << 32) | (u[look] + 1)
            pos = np.minimum(np.searchsorted(keys, key), max(keys.size - 1, 0))
            hit[look] = (keys[pos] == key) if keys.size else False
            if reads is not None:
                has = look & (e > s)
                reads.setdefault("col", []).extend([s[has].copy(), e[has] - 1])
            if stats is not None:
                np.add.at(stats["searches_of_row"], rr[look], 1)
                np.add.at(stats["hits_of_row"], rr[hit], 1)
        reject = own | hit
        if stats is not None:
            stats["tries"] += int(at.size)
            stats["self"] += int(own.sum())
            stats["hit"] += int(hit.sum())
        out[at[~reject]] = u[~reject]
        rejected[at[reject]] = True
        keep = reject
        at, x = at[keep], x[keep]
        if exclude & EDGES:
            s, e = s[keep], e[keep]
    if stats is not None:
        stats["rejected_slots"] += int(rejected.sum())
        stats["exhausted"] += int(at.size)                         # 3. every try rejected: the slot stays -1
    return out.reshape(n, k)


# ---- unique_ids -------------------------------------------------------------------------------------------------------------------
def unique_ids(ids):
    """(unique int32 [m], local int32 [m], count)."""
    ids = np.asarray(ids, dtype=np.int32)
    m = ids.size
    unique, local = np.full(m, -1, dtype=np.int32), np.full(m, -1, dtype=np.int32)
    live = np.nonzero(ids >= 0)[0]
    vals, first, inv = np.unique(ids[live], return_index=True, return_inverse=True)      # first: the first occurrence among the live
    order = np.argsort(first, kind="stable")                       # the distinct values in order of first appearance
    rank = np.empty(vals.size, dtype=np.int64)
    rank[order] = np.arange(vals.size)
    unique[:vals.size] = vals[order]
    local[live] = rank[inv.reshape(-1)]
    return unique, local, int(vals.size)


# ---- the three chained ------------------------------------------------------------------------------------------------------------
def edge_prediction_seeds(indptr, col, eids, k, exclude=3, max_tries=MAX_TRIES, base=0):
    """What GraphStorage.edge_prediction_seeds returns, and the concatenation it made: a dict of ids, seeds, num_seeds, pos_row, pos_col,
    neg_col, and the global row, col and neg."""
    row, c = find_edges(indptr, col, eids)
    neg = negative_sample(indptr, col, row, k, exclude, max_tries, base)
    ids = np.concatenate([row, c, neg.reshape(-1)])
    unique, local, count = unique_ids(ids)
    B = row.size
    return dict(ids=ids, row=row, col=c, neg=neg, seeds=unique, num_seeds=count, pos_row=local[:B], pos_col=local[B:2 * B],
                neg_col=local[2 * B:].reshape(B, k))


# ---- inputs of the tests ----------------------------------------------------------------------------------------------------------
def eids_for(indptr, col, n):
    """n edge ids over the graph of node2vec_ref.sym_graph(): -1, E and E + 5; the first and last entry of every hub row; indptr[v] of
    the rows right after the empty rows; every dead entry; E - 1; then a spread over all edges.  Truncated to n (n >= 1: E - 1 first)."""
    indptr, col = np.asarray(indptr, dtype=np.int64), np.asarray(col, dtype=np.int32)
    E = col.size
    head = [E - 1, -1, E, E + 5]
    for h in node2vec_ref.HUBS:
        head += [int(indptr[h]), int(indptr[h + 1]) - 1]
    deg = np.diff(indptr)
    after = [v + 1 for v in node2vec_ref.EMPTY if v + 1 < deg.size and deg[v + 1] > 0]
    head += [int(indptr[v]) for v in after]
    head += np.nonzero(col < 0)[0].tolist()
    rest = (np.arange(max(n, 1), dtype=np.int64) * 2654435761 % E)
    return np.concatenate([np.array(head, dtype=np.int64), rest])[:n]


def complete_graph(n=8):
    """K_n without loops: every row holds every other vertex, sorted."""
    col = np.array([u for v in range(n) for u in range(n) if u != v], dtype=np.int32)
    return np.arange(n + 1, dtype=np.int64) * (n - 1), col


def ring_graph(n=8):
    """The n-ring: row v holds v - 1 and v + 1 (mod n), sorted."""
    col = np.array([sorted(((v - 1) % n, (v + 1) % n)) for v in range(n)], dtype=np.int32).reshape(-1)
    return np.arange(n + 1, dtype=np.int64) * 2, col
