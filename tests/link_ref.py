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


# ---- the table of unique_ids, restated to say what an input does to it ------------------------------------------------------------
HASH = 2654435769                                                  # the multiplicative hash of kernels_link.hip; odd: a bijection mod 2^32
HASH_INV = pow(HASH, -1, 2 ** 32)


def ids_with_home(m, homes, per):
    """`per` distinct non-negative int32 ids for each home slot in `homes` of the table of m ids, home by home: the hash inverted.
    y = id * HASH mod 2^32 has home y >> shift, so the ids of a home are y * HASH_INV mod 2^32 over y in [home << shift,
    (home + 1) << shift), those below 2^31 kept, the first `per` in order of y taken."""
    slots = table_slots(m)
    shift = 32 - (slots.bit_length() - 1)
    out = []
    for home in homes:
        assert 0 <= home < slots, (home, slots)
        y = np.arange(home << shift, min((home + 1) << shift, (home << shift) + 4 * per + 4096), dtype=np.uint64)      # (half are kept)
        ids = (y * np.uint64(HASH_INV)) & np.uint64(0xFFFFFFFF)
        ids = ids[ids < 2 ** 31][:per]
        assert ids.size == per, f"home {home} of {slots} slots has {ids.size} non-negative ids, {per} asked for"
        out.append(ids.astype(np.int64))
    out = np.concatenate(out) if out else np.zeros(0, dtype=np.int64)
    assert np.array_equal(home_slots(out, m), np.repeat(np.asarray(homes, dtype=np.int64), per)) and np.unique(out).size == out.size
    return out.astype(np.int32)


def probe_table(ids, m, order, wrap=True):
    """The insert of unique_ids done one id at a time in the arrival order `order` (a permutation of the indices): linear probing from
    home_slots over table_slots(m) slots.  Returns (slot int64 [len(ids)], -1 for a negative id; the longest probe run, in slots looked
    at; how many distinct ids sit in a slot below their home: a wrap).  wrap=False is a wrong table, one that stops probing at its last
    slot: an id that finds no place gets slot -1.  Only a statement about inputs: which slot a key lands in depends on arrival order,
    so no GPU result is compared with this."""
    ids = np.asarray(ids, dtype=np.int64)
    slots = table_slots(m)
    homes = home_slots(np.maximum(ids, 0), m)
    nxt = np.arange(slots + 1, dtype=np.int64)                     # nxt[s]: a free slot at or after s, found by path halving; slots: none

    def free(s):
        while nxt[s] != s:
            nxt[s] = nxt[nxt[s]]
            s = nxt[s]
        return int(s)

    where, slot = {}, np.full(ids.size, -1, dtype=np.int64)
    longest = wraps = 0
    for i in np.asarray(order).tolist():
        v = int(ids[i])
        if v < 0:
            continue
        if v not in where:
            h = int(homes[i])
            s = free(h)
            if s == slots:                                         # nothing free up to the table's end
                s = free(0) if wrap else -1
            where[v] = s
            if s >= 0:
                nxt[s] = s + 1
                wraps += int(s < h)
                longest = max(longest, (s - h) % slots + 1)
            else:
                longest = max(longest, slots - h)
        slot[i] = where[v]
    return slot, longest, wraps


# ---- small graphs for find_edges --------------------------------------------------------------------------------------------------
def _graph_of_degrees(deg, seed, dead=0):
    deg = np.asarray(deg, dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    rng = np.random.RandomState(seed)
    col = rng.randint(0, deg.size, int(indptr[-1])).astype(np.int32)
    if dead:
        col[rng.choice(col.size, dead, replace=False)] = -1
    return indptr, col


def small_graphs():
    """name -> (indptr, col): one vertex with a self-loop; two and three vertices with empty rows first, in the middle and last; 254 to
    257 vertices of degree 0 .. 3 (N + 1 row pointers: a power of two and one or two either side) with three dead entries each; a
    graph whose first three and last three rows are empty; 64 rows with every edge in row 17."""
    g = {"loop": (np.array([0, 1], dtype=np.int64), np.array([0], dtype=np.int32)),
         "two-first-empty": _graph_of_degrees([0, 2], 1),
         "two-last-empty": _graph_of_degrees([2, 0], 2),
         "three-middle-empty": _graph_of_degrees([1, 0, 2], 3),
         "three-two-empty": _graph_of_degrees([0, 0, 3], 4),
         "ends-empty": _graph_of_degrees([0, 0, 0, 2, 1, 0, 3, 1, 0, 0, 2, 0, 0, 0], 5),
         "one-row": _graph_of_degrees([0] * 17 + [40] + [0] * 46, 6)}
    for n in (254, 255, 256, 257):
        g[f"degrees-{n}"] = _graph_of_degrees(np.random.RandomState(100 + n).randint(0, 4, n), 200 + n, dead=3)
    return g


def find_edges_lower_bound(indptr, col, eids):
    """A wrong find_edges: the row by a lower bound over the row pointers -- the first v with indptr[v] >= e, one less where that
    pointer is past e.  Right except where e starts a row that follows empty rows: there it names the first of the empty rows."""
    indptr = np.asarray(indptr, dtype=np.int64)
    row, c = find_edges(indptr, col, eids)
    e = np.asarray(eids, dtype=np.int64)
    live = row >= 0
    pos = np.searchsorted(indptr, e[live], side="left")
    row[live] = np.where(indptr[np.minimum(pos, indptr.size - 1)] == e[live], pos, pos - 1)
    return row, c
