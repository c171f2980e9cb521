"""Random walks (GraphStorage.random_walk, legion_random_walk) restated in numpy on the CPU, step by step as the contract in
include/legion_hip.h writes them: the minstd power is Python's pow(48271, k, 2**31 - 1), the weighted pick is tests/weighted_ref's table
with np.searchsorted(side="right").  A helper of the tests, not a test file."""
import numpy as np

M31 = 2 ** 31 - 1


def minstd(k):
    """48271^k mod (2^31 - 1)."""
    return pow(48271, int(k), M31)


def refused(num_walks, length, weighted, restart_prob, base, has_table):
    """True where legion_random_walk returns -1 for these values (null pointers aside)."""
    if num_walks < 0 or length < 1 or base < 0 or base + num_walks * length > M31:
        return True
    if weighted not in (0, 1) or (weighted == 1 and not has_table):
        return True
    p = np.float32(restart_prob)
    return not (p >= 0 and p <= 1)


def draws_slow(first, count, offset=0):
    """The definition of draws: one pow per draw index, nothing shared."""
    return np.array([minstd(((k + 1) & 0xFFFFFFFF) + offset) for k in range(first, first + count)], dtype=np.uint64)


_DRAWS = {}                                                       # (first, offset) -> the longest run computed so far


def draws(first, count, offset=0):
    """minstd(k + offset) for k = first + 1 .. first + count as uint64: the x of draw indices first .. first + count - 1 (offset 0) or
    their restart draws (offset 2^31, on the uint32 of k).  A run is computed once and shared: shorter runs are its prefixes.
    The exponents of a legal call are consecutive integers (first + count <= 2^31 - 1: nothing wraps inside a run), so a run grows by
    doubling: a run of length m, then the same run times 48271^m -- in uint64, products below 2^62.  draws_slow is the definition."""
    have = _DRAWS.get((first, offset))
    if have is None and count > 0:
        have = np.array([minstd(first + 1 + offset)], dtype=np.uint64)
    if have is not None and have.size < count:
        assert first >= 0 and first + count <= M31 and offset in (0, 2 ** 31), (first, count, offset)
        while have.size < count:
            m = min(have.size, count - have.size)
            have = np.concatenate([have, have[:m] * np.uint64(minstd(have.size)) % np.uint64(M31)])
        have.setflags(write=False)
        _DRAWS[(first, offset)] = have
    return have[:count] if have is not None else np.zeros(0, dtype=np.uint64)


def unit_of(x):
    """The double both draws form from a minstd value: (x - 1) / 2147483646."""
    return (x - np.uint64(1)).astype(np.float64) / 2147483646.0


def step(indptr, col, node_num, v, x, y=None, table=None, restart_prob=0.0, reads=None):
    """One transition of every walk at once: v int64[n] the current vertices, x (and y with restart_prob > 0) the minstd values of the
    step's draw indices.  Returns (next vertex, edge id), both -1 where the walk has ended or ends.  reads, if a dict, collects every
    index the step reads per array name."""
    def read(name, arr, i):
        if reads is not None:
            reads.setdefault(name, []).append(np.asarray(i, dtype=np.int64).copy())
        return arr[i]
    nxt = np.full(v.size, -1, dtype=np.int64)
    eid = np.full(v.size, -1, dtype=np.int64)
    live = (v >= 0) & (v < node_num)                             # 1. before any load
    if restart_prob > 0:                                         # 2.
        live &= ~(unit_of(y) < np.float64(np.float32(restart_prob)))
    at = np.nonzero(live)[0]
    s = read("indptr", indptr, v[at])                            # 3.
    D = read("indptr", indptr, v[at] + 1) - s
    at, s, D = at[D > 0], s[D > 0], D[D > 0]
    r = unit_of(x[at])                                           # 4.
    if table is None:
        pick = (r * D.astype(np.float64)).astype(np.int64)
    else:
        T = read("edge_cdf", table, s + D - 1).astype(np.float64)
        at, s, D, r, T = at[T > 0], s[T > 0], D[T > 0], r[T > 0], T[T > 0]
        t = r * T
        pick = np.zeros(at.size, dtype=np.int64)
        order = np.argsort(s, kind="stable")                     # (rows with entries have distinct starts: one search per row)
        cuts = np.nonzero(np.diff(s[order]))[0] + 1
        for grp in np.split(order, cuts) if at.size else []:
            row = table[s[grp[0]]:s[grp[0]] + D[grp[0]]].astype(np.float64)      # (every probe of the search lies in here)
            pick[grp] = np.searchsorted(row, t[grp], side="right")
        pick = np.minimum(pick, D - 1)
    u = read("col", col, s + pick).astype(np.int64)              # 5.
    ok = u >= 0
    nxt[at[ok]], eid[at[ok]] = u[ok], (s + pick)[ok]
    return nxt, eid


def walk(indptr, col, seeds, length, table=None, restart_prob=0.0, base=0, reads=None):
    """(traces int32 [n, length + 1], eids int64 [n, length]) of the walks from seeds; table: the prefix table of a weighted walk."""
    indptr = np.asarray(indptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int32)
    seeds = np.asarray(seeds, dtype=np.int32)
    n, node_num = seeds.size, indptr.size - 1
    traces = np.full((n, length + 1), -1, dtype=np.int32)
    eids = np.full((n, length), -1, dtype=np.int64)
    traces[:, 0] = seeds                                         # copied as given
    x = draws(base, n * length).reshape(n, length)               # walk w, step j: draw index base + w * length + (j - 1)
    y = draws(base, n * length, 2 ** 31).reshape(n, length) if restart_prob > 0 else None
    v = seeds.astype(np.int64)
    for j in range(1, length + 1):
        v, e = step(indptr, col, node_num, v, x[:, j - 1], None if y is None else y[:, j - 1], table, restart_prob, reads)
        traces[:, j], eids[:, j - 1] = v, e                      # 1. / 6.: an ended walk stays -1 in both arrays
    return traces, eids


def check(indptr, col, seeds, traces, eids):
    """What holds for every walk whatever was drawn: the seed is copied, every transition is an edge named by its id inside the row of
    the vertex it leaves, and -1 is absorbing in both arrays."""
    indptr = np.asarray(indptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int32)
    assert traces.dtype == np.int32 and eids.dtype == np.int64
    n, L1 = traces.shape
    assert eids.shape == (n, L1 - 1) and np.array_equal(traces[:, 0], np.asarray(seeds, dtype=np.int32))
    nxt, prev = traces[:, 1:], traces[:, :-1].astype(np.int64)
    live = nxt >= 0
    assert np.all(nxt[~live] == -1) and np.all(eids[~live] == -1)
    assert np.all(live[:, 1:] <= live[:, :-1])                    # once ended, ended
    e = eids[live]
    assert np.all((prev[live] >= 0) & (prev[live] < indptr.size - 1))
    assert np.all((indptr[prev[live]] <= e) & (e < indptr[prev[live] + 1]))
    assert np.array_equal(col[e], nxt[live])


def assert_reads_in_bounds(reads, node_num, edge_num):
    """Every index a walk read (walk(..., reads={})) lies inside its array: indptr has node_num + 1 entries, col and edge_cdf edge_num."""
    size = {"indptr": node_num + 1, "col": edge_num, "edge_cdf": edge_num}
    for name, chunks in reads.items():
        for i in chunks:
            assert i.size == 0 or (int(i.min()) >= 0 and int(i.max()) < size[name]), (name, int(i.min()), int(i.max()), size[name])


# ---- the hand-built graph of the walk tests ---------------------------------------------------------------------------------------
SPECIAL_DEGREES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 4097]      # vertices 0 .. 9
ZERO_ROW = 10                                                      # every weight of this row is zero
NODE_NUM = 6000


def hand_graph():
    """About 6 000 vertices: the rows of SPECIAL_DEGREES, then degrees 1 .. 12 and a few empty rows; a tenth of the entries point at the first sixteen
    vertices (so walks reach the special rows), self-loops, parallel edges and a few dead (negative) column entries.  Weights are
    multiples of 1/8 (exact prefix sums: the table is unique) with leading, inner and trailing runs of zeros and one all-zero row."""
    rng = np.random.RandomState(20)
    deg = rng.randint(1, 13, NODE_NUM).astype(np.int64)
    deg[rng.rand(NODE_NUM) < 0.03] = 0
    deg[:len(SPECIAL_DEGREES)] = SPECIAL_DEGREES
    deg[ZERO_ROW] = 9
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    E = int(indptr[-1])
    col = rng.randint(0, NODE_NUM, E).astype(np.int32)
    near = rng.rand(E) < 0.1
    col[near] = rng.randint(0, 16, int(near.sum()))
    w = (rng.randint(1, 33, E) / 8).astype(np.float32)
    for v in range(NODE_NUM):
        s, D = int(indptr[v]), int(deg[v])
        if D >= 1 and v % 7 == 0:
            col[s] = v                                             # a self-loop
        if D >= 2 and v % 5 == 0:
            col[s + 1] = col[s]                                    # parallel edges
        if D >= 2 and v % 2 == 0:
            w[s:s + max(D // 5, 1)] = 0                            # a leading run of zeros
        if D >= 2 and v % 3 == 0:
            w[s + D - max(D // 7, 1):s + D] = 0                    # a trailing run
        if D >= 60:
            w[s + D // 2:s + D // 2 + D // 9] = 0                  # an inner run
    col[rng.rand(E) < 0.005] = -1                                  # dead entries
    col[indptr[4] + 7] = -1                                        # ... one of them in a special row
    w[indptr[ZERO_ROW]:indptr[ZERO_ROW + 1]] = 0
    return indptr, col, w


def seeds_for(n):
    """n seeds over the whole graph: the special rows first, with repeats, a -1 and a node_num among them (n >= 4)."""
    s = (np.arange(n, dtype=np.int64) * 2654435761 % NODE_NUM).astype(np.int32)
    s[:min(n, 12)] = np.arange(12, dtype=np.int32)[:min(n, 12)]   # vertices 0 .. 9, the zero row, one more
    if n >= 4:
        s[n // 2] = s[0]                                           # a repeat
        s[n - 1] = -1
        s[n - 2] = NODE_NUM
    if n == 1:
        s[0] = 9                                                   # the long row
    return s
