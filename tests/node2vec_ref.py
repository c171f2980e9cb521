"""node2vec walks (GraphStorage.node2vec_random_walk, legion_node2vec_walk) restated in numpy on the CPU, try by try as the contract in
include/legion_hip.h writes them, over tests/walk_ref's draws and unit_of: every try forms its candidate, its class (by np.searchsorted
over the sorted rows) and its accept draw; nothing is decided early.  A helper of the tests, not a test file."""
import numpy as np

from tests import walk_ref

M31 = walk_ref.M31
MAX_TRIES = 256                                                    # LEGION_NODE2VEC_MAX_TRIES
MAX_BIAS = 16                                                      # LEGION_NODE2VEC_MAX_BIAS
RETURN, NEIGHBOUR, OTHER = 0, 1, 2                                 # the class of a candidate u: u == t, u in t's row, neither


def bias(p, q):
    """(a, b, Mx) in double from the float32 p, q the library sees."""
    a, b = 1.0 / float(np.float32(p)), 1.0 / float(np.float32(q))
    return a, b, max(a, 1.0, b)


def refused(num_walks, length, p, q, weighted, max_tries, base, has_table, rows_sorted):
    """True where legion_node2vec_walk returns -1 for these values (null pointers aside).  rows_sorted: 1, 0, or -1 (never checked)."""
    if num_walks < 0 or length < 1 or base < 0 or base + num_walks * length > M31:
        return True
    if weighted not in (0, 1) or (weighted == 1 and not has_table):
        return True
    if not 1 <= max_tries <= MAX_TRIES:
        return True
    with np.errstate(over="ignore", invalid="ignore"):
        pf, qf = np.float32(p), np.float32(q)
    if not (pf > 0 and qf > 0 and np.isfinite(pf) and np.isfinite(qf)):
        return True
    a, b, mx = bias(pf, qf)
    if min(a, 1.0, b) * MAX_BIAS < mx:
        return True
    return rows_sorted != 1


def rows_sorted(indptr, col):
    """The definition: no two adjacent entries of one row decrease."""
    indptr, col = np.asarray(indptr, dtype=np.int64), np.asarray(col, dtype=np.int32)
    if col.size < 2:
        return True
    down = col[:-1] > col[1:]                                      # down[e - 1]: the pair (e - 1, e)
    starts = indptr[:-1][np.diff(indptr) > 0]
    inside = np.ones(col.size - 1, dtype=bool)
    inside[starts[(starts > 0) & (starts < col.size)] - 1] = False
    return not bool((down & inside).any())


def _keys(indptr, col):
    """(row, entry + 1) of every column position as one int64, increasing over the whole array when the rows are sorted: membership of
    u in row t is one np.searchsorted."""
    rows = np.repeat(np.arange(indptr.size - 1, dtype=np.int64), np.diff(indptr))
    keys = (rows << 32) | (col.astype(np.int64) + 1)
    assert np.all(keys[1:] >= keys[:-1]), "rows not sorted"
    return keys


def new_stats():
    return {"accepted": [0, 0, 0], "rejected": [0, 0, 0], "forced": 0, "first": 0, "tries": 0, "steps": 0, "searches": 0,
            "searched_rows": set()}


def walk(indptr, col, seeds, length, p, q, table=None, max_tries=MAX_TRIES, base=0, reads=None, stats=None):
    """(traces int32 [n, length + 1], eids int64 [n, length]) of the node2vec walks from seeds; table: the prefix table of a weighted
    walk.  reads, if a dict, collects every index read per array name (for the search of t's row: its first and last position).
    stats, if a new_stats(): accepted / rejected candidates per class (tries with an accept draw), forced last tries, first steps,
    tries and steps taken, and the tries an implementation that decides before searching still has to search (with their t)."""
    indptr = np.asarray(indptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int32)
    seeds = np.asarray(seeds, dtype=np.int32)
    n, node_num = seeds.size, indptr.size - 1
    a, b, mx = bias(p, q)
    keys = _keys(indptr, col)

    def read(name, arr, i):
        if reads is not None:
            reads.setdefault(name, []).append(np.asarray(i, dtype=np.int64).copy())
        return arr[i]

    traces = np.full((n, length + 1), -1, dtype=np.int32)
    eids = np.full((n, length), -1, dtype=np.int64)
    traces[:, 0] = seeds
    x0 = walk_ref.draws(base, n * length).reshape(n, length)       # try 0 of walk w, step j: minstd(base + w * length + (j - 1) + 1)
    v = seeds.astype(np.int64)
    t = np.full(n, -1, dtype=np.int64)
    for j in range(1, length + 1):
        nxt = np.full(n, -1, dtype=np.int64)
        live = (v >= 0) & (v < node_num)                           # 1. before any load
        at = np.nonzero(live)[0]
        s = read("indptr", indptr, v[at])                          # 2.
        D = read("indptr", indptr, v[at] + 1) - s
        at, s, D = at[D > 0], s[D > 0], D[D > 0]
        T = None
        if table is not None:
            T = read("edge_cdf", table, s + D - 1).astype(np.float64)
            at, s, D, T = at[T > 0], s[T > 0], D[T > 0], T[T > 0]
        for i in range(max_tries):                                 # 3. the lanes in `at` are those still without an accepted candidate
            if at.size == 0:
                break
            x = x0[at, j - 1] * np.uint64(walk_ref.minstd(i << 23)) % np.uint64(M31)      # minstd((n + 1) + i 2^23)
            r = walk_ref.unit_of(x)
            if table is None:
                pick = (r * D.astype(np.float64)).astype(np.int64)
            else:
                target = r * T
                lo, hi = np.zeros(at.size, dtype=np.int64), D.copy()                      # #{e : cdf[s + e] <= target} by bisection
                while True:
                    open_ = np.nonzero(lo < hi)[0]
                    if open_.size == 0:
                        break
                    mid = (lo[open_] + hi[open_]) // 2
                    le = read("edge_cdf", table, s[open_] + mid).astype(np.float64) <= target[open_]
                    lo[open_] = np.where(le, mid + 1, lo[open_])
                    hi[open_] = np.where(le, hi[open_], mid)
                pick = np.minimum(lo, D - 1)
            u = read("col", col, s + pick).astype(np.int64)
            dead = u < 0                                           # ends the walk at once: nxt stays -1
            if stats is not None:
                stats["tries"] += int(at.size)
            if j == 1 or i == max_tries - 1:
                accept = ~dead
                if stats is not None:
                    stats["first" if j == 1 else "forced"] += int(accept.sum())
            else:
                tt = t[at]
                ts, te = indptr[tt], indptr[tt + 1]
                if reads is not None:
                    has = te > ts
                    reads.setdefault("col", []).extend([ts[has].copy(), te[has] - 1])
                key = (tt << 32) | (u + 1)
                pos = np.minimum(np.searchsorted(keys, key), keys.size - 1)
                member = keys[pos] == key                          # u occurs in col[indptr[t] .. indptr[t + 1])
                cls = np.where(u == tt, RETURN, np.where(member, NEIGHBOUR, OTHER))
                wt = np.where(cls == RETURN, a, np.where(cls == NEIGHBOUR, 1.0, b))
                y = x * np.uint64(walk_ref.minstd(1 << 22)) % np.uint64(M31)              # minstd((n + 1) + i 2^23 + 2^22)
                z = walk_ref.unit_of(y) * mx
                accept = (z < wt) & ~dead
                if stats is not None:
                    for c in (RETURN, NEIGHBOUR, OTHER):
                        stats["accepted"][c] += int((accept & (cls == c)).sum())
                        stats["rejected"][c] += int((~accept & ~dead & (cls == c)).sum())
                    need = ~dead & (cls != RETURN) & (z >= min(1.0, b)) & (z < max(1.0, b))
                    stats["searches"] += int(need.sum())
                    stats["searched_rows"].update(np.unique(tt[need]).tolist())
            nxt[at[accept]] = u[accept]
            eids[at[accept], j - 1] = (s + pick)[accept]
            go = ~accept & ~dead
            at, s, D = at[go], s[go], D[go]
            if T is not None:
                T = T[go]
        assert at.size == 0, "a lane left the last try without a candidate"
        took = nxt >= 0
        t = np.where(took, v, t)
        v = nxt
        traces[:, j] = v
        if stats is not None:
            stats["steps"] += int(took.sum())
    return traces, eids


# ---- the symmetric graph of the node2vec tests ------------------------------------------------------------------------------------
NODE_NUM = 6000
HUBS = {0: 63, 1: 64, 2: 65, 3: 255, 4: 256, 5: 257, 6: 4097}      # vertex -> entries of its row
ZERO_ROW = 10                                                      # every weight of this row is zero
EMPTY = (7, 40, 41, 1234, 3000, 5998)                              # rows without entries (nothing points at them either)


def sym_graph(node_num=NODE_NUM, hubs=HUBS, empty=EMPTY, chords=3000):
    """About 6 000 vertices, every edge in both directions so that all three classes are common: a ring lattice v +- 1 .. 3 over the
    vertices that have rows, 3 000 random chords, hub rows of 63-65, 255-257 and 4 097 entries, a few empty rows, parallel edges and
    self-loops; rows sorted; then the first entry of a few rows made dead (-1, still first).  Weights are walk_ref's multiples of 1/8
    with leading, inner and trailing runs of zeros and one all-zero row.  node_num, hubs, empty and chords: the same graph at another
    size (tests/far_rows.py); the defaults are the graph of the node2vec tests."""
    rng = np.random.RandomState(22)
    ring = np.array([v for v in range(node_num) if v not in empty], dtype=np.int64)
    src, dst = [], []
    for d in (1, 2, 3):
        src.append(ring)
        dst.append(np.roll(ring, -d))
    plain = ring[ring > max(hubs)]                                 # the hubs get their chords below, counted
    c = rng.choice(plain, (chords, 2))
    c = c[c[:, 0] != c[:, 1]]
    src.append(c[:, 0])
    dst.append(c[:, 1])
    twice = c[::10]                                                # parallel edges: every tenth chord a second time
    src.append(twice[:, 0])
    dst.append(twice[:, 1])
    src, dst = np.concatenate(src), np.concatenate(dst)
    loops = plain[::7]                                             # self-loops: one entry each
    deg = np.bincount(np.concatenate([src, dst, loops]), minlength=node_num)
    hs, hd = [], []
    for h, want in hubs.items():
        near = set(dst[src == h].tolist()) | set(src[dst == h].tolist())
        pool = np.array([x for x in plain if x not in near], dtype=np.int64)
        more = rng.choice(pool, want - int(deg[h]), replace=False)
        hs.append(np.full(more.size, h, dtype=np.int64))
        hd.append(more)
    src, dst = np.concatenate([src] + hs), np.concatenate([dst] + hd)
    rows = np.concatenate([src, dst, loops])
    cols = np.concatenate([dst, src, loops])
    order = np.lexsort((cols, rows))
    rows, col = rows[order], cols[order].astype(np.int32)
    deg = np.bincount(rows, minlength=node_num).astype(np.int64)
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    assert all(deg[h] == want for h, want in hubs.items()) and all(deg[v] == 0 for v in empty)
    for v in list(range(50, node_num, 211)) + [3]:                 # dead entries: first in their rows, so the rows stay sorted
        col[indptr[v]] = -1
    E = col.size
    w = (rng.randint(1, 33, E) / 8).astype(np.float32)
    for v in range(node_num):
        s, D = int(indptr[v]), int(deg[v])
        if D >= 2 and v % 2 == 0:
            w[s:s + max(D // 5, 1)] = 0                            # a leading run of zeros
        if D >= 2 and v % 3 == 0:
            w[s + D - max(D // 7, 1):s + D] = 0                    # a trailing run
        if D >= 60:
            w[s + D // 2:s + D // 2 + D // 9] = 0                  # an inner run
    w[indptr[ZERO_ROW]:indptr[ZERO_ROW + 1]] = 0
    assert rows_sorted(indptr, col)
    return indptr, col, w


def seeds_for(n):
    """n seeds over the whole graph: the hubs and the special rows first, with repeats, a -1 and a node_num among them (n >= 4)."""
    s = (np.arange(n, dtype=np.int64) * 2654435761 % NODE_NUM).astype(np.int32)
    s[:min(n, 12)] = np.arange(12, dtype=np.int32)[:min(n, 12)]   # the hubs, an empty row, the zero row, two more
    s[12:n:5] = 6                                                  # the long row often: walks leave it and search it on the step after
    if n >= 4:
        s[n // 2] = s[0]                                           # a repeat
        s[n - 1] = -1
        s[n - 2] = NODE_NUM
    if n == 1:
        s[0] = 6                                                   # the long row
    return s
