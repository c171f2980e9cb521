"""Seed-edge exclusion (GraphStorage.reverse_edge_ids / seed_edge_exclusion, engine.EdgeIdSet, engine.exclude_edges and the block ops'
exclude_eids; the C ABI's legion_reverse_edge_ids, legion_edge_set_build, legion_edge_set_contains, legion_edge_filter_count and
legion_edge_filter_edges) restated in numpy on the CPU as the contracts in include/legion_hip.h write them: the reverse of an edge is
one np.searchsorted over the packed (row, col) keys of the live entries in edge order -- independent of how rows are sorted, which is
what lets it judge both search paths; membership is np.isin over the non-negative ids; the filter is one boolean mask.  Beside them the
set's table as legion_amd/csrc/exclude_rule.h has it, inputs whose home slots cluster, and numpy models of wrong kernels, which must
differ from the reference on the GPU files' own inputs.  A helper of the tests, not a test file."""
import numpy as np

from tests import reverse_ref

SET_MAX_IDS = 2 ** 21                                              # LEGION_EDGE_SET_MAX_IDS
FILTER_MAX_EDGES = 2 ** 30                                         # LEGION_EDGE_FILTER_MAX_EDGES
HASH = 0x9E3779B97F4A7C15                                          # odd: a bijection mod 2^64
HASH_INV = pow(HASH, -1, 2 ** 64)
IDS_TILE = 4 * 256                                                 # edge ids a workgroup of reverse_edge_ids takes at a time
IDS_STRIDE = 2048 * IDS_TILE                                       # edge ids of one trip of its capped grid
TILE = 1024                                                        # entries a workgroup of the filter takes at a time
STRIDE = 2048 * TILE                                               # entries of one trip of the filter's capped grid
ITEM_STRIDE = 2048 * 256                                           # ids of one trip of the set's insert and contains


# ---- reverse edge ids -------------------------------------------------------------------------------------------------------------------
def reverse_edge_ids(indptr, col, eids):
    """int64 [n]: for e = eids[i], the least e' in row col[e] with col[e'] == row(e); -1 for an e outside [0, E), for a dead entry or
    one outside the graph, and where there is none."""
    indptr, col = np.asarray(indptr, dtype=np.int64), np.asarray(col, dtype=np.int32)
    e = np.asarray(eids, dtype=np.int64)
    N = indptr.size - 1
    out = np.full(e.size, -1, dtype=np.int64)
    live = reverse_ref.live_entries(indptr, col)                   # ascending
    rows = reverse_ref.rows_of(indptr, live).astype(np.int64)
    keep = rows >= 0
    live, rows = live[keep], rows[keep]
    key = rows * (N + 1) + col[live]                               # (row, col) of every live entry
    order = np.argsort(key, kind="stable")                         # equal keys in ascending e: the first is the least
    skey, se = key[order], live[order]
    at = np.nonzero((e >= 0) & (e < col.size))[0]                  # 1. before any load
    u = col[e[at]].astype(np.int64)
    ok = (u >= 0) & (u < N)                                        # 2. dead, or outside the graph
    at, u = at[ok], u[ok]
    v = reverse_ref.rows_of(indptr, e[at]).astype(np.int64)        # 3.
    ok = v >= 0
    at, u, v = at[ok], u[ok], v[ok]
    want = u * (N + 1) + v                                         # 4. an entry of row u that names v
    pos = np.searchsorted(skey, want, side="left")
    hit = pos < skey.size
    hit[hit] = skey[pos[hit]] == want[hit]
    out[at[hit]] = se[pos[hit]]
    return out


def reverse_loop(indptr, col, eids):
    """The definition, entry by entry."""
    N = len(indptr) - 1
    out = []
    for e in np.asarray(eids).tolist():
        r = -1
        if 0 <= e < len(col) and 0 <= col[e] < N:
            u = int(col[e])
            v = [w for w in range(N) if indptr[w] <= e < indptr[w + 1]]
            if v:
                found = [x for x in range(int(indptr[u]), int(indptr[u + 1])) if col[x] == v[0]]
                r = found[0] if found else -1
        out.append(r)
    return np.array(out, dtype=np.int64)


def reverse_refused(n, via, rows_sorted, built):
    """rows_sorted: 1, 0, or -1 (never checked)."""
    if n < 0 or n > 2 ** 31 - 1 or via not in (0, 1):
        return True
    return rows_sorted != 1 if via == 0 else not built


def figures(indptr, col):
    """What the issue's table lists of a graph: entries, live, live without a reverse, self-loops, rev(rev(e)) != e, the longest row."""
    indptr, col = np.asarray(indptr, dtype=np.int64), np.asarray(col, dtype=np.int32)
    e = np.arange(col.size, dtype=np.int64)
    rev = reverse_edge_ids(indptr, col, e)
    live = reverse_ref.live_entries(indptr, col)
    rows = reverse_ref.rows_of(indptr, e)
    back = reverse_edge_ids(indptr, col, rev)
    loops = np.nonzero((rows == col) & (col >= 0))[0]
    return dict(entries=int(col.size), live=int(live.size), no_reverse=int((rev[live] < 0).sum()), loops=int(loops.size),
                loops_fixed=int((rev[loops] == loops).sum()), not_involution=int(((rev >= 0) & (back != e)).sum()),
                longest=int(np.diff(indptr).max()))


# ---- the set ----------------------------------------------------------------------------------------------------------------------------
def set_slots(k):
    s = 256
    while s < 2 * k:
        s *= 2
    return s


def set_bytes(k):
    return 8 * set_slots(k) if 0 <= k <= SET_MAX_IDS else -1


def home_slots(ids, k):
    """The slot at which the set of k ids starts probing for each non-negative id: the top log2 S bits of id * HASH mod 2^64."""
    bits = set_slots(k).bit_length() - 1
    with np.errstate(over="ignore"):
        return ((np.asarray(ids, dtype=np.int64).astype(np.uint64) * np.uint64(HASH)) >> np.uint64(64 - bits)).astype(np.int64)


def contains(members, ids):
    """int32 [m] of 0 / 1: ids[i] >= 0 and occurs in members."""
    members, ids = np.asarray(members, dtype=np.int64), np.asarray(ids, dtype=np.int64)
    return ((ids >= 0) & np.isin(ids, members[members >= 0])).astype(np.int32)


def ids_with_home(k, homes, per, high=0):
    """`per` distinct non-negative int64 ids for each home slot in `homes` of the set of k ids, home by home: the hash inverted, as
    link_ref.ids_with_home does for the 32-bit table.  y = id * HASH mod 2^64 has home y >> shift, so the ids of a home are
    y * HASH_INV mod 2^64 over y in the home's range; those below 2^63 are kept (high: and at or above it -- ids past 2^32 on demand)."""
    slots = set_slots(k)
    shift = 64 - (slots.bit_length() - 1)
    out = []
    for home in homes:
        assert 0 <= home < slots, (home, slots)
        got, y = [], home << shift
        while len(got) < per:
            i = (y * HASH_INV) % 2 ** 64
            if high <= i < 2 ** 63:
                got.append(i)
            y += 1
            assert y < (home + 1) << shift
        out += got
    out = np.array(out, dtype=np.int64)
    assert np.array_equal(home_slots(out, k), np.repeat(np.asarray(homes, dtype=np.int64), per)) and np.unique(out).size == out.size
    return out


def probe_lengths(members, k):
    """(the longest probe run of an insert in index order, how many keys sit below their home: wraps).  A statement about inputs."""
    slots = set_slots(k)
    table, longest, wraps = {}, 0, 0
    seen = set()
    for e, h in zip(np.asarray(members).tolist(), home_slots(np.maximum(members, 0), k).tolist()):
        if e < 0 or e in seen:
            continue
        seen.add(e)
        s, run = h, 1
        while s in table:
            s, run = (s + 1) % slots, run + 1
        table[s] = e
        longest, wraps = max(longest, run), wraps + int(s < h)
    return longest, wraps


# ---- the filter -------------------------------------------------------------------------------------------------------------------------
def kept_mask(dst, eid, members):
    return (np.asarray(dst) >= 0) & (contains(members, eid) == 0)


def exclude_edges(dst, src, eid, members, cap=None):
    """(dst_out int32 [cap], src_out int32 [cap], eid_out int64 [cap], K): the kept triples in order, -1 from K on; cap None: K."""
    dst, src, eid = np.asarray(dst, dtype=np.int32), np.asarray(src, dtype=np.int32), np.asarray(eid, dtype=np.int64)
    keep = kept_mask(dst, eid, members)
    K = int(keep.sum())
    cap = K if cap is None else cap
    out = [np.full(cap, -1, dtype=a.dtype) for a in (dst, src, eid)]
    for o, a in zip(out, (dst, src, eid)):
        o[:min(K, cap)] = a[keep][:cap]
    return out[0], out[1], out[2], K


def filter_refused(m, k, set_bytes_, scratch, cap=0):
    if m < 0 or m > FILTER_MAX_EDGES or k < 0 or k > SET_MAX_IDS or set_bytes_ < set_bytes(k) or cap < 0 or cap > 2 ** 31 - 1:
        return True
    tiles = (m + 1023) // 1024
    return scratch < 8 * (tiles + 1 + (tiles + 255) // 256)


def seed_exclusion(indptr, col, seeds, exclude):
    """The ids GraphStorage.seed_edge_exclusion puts into its set."""
    seeds = np.asarray(seeds, dtype=np.int64)
    if exclude == "self":
        return seeds
    assert exclude == "reverse_id"
    return np.concatenate([seeds, reverse_edge_ids(indptr, col, seeds)])


def block_of(seeds, dst, src, eid, members):
    """A block op's result with exclude_eids, composed in numpy from its result without: (input_nodes, dst, src_local, eid) -- the
    filter, then unique_ids over [seeds | src] in order of first appearance (dst indexes the seeds)."""
    from tests import link_ref
    d, s, e, K = exclude_edges(dst, src, eid, members)
    unique, local, U = link_ref.unique_ids(np.concatenate([np.asarray(seeds, dtype=np.int32), s]))
    return unique[:U], d, local[len(seeds):], e


# ---- wrong kernels ----------------------------------------------------------------------------------------------------------------------
def _low32(x):
    return np.asarray(x, dtype=np.int64) & 0xFFFFFFFF


def contains_key32(members, ids):
    """A key cut to 32 bits: an id is a member when its low half is some member's."""
    members, ids = np.asarray(members, dtype=np.int64), np.asarray(ids, dtype=np.int64)
    return ((ids >= 0) & np.isin(_low32(ids), _low32(members[members >= 0]))).astype(np.int32)


def home_slots_hash32(ids, k):
    """A hash cut to 32 bits: the 32-bit table's home of the id's low half."""
    bits = set_slots(k).bit_length() - 1
    return ((_low32(ids) * 2654435769) & 0xFFFFFFFF) >> (32 - bits)


def reverse_e32(indptr, col, eids):
    """The answer formed in 32 bits."""
    r = reverse_edge_ids(indptr, col, eids)
    return np.where(r >= 0, ((r + 2 ** 31) % 2 ** 32) - 2 ** 31, -1)


def reverse_first_probed(indptr, col, eids):
    """The first match a binary search meets instead of the least e': the classic search that stops at equality."""
    indptr, col = np.asarray(indptr, dtype=np.int64), np.asarray(col, dtype=np.int32)
    out = reverse_edge_ids(indptr, col, eids)
    for i in np.nonzero(out >= 0)[0].tolist():
        e = int(np.asarray(eids)[i])
        u, v = int(col[e]), int(reverse_ref.rows_of(indptr, np.array([e]))[0])
        lo, hi = int(indptr[u]), int(indptr[u + 1])
        row = col[lo:hi]
        if not np.all(row[1:] >= row[:-1]):
            continue                                               # (an unsorted row: the model says nothing)
        a, b = 0, row.size
        while a < b:
            mid = (a + b) // 2
            if row[mid] == v:
                out[i] = lo + mid
                break
            if row[mid] < v:
                a = mid + 1
            else:
                b = mid
    return out


def reverse_dead_given(indptr, col, eids):
    """A dead or out-of-graph entry given a reverse: its col taken modulo N (-1 wraps to the last vertex)."""
    indptr, col = np.asarray(indptr, dtype=np.int64), np.asarray(col, dtype=np.int32)
    N = indptr.size - 1
    wrapped = np.where((col < 0) | (col >= N), np.mod(col.astype(np.int64), max(N, 1)), col).astype(np.int32)
    e = np.asarray(eids, dtype=np.int64)
    out = reverse_edge_ids(indptr, col, e)
    bad = np.nonzero((e >= 0) & (e < col.size))[0]
    bad = bad[(col[e[bad]] < 0) | (col[e[bad]] >= N)]
    u = wrapped[e[bad]].astype(np.int64)
    v = reverse_ref.rows_of(indptr, e[bad])
    for i, uu, vv in zip(bad.tolist(), u.tolist(), v.tolist()):
        found = np.nonzero(col[indptr[uu]:indptr[uu + 1]] == vv)[0]
        out[i] = int(indptr[uu]) + int(found[0]) if found.size else -1
    return out


def stale_second_trip(values, stride):
    """A second grid trip that reads the inputs one stride earlier again: what lies past the stride is answered as what lies a stride
    before it."""
    values = np.asarray(values)
    out = values.copy()
    out[stride:] = values[:values.size - stride]
    return out


def exclude_unstable(dst, src, eid, members, cap=None):
    """An unstable compaction: every tile's kept entries in reverse order."""
    d, s, e, K = exclude_edges(dst, src, eid, members, cap)
    keep = kept_mask(dst, eid, members)
    per_tile = np.add.reduceat(keep.astype(np.int64), np.arange(0, max(keep.size, 1), TILE)) if keep.size else np.zeros(0, np.int64)
    at = 0
    for c in per_tile.tolist():
        a, b = min(at, d.size), min(at + c, d.size, K)
        for o in (d, s, e):
            o[a:b] = o[a:b][::-1].copy()
        at += c
    return d, s, e, K


def exclude_tail_unfilled(dst, src, eid, members, cap, poison=7):
    """A tail not filled: [K, cap) keeps what the buffers held."""
    d, s, e, K = exclude_edges(dst, src, eid, members, cap)
    for o in (d, s, e):
        o[K:] = poison
    return d, s, e, K
