"""A vertex set and the subgraph it induces (engine.NodeSet, GraphStorage.induced_edges / node_subgraph; the C ABI's
legion_node_set_build, legion_node_set_lookup, legion_induced_count, legion_induced_edges, legion_dst_offsets) restated in numpy on the
CPU as the contracts in include/legion_hip.h write them: pos by a dict, the slots through in_edges_ref.in_edges and then the mask (as
labor_ref.slot_mask does), the row pointers by np.searchsorted(side="left").  And numpy models of wrong kernels, which must differ from
the reference on the GPU files' own inputs.  A helper of the tests, not a test file."""
import numpy as np

from tests import in_edges_ref, labor_ref, link_ref

MAX_ROWS = 2 ** 20                                                 # LEGION_IN_EDGES_MAX_ROWS
MAX_SLOTS = 2 ** 30                                                # LEGION_INDUCED_MAX_SLOTS
MAX_IDS = 2 ** 20                                                  # LEGION_NODE_SET_MAX_IDS
MAX_CAP = 2 ** 31 - 1
TILE, STRIP, GROUP, STRIDE = labor_ref.TILE, labor_ref.STRIP, labor_ref.GROUP, labor_ref.STRIDE


# ---- the refusals (null pointers aside) ---------------------------------------------------------------------------------------------
def set_bytes(k):
    """legion_node_set_bytes: int32 keys[S] then uint32 first[S], S = link_ref.table_slots(k); -1 for an illegal k."""
    if k < 0 or k > MAX_IDS:
        return -1
    return 8 * link_ref.table_slots(k)


def scratch_bytes(m):
    """legion_induced_scratch_bytes: LABOR's formula; -1 for an illegal m."""
    if m < 0 or m > MAX_SLOTS:
        return -1
    return labor_ref.scratch_bytes(m)


def refused(op, n=0, m=0, k=0, set_b=1 << 40, scratch=1 << 40, cap=0):
    """op: "build" (k, set_b), "lookup" (k, set_b, m), "count", "edges" or "dst_offsets" (cap, n)."""
    assert op in ("build", "lookup", "count", "edges", "dst_offsets")
    if op == "dst_offsets":
        return cap < 0 or cap > MAX_CAP or n < 0 or n > MAX_ROWS
    if op in ("count", "edges") and (n < 0 or n > MAX_ROWS or m < 0 or m > MAX_SLOTS):
        return True
    if k < 0 or k > MAX_IDS or set_b < set_bytes(k):
        return True
    if op == "build":
        return False
    if op == "lookup":
        return m < 0 or m > MAX_CAP
    if op == "edges" and (cap < 0 or cap > MAX_CAP):
        return True
    return scratch < scratch_bytes(m)


# ---- the set ------------------------------------------------------------------------------------------------------------------------
def positions(nodes, last=False):
    """v -> pos(v) for the non-negative entries of nodes: the first position (last: a wrong kernel's, the last)."""
    where = {}
    for j, v in enumerate(np.asarray(nodes).tolist()):
        if v >= 0 and (last or v not in where):
            where[v] = j
    return where


def distinct(nodes):
    return len(positions(nodes))


def pos(nodes, ids, last=False, lost=()):
    """int32 [m]: pos(ids[i]); lost: members a wrong table has lost."""
    where = positions(nodes, last)
    for v in lost:
        where.pop(int(v), None)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    out = np.full(ids.size, -1, dtype=np.int32)
    if where and ids.size:                                         # the dict, asked for every id at once
        keys = np.array(sorted(where), dtype=np.int64)
        vals = np.array([where[v] for v in keys.tolist()], dtype=np.int32)
        at = np.minimum(np.searchsorted(keys, ids), keys.size - 1)
        hit = (ids >= 0) & (keys[at] == ids)
        out[hit] = vals[at[hit]]
    return out


def lost_without_wrap(nodes, order=None):
    """The members a table that stops probing at its last slot loses (link_ref.probe_table(wrap=False)), for an arrival order."""
    nodes = np.asarray(nodes, dtype=np.int64)
    order = np.arange(nodes.size) if order is None else order
    slot = link_ref.probe_table(nodes, nodes.size, order, wrap=False)[0]
    return sorted(set(nodes[(slot < 0) & (nodes >= 0)].tolist()))


# ---- the edges ----------------------------------------------------------------------------------------------------------------------
def slot_mask(indptr, col, rows, offsets, m, nodes, reads=None, wrong=None, order=None):
    """(kept bool [m], dst, src_local, eid over the m slots, and the global src).  wrong: one of WRONG."""
    assert wrong is None or wrong in WRONG, wrong
    rows = np.asarray(rows, dtype=np.int64)
    if wrong == "e32":
        dst, src, eid = in_edges_ref.in_edges_e32(indptr, col, rows, offsets, m)
    else:
        dst, src, eid = in_edges_ref.in_edges(indptr, col, rows, offsets, m, reads)
    lost = lost_without_wrap(nodes, order) if wrong == "no-wrap" else ()
    local = pos(nodes, src, last=wrong == "last-position", lost=lost)
    kept = (eid >= 0) & (src >= 0) & (local >= 0)                  # 3.
    if wrong == "dead-matches-empty":
        kept |= (eid >= 0) & (src < 0)                             # kept, local -1
    if wrong == "member-of-dst":
        r = np.where(dst >= 0, rows[np.maximum(dst, 0)], -1)
        kept = (eid >= 0) & (src >= 0) & (pos(nodes, r) >= 0)
    if wrong == "global-src":
        local = src.copy()
    return kept, dst, local, eid, src


def count(indptr, col, rows, offsets, m, nodes):
    return int(slot_mask(indptr, col, rows, offsets, m, nodes)[0].sum())


def edges(indptr, col, rows, offsets, m, nodes, cap=None, reads=None, wrong=None, order=None):
    """(K, dst int32 [cap], src_local int32 [cap], eid int64 [cap]); cap None: K."""
    kept, dst, local, eid, _ = slot_mask(indptr, col, rows, offsets, m, nodes, reads, wrong, order)
    K = int(kept.sum())
    cap = K if cap is None else cap
    out = []
    for x in (dst, local, eid):
        y = np.full(cap, -1, dtype=x.dtype)
        y[:min(K, cap)] = x[kept][:cap]
        out.append(y)
    return (K,) + tuple(out)


def edges_full(indptr, col, rows, nodes, wrong=None):
    """(dst, src_local, eid) sized exactly K: what GraphStorage.induced_edges returns with return_eids."""
    offsets = in_edges_ref.row_offsets(indptr, rows)
    return edges(indptr, col, rows, offsets, int(offsets[-1]), nodes, wrong=wrong)[1:]


# ---- the row pointers ---------------------------------------------------------------------------------------------------------------
def dst_offsets(dst, cap, count, n, upper=False):
    """int64 [n + 1]: #{ p in [0, L) : dst[p] < i }, L = count clamped to [0, cap] (upper: a wrong kernel's, dst[p] <= i)."""
    L = min(max(int(count), 0), int(cap))
    d = np.asarray(dst, dtype=np.int64)[:L]
    return np.searchsorted(d, np.arange(n + 1, dtype=np.int64), side="right" if upper else "left").astype(np.int64)


def node_subgraph(indptr, col, nodes):
    """(indptr_sub int64 [k + 1], col_sub int32 [K], eids int64 [K]): what GraphStorage.node_subgraph returns with return_eids.  The
    nodes are distinct vertices of the graph (asserted)."""
    nodes = np.asarray(nodes, dtype=np.int32)
    assert np.unique(nodes).size == nodes.size and (nodes.size == 0 or (nodes.min() >= 0 and nodes.max() < len(indptr) - 1))
    dst, local, eid = edges_full(indptr, col, nodes, nodes)
    return dst_offsets(dst, dst.size, dst.size, nodes.size), local, eid


# ---- wrong kernels --------------------------------------------------------------------------------------------------------------------
# the last position of a repeated node (no atomicMin); a table that stops probing at its last slot; a dead entry matched against the
# empty key; the membership of dst's vertex instead of src's; the global src written; e in 32 bits.  Lane-major ranks and a stale second
# trip are labor_ref's, an upper-bound dst_offsets is dst_offsets(upper=True).
WRONG = ("last-position", "no-wrap", "dead-matches-empty", "member-of-dst", "global-src", "e32")
lane_major = labor_ref.lane_major
stale_second_trip = labor_ref.stale_second_trip


# ---- inputs of the tests ----------------------------------------------------------------------------------------------------------
def tile_counts(kept):
    return np.add.reduceat(kept.astype(np.int64), np.arange(0, kept.size, TILE)) if kept.size else np.zeros(0, np.int64)


def wave_counts(kept):
    pad = np.concatenate([kept, np.zeros(-kept.size % 64, bool)])
    return pad.reshape(-1, 64).sum(axis=1)


def wrap_set(node_num=6000, k=100):
    """A set of k nodes below node_num whose 256-slot table wraps: every id whose home lies in the last two slots, filled up to k with
    ids of other homes (the ids of the wrap first)."""
    ids = np.arange(node_num, dtype=np.int64)
    homes = link_ref.home_slots(ids, k)
    slots = link_ref.table_slots(k)
    last = ids[homes >= slots - 2]
    rest = ids[homes < slots - 2]
    return np.concatenate([last, rest[:k - last.size]]).astype(np.int32), last.astype(np.int32)
