"""Layer-neighbour sampling (GraphStorage.labor_edges / labor_block; the C ABI's legion_labor_count and legion_labor_edges) restated in
numpy on the CPU as the contract in include/legion_hip.h writes it: the hash through synth.splitmix64_np, the predicate in Python
integers, the slots through in_edges_ref.in_edges and then the mask, the block's relabelling through link_ref.unique_ids.  And numpy
models of wrong kernels, which must differ from the reference on the GPU files' own inputs.  A helper of the tests, not a test file."""
import numpy as np

from legion_amd.synth import splitmix64_np
from tests import in_edges_ref, link_ref

MAX_ROWS = 2 ** 20                                                 # LEGION_IN_EDGES_MAX_ROWS
MAX_SLOTS = 2 ** 30                                                # LEGION_LABOR_MAX_SLOTS
MAX_CAP = 2 ** 31 - 1
TILE = 1024                                                        # slots a workgroup takes at a time
STRIP = 256                                                        # consecutive slots of a tile that are ranked together
GROUP = 256                                                        # tiles per second-level sum
STRIDE = 2048 * TILE                                               # slots of one trip of the capped grid


# ---- the rule -----------------------------------------------------------------------------------------------------------------------
def u64(x):
    return int(x) & (2 ** 64 - 1)


def key(salt):
    return int(splitmix64_np(np.uint64(u64(salt))))


def hashes(v, salt, raw_key=False):
    """labor_hash(v, salt) for an array of non-negative int32 v: uint32 values in an int64 array."""
    k = u64(salt) if raw_key else key(salt)
    v = np.asarray(v, dtype=np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    return (splitmix64_np(np.uint64(k) ^ v) >> np.uint64(32)).astype(np.int64)


def keep_one(h, d, fanout):
    """labor_keep in Python integers."""
    return int(h) * int(d) < int(fanout) * 2 ** 32


def keeps(h, d, fanout):
    """labor_keep over arrays, exactly: floor(h d / 2^32) < fanout through the halves of d (every partial product fits uint64), or
    Python integers where some d is too large for that."""
    h, d = np.asarray(h, dtype=np.int64), np.asarray(d, dtype=np.int64)
    if h.size == 0:
        return np.zeros(h.shape, dtype=bool)
    if int(d.max()) >= 2 ** 62 or int(d.min()) < 0:
        return np.array([keep_one(a, b, fanout) for a, b in zip(h.tolist(), np.broadcast_to(d, h.shape).tolist())], dtype=bool)
    hu, du = h.astype(np.uint64), d.astype(np.uint64)
    top = hu * (du >> np.uint64(32)) + ((hu * (du & np.uint64(0xFFFFFFFF))) >> np.uint64(32))
    return top < np.uint64(fanout)


# ---- the refusals (null pointers aside) ---------------------------------------------------------------------------------------------
def tiles_of(m):
    return (m + TILE - 1) // TILE


def scratch_bytes(m):
    """legion_labor_scratch_bytes: one int64 per tile plus one, plus one per 256 tiles; -1 for an illegal m."""
    if m < 0 or m > MAX_SLOTS:
        return -1
    t = tiles_of(m)
    return 8 * (t + 1 + (t + GROUP - 1) // GROUP)


def refused(op, n, m, fanout, scratch=1 << 40, cap=0):
    """op: "count" or "edges"."""
    assert op in ("count", "edges")
    if n < 0 or n > MAX_ROWS or m < 0 or m > MAX_SLOTS or fanout < 1:
        return True
    if op == "edges" and (cap < 0 or cap > MAX_CAP):
        return True
    return scratch < scratch_bytes(m)


# ---- the ops ------------------------------------------------------------------------------------------------------------------------
def slot_mask(indptr, col, rows, offsets, m, fanout, salt, reads=None, hash_of="src", raw_key=False, keep=None, degree="row"):
    """(kept bool [m], dst, src, eid of in_edges over the m slots).  The keywords select the wrong kernels below."""
    indptr = np.asarray(indptr, dtype=np.int64)
    rows = np.asarray(rows, dtype=np.int64)
    dst, src, eid = in_edges_ref.in_edges(indptr, col, rows, offsets, m, reads)
    ok = (eid >= 0) & (src >= 0)
    at = np.nonzero(ok)[0]
    r = rows[dst[at]]
    d = indptr[r + 1] - indptr[r]                                  # 2. the row's whole degree
    if degree == "below-m":                                        # a wrong kernel: the slots of the row that lie below m
        off = np.asarray(offsets, dtype=np.int64)
        d = np.minimum(off[dst[at] + 1], m) - off[dst[at]]
    v = src[at] if hash_of == "src" else r
    h = hashes(v, salt, raw_key)
    kept = np.zeros(m, dtype=bool)
    kept[at] = (keep or keeps)(h, d, fanout)
    return kept, dst, src, eid


def count(indptr, col, rows, offsets, m, fanout, salt):
    return int(slot_mask(indptr, col, rows, offsets, m, fanout, salt)[0].sum())


def edges(indptr, col, rows, offsets, m, fanout, salt, cap=None, reads=None, **wrong):
    """(K, dst int32 [cap], src int32 [cap], eid int64 [cap]); cap None: K."""
    kept, dst, src, eid = slot_mask(indptr, col, rows, offsets, m, fanout, salt, reads, **wrong)
    K = int(kept.sum())
    cap = K if cap is None else cap
    out = []
    for x in (dst, src, eid):
        y = np.full(cap, -1, dtype=x.dtype)
        y[:min(K, cap)] = x[kept][:cap]
        out.append(y)
    return (K,) + tuple(out)


def edges_full(indptr, col, rows, fanout, salt):
    """(dst, src, eid) sized exactly K: what GraphStorage.labor_edges returns with return_eids."""
    offsets = in_edges_ref.row_offsets(indptr, rows)
    return edges(indptr, col, rows, offsets, int(offsets[-1]), fanout, salt)[1:]


def block(indptr, col, seeds, fanout, salt):
    """dict of input_nodes, dst_local, src_local, eids, and the global dst, src: what GraphStorage.labor_block returns.  The seeds are
    distinct vertices of the graph (asserted)."""
    seeds = np.asarray(seeds, dtype=np.int32)
    assert np.unique(seeds).size == seeds.size and (seeds.size == 0 or (seeds.min() >= 0 and seeds.max() < len(indptr) - 1))
    dst, src, eid = edges_full(indptr, col, seeds, fanout, salt)
    unique, local, cnt = link_ref.unique_ids(np.concatenate([seeds, src]))
    n = seeds.size
    assert np.array_equal(local[:n], np.arange(n))
    return dict(input_nodes=unique[:cnt], dst_local=dst, src_local=local[n:], eids=eid, dst=dst, src=src)


# ---- wrong kernels --------------------------------------------------------------------------------------------------------------------
# (Two more were modelled and dropped, because no input of the GPU files makes them differ: h * d truncated to 64 bits needs a row of
# more than 2^32 entries, and the far-row layouts' ballast rows have 2^20; the predicate in float32 differs where h / 2^32 lies within
# 2^-24 of fanout / d, which none of some five million slots does.  tests/cpu/labor_rule_test.cpp pins both sides of those edges.)
WRONG = {"raw-salt": dict(raw_key=True), "hash-of-dst": dict(hash_of="dst"), "degree-below-m": dict(degree="below-m")}


def lane_major(want, kept):
    """In-tile ranks in lane-major order: a lane's four slots (256 apart) one after another, lane by lane.  want: one of the exact
    outputs [K], kept: the mask over the m slots.  The tiles' bases are right, so the kept slots come tile by tile, and inside a tile
    in the wrong order."""
    m = kept.size
    order = np.arange(m + -m % TILE).reshape(-1, TILE // STRIP, STRIP).transpose(0, 2, 1).reshape(-1)      # slots, lane-major per tile
    order = order[order < m]
    pos = np.cumsum(kept) - 1                                      # kept slot -> its right position
    return np.asarray(want)[pos[order[kept[order]]]]


def stale_second_trip(kept):
    """A second grid trip that repeats the tile one stride earlier: the mask it would count."""
    out = np.array(kept, copy=True)
    out[STRIDE:] = kept[:out.size - STRIDE]
    return out
