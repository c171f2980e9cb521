"""A neighbourhood taken whole (GraphStorage.row_offsets / in_edges / full_neighbor_block; the C ABI's legion_row_offsets and
legion_in_edges) restated in numpy on the CPU as the contracts in include/legion_hip.h write them: the offsets are np.cumsum over the
degrees, the row of a slot is np.searchsorted(side="right") over the offsets, the block's relabelling is link_ref.unique_ids.  And numpy
models of wrong kernels, which must differ from the reference on the GPU files' own inputs.  A helper of the tests, not a test file."""
import numpy as np

from tests import link_ref

MAX_ROWS = 2 ** 20                                                 # LEGION_IN_EDGES_MAX_ROWS
MAX_SLOTS = 2 ** 31 - 1
TILE = 1024                                                        # slots a workgroup takes at a time
STRIDE = 2048 * TILE                                               # slots of one trip of the capped grid
ROW_TILE = 256                                                     # rows per tile of the offsets kernels
ROW_STRIDE = 2048 * ROW_TILE
STAGE = TILE + 1                                                   # offsets a tile stages in LDS at most


# ---- the refusals (null pointers aside) ---------------------------------------------------------------------------------------------
def scratch_bytes(n):
    """legion_row_offsets_scratch_bytes: one int64 per tile of 256 rows; -1 for an illegal n."""
    if n < 0 or n > MAX_ROWS:
        return -1
    return 8 * ((n + ROW_TILE - 1) // ROW_TILE)


def refused(op, n, m=0, scratch=1 << 40):
    """op: "row_offsets" (n, scratch bytes) or "in_edges" (n, m)."""
    if n < 0 or n > MAX_ROWS:
        return True
    if op == "row_offsets":
        return scratch < scratch_bytes(n)
    assert op == "in_edges"
    return m < 0 or m > MAX_SLOTS


# ---- the ops ------------------------------------------------------------------------------------------------------------------------
def degrees(indptr, rows, reads=None):
    indptr = np.asarray(indptr, dtype=np.int64)
    rows = np.asarray(rows, dtype=np.int64)
    deg = np.zeros(rows.size, dtype=np.int64)
    ok = (rows >= 0) & (rows < indptr.size - 1)                    # else: no memory is read for r
    if reads is not None:
        reads.setdefault("indptr", []).extend([rows[ok].copy(), rows[ok] + 1])
    deg[ok] = indptr[rows[ok] + 1] - indptr[rows[ok]]
    return deg


def row_offsets(indptr, rows, reads=None):
    """int64 [n + 1]."""
    return np.concatenate([[0], np.cumsum(degrees(indptr, rows, reads))]).astype(np.int64)


def _expand(indptr, col, rows, offsets, m, i, reads=None, e32=False):
    """Rules 2 - 4 of legion_in_edges for slots 0 .. m - 1 whose search gave i."""
    indptr = np.asarray(indptr, dtype=np.int64)
    if isinstance(col, (list, tuple, np.ndarray)):                 # (else: something indexed like col that the host cannot hold)
        col = np.asarray(col, dtype=np.int32)
    rows, offsets = np.asarray(rows, dtype=np.int64), np.asarray(offsets, dtype=np.int64)
    n, N = rows.size, indptr.size - 1
    p = np.arange(m, dtype=np.int64)
    dst, src, eid = np.full(m, -1, np.int32), np.full(m, -1, np.int32), np.full(m, -1, np.int64)
    at = np.nonzero((i >= 0) & (i < n))[0]
    r = rows[i[at]]
    keep = (r >= 0) & (r < N)
    at, r = at[keep], r[keep]
    j = p[at] - offsets[i[at]]
    keep = (j >= 0) & (j < indptr[r + 1] - indptr[r])
    at, r, j = at[keep], r[keep], j[keep]
    e = indptr[r] + j
    if e32:                                                        # a wrong kernel: e through a signed 32-bit value
        e = ((e + 2 ** 31) % 2 ** 32) - 2 ** 31
        keep = (e >= 0) & (e < col.size)
        at, e = at[keep], e[keep]
    if reads is not None:
        reads.setdefault("indptr", []).extend([r.copy(), r + 1])
        reads.setdefault("col", []).append(e.copy())
    dst[at], src[at], eid[at] = i[at], col[e], e
    return dst, src, eid


def in_edges(indptr, col, rows, offsets, m, reads=None):
    """(dst int32 [m], src int32 [m], eid int64 [m]) for non-decreasing offsets (of any values)."""
    offsets = np.asarray(offsets, dtype=np.int64)
    assert np.all(np.diff(offsets) >= 0), "the search is specified for non-decreasing offsets"
    i = np.searchsorted(offsets, np.arange(m, dtype=np.int64), side="right") - 1      # 1. #{v : offsets[v] <= p} - 1
    return _expand(indptr, col, rows, offsets, m, i, reads)


def in_edges_full(indptr, col, rows):
    """(offsets, dst, src, eid) sized exactly M: what GraphStorage.in_edges returns."""
    offsets = row_offsets(indptr, rows)
    return (offsets,) + in_edges(indptr, col, rows, offsets, int(offsets[-1]))


def consistent(indptr, col, rows, offsets, dst, src, eid):
    """Rule 4 for offsets of any kind: every slot is -1 / -1 / -1 or entry p - offsets[i] of row rows[i]."""
    indptr, col, rows, offsets = (np.asarray(x) for x in (indptr, col, rows, offsets))
    none = dst < 0
    if not (np.all(src[none] == -1) and np.all(eid[none] == -1)):
        return False
    p = np.nonzero(~none)[0]
    i = dst[p].astype(np.int64)
    if np.any(i >= rows.size):
        return False
    r = rows[i].astype(np.int64)
    if np.any((r < 0) | (r >= indptr.size - 1)):
        return False
    j = p - offsets[i]
    return bool(np.all((j >= 0) & (j < indptr[r + 1] - indptr[r]) & (eid[p] == indptr[r] + j)) and np.array_equal(src[p], col[eid[p]]))


def full_neighbor_block(indptr, col, seeds):
    """dict of input_nodes, dst_local, src_local, offsets, eids, and the global dst, src: what GraphStorage.full_neighbor_block returns.
    The seeds are distinct vertices of the graph (asserted)."""
    seeds = np.asarray(seeds, dtype=np.int32)
    assert np.unique(seeds).size == seeds.size and (seeds.size == 0 or (seeds.min() >= 0 and seeds.max() < len(indptr) - 1))
    offsets, dst, src, eid = in_edges_full(indptr, col, seeds)
    unique, local, count = link_ref.unique_ids(np.concatenate([seeds, src]))
    n = seeds.size
    assert np.array_equal(local[:n], np.arange(n))
    return dict(input_nodes=unique[:count], dst_local=dst, src_local=local[n:], offsets=offsets, eids=eid, dst=dst, src=src)


# ---- wrong kernels --------------------------------------------------------------------------------------------------------------------
def in_edges_lower_bound(indptr, col, rows, offsets, m):
    """The slot's row by a lower bound: the first v with offsets[v] >= p, one less where that offset is past p.  Right except where p
    starts a row that follows empty rows: there it names the first of the empty rows, whose span holds no position 0."""
    offsets = np.asarray(offsets, dtype=np.int64)
    p = np.arange(m, dtype=np.int64)
    pos = np.searchsorted(offsets, p, side="left")
    i = np.where(offsets[np.minimum(pos, offsets.size - 1)] == p, pos, pos - 1)
    i = np.where(pos >= offsets.size, offsets.size - 1, i)
    return _expand(indptr, col, rows, offsets, m, i)


def stale_second_trip(want, stride):
    """A second grid trip that repeats the tile one stride earlier."""
    out = np.array(want, copy=True)
    out[stride:] = want[:out.size - stride]
    return out


def in_edges_e32(indptr, col, rows, offsets, m):
    """e formed in 32 bits."""
    offsets = np.asarray(offsets, dtype=np.int64)
    i = np.searchsorted(offsets, np.arange(m, dtype=np.int64), side="right") - 1
    return _expand(indptr, col, rows, offsets, m, i, e32=True)


def row_offsets_int32_tiles(indptr, rows):
    """A scan whose tile sums (and their prefix sums) are int32."""
    deg = degrees(indptr, rows)
    pad = np.concatenate([deg, np.zeros(-deg.size % ROW_TILE, np.int64)]).reshape(-1, ROW_TILE)
    wrap = lambda x: ((x + 2 ** 31) % 2 ** 32) - 2 ** 31
    tiles = wrap(pad.sum(axis=1))
    base = np.zeros(tiles.size + 1, dtype=np.int64)
    for t in range(tiles.size):
        base[t + 1] = wrap(base[t] + tiles[t])
    inner = np.cumsum(pad, axis=1) - pad
    out = (inner + base[:-1, None]).reshape(-1)[:deg.size]
    return np.concatenate([out, [base[-1]]]).astype(np.int64)


# ---- inputs of the tests --------------------------------------------------------------------------------------------------------------
def tile_ranges(offsets, m):
    """Per tile of 1 024 slots, the entries of offsets its range holds (the first row it touches up to the closing offset of the last):
    above STAGE the kernel searches global memory."""
    offsets = np.asarray(offsets, dtype=np.int64)
    n = offsets.size - 1
    p0 = np.arange(0, m, TILE, dtype=np.int64)
    p1 = np.minimum(p0 + TILE - 1, m - 1)
    a = np.maximum(np.searchsorted(offsets, p0, side="right") - 1, 0)
    b = np.minimum(np.searchsorted(offsets, p1, side="right"), n)
    return b - a + 1
