"""The rule of per-edge-type sampling (legion_etype_degrees .. legion_etype_sample_edges in include/legion_hip.h) restated in plain
numpy: the segments of a row by np.searchsorted, the slot count, the draw, Floyd's algorithm in a loop, the edge list.  Not a port of the
kernel.  A helper of the tests, not a test file."""
import numpy as np

U = np.uint64


def _mix(x):
    x = x + U(0x9E3779B97F4A7C15)
    x = (x ^ (x >> U(30))) * U(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> U(27))) * U(0x94D049BB133111EB)
    return x ^ (x >> U(31))


def draw(salt, row, t, k, R):
    """Slot k of the pair (row, t) draws from [0, R), R < 2^32; row, k and R may be arrays (int64 out)."""
    with np.errstate(over="ignore"):
        x = (np.asarray(row).astype(U) << U(32)) | U(t << 16) | np.asarray(k).astype(U)
        h = _mix(_mix(np.array(salt & (2 ** 64 - 1), dtype=U)) ^ x) >> U(32)
        return ((h * np.asarray(R).astype(U)) >> U(32)).astype(np.int64)


def slots(D, f, replace):
    if f == 0 or D == 0:
        return 0
    return D if f == -1 or (not replace and D <= f) else f


def pair_picks(salt, row, t, D, f, replace):
    """The positions inside the segment, of D entries, that the slots of the pair (row, t) pick, in slot order."""
    if slots(D, f, replace) == D:
        return list(range(D))
    k = np.arange(f)
    if replace:
        return draw(salt, row, t, k, D).tolist()
    picks = []
    for j, c in zip((D - f + k).tolist(), draw(salt, row, t, k, D - f + k + 1).tolist()):
        picks.append(j if c in picks else c)
    return picks


def segments(indptr, etype, r, T):
    """b[0 .. T] of row r, positions in col: segment t is [b[t], b[t + 1]).  A row outside the graph has empty segments at 0."""
    if not 0 <= r < indptr.size - 1:
        return np.zeros(T + 1, dtype=np.int64)
    lo, hi = int(indptr[r]), int(indptr[r + 1])
    return lo + np.searchsorted(etype[lo:hi], np.arange(T + 1), side="left").astype(np.int64)


def degrees(indptr, etype, rows, T):
    return np.stack([np.diff(segments(indptr, etype, int(r), T)) for r in rows]).reshape(len(rows), T)


def sample(indptr, col, etype, T, rows, fanouts, replace, salt, add=0):
    """(offsets [n + 1], dst, src, eid, etype) of the picks; add: what turns a position in col into the edge id."""
    dst, eid, ety, offsets = [], [], [], [0]
    for i, r in enumerate(rows):
        b = segments(indptr, etype, int(r), T)
        for t in range(T):
            picks = pair_picks(salt, int(r), t, int(b[t + 1] - b[t]), int(fanouts[t]), replace)
            dst += [i] * len(picks)
            eid += [int(b[t]) + p for p in picks]
            ety += [t] * len(picks)
        offsets.append(len(dst))
    eid = np.array(eid, dtype=np.int64)
    return np.array(offsets, dtype=np.int64), np.array(dst, dtype=np.int32), col[eid].astype(np.int32), eid + add, np.array(ety, dtype=np.uint8)
