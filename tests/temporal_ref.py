"""The rule of temporal neighbour sampling (legion_temporal_sample_count, legion_temporal_sample_edges in include/legion_hip.h) restated
in plain numpy: the candidates of a row by a boolean mask, their ranks by np.flatnonzero, the draw of tests/etype_ref.py, Floyd's algorithm
in a loop.  It knows no classes: sorted or not, a rank is an index into the candidates' positions.  Not a port of the kernel.  A helper of
the tests, not a test file."""
import numpy as np

from tests.etype_ref import draw, slots

UNIFORM, LAST = 0, 1


def candidates(indptr, time, r, bound):
    """The positions in col of the candidates of row r observed at bound, in CSR order; none for a row outside the graph."""
    if not 0 <= r < indptr.size - 1:
        return np.zeros(0, dtype=np.int64)
    lo, hi = int(indptr[r]), int(indptr[r + 1])
    return lo + np.flatnonzero(time[lo:hi] < bound).astype(np.int64)


def ranks(salt, row, C, f, strategy, replace):
    """The ranks among a row's C candidates that its slots pick, in slot order."""
    s = slots(C, f, replace)
    if strategy == LAST or s == C:
        return list(range(C - s, C))
    k = np.arange(f)
    if replace:
        return draw(salt, row, 0, k, C).tolist()
    picks = []
    for j, c in zip((C - f + k).tolist(), draw(salt, row, 0, k, C - f + k + 1).tolist()):
        picks.append(j if c in picks else c)
    return picks


def degrees(indptr, time, rows, bounds):
    return np.array([candidates(indptr, time, int(r), int(b)).size for r, b in zip(rows, bounds)], dtype=np.int64)


def sample(indptr, col, time, rows, bounds, fanout, strategy, replace, salt, add=0):
    """(cand [n], offsets [n + 1], dst, src, eid, time) of the picks; add: what turns a position in col into the edge id."""
    dst, eid, cand, offsets = [], [], [], [0]
    for i, (r, b) in enumerate(zip(rows, bounds)):
        at = candidates(indptr, time, int(r), int(b))
        picks = at[ranks(salt, int(r), at.size, fanout, strategy, replace)] if at.size else at
        cand.append(at.size)
        dst += [i] * picks.size
        eid += picks.tolist()
        offsets.append(len(dst))
    eid = np.array(eid, dtype=np.int64)
    return (np.array(cand, dtype=np.int64), np.array(offsets, dtype=np.int64), np.array(dst, dtype=np.int32), col[eid].astype(np.int32),
            eid + add, time[eid].astype(np.int64))
