"""PinSAGE's neighbour sampler (GraphStorage.pinsage_neighbors, legion_pinsage_neighbors) restated in numpy on the CPU over
tests/walk_ref.step, as the contract in include/legion_hip.h writes it: R walks per seed whose first step takes no restart draw, the
visits counted per seed, the k most visited by (count descending, vertex id ascending).  A helper of the tests, not a test file."""
import numpy as np

from tests import walk_ref

M31 = 2 ** 31 - 1
MAX_VISITS = 1024                                                  # LEGION_PINSAGE_MAX_VISITS


def refused(num_seeds, R, T, k, weighted, termination_prob, base, has_table):
    """True where legion_pinsage_neighbors returns -1 for these values (null pointers aside)."""
    if num_seeds < 0 or R < 1 or T < 1 or k < 1 or R * T > MAX_VISITS or k > MAX_VISITS:
        return True
    if base < 0 or base + num_seeds * R * T > M31:
        return True
    if weighted not in (0, 1) or (weighted == 1 and not has_table):
        return True
    p = np.float32(termination_prob)
    return not (p >= 0 and p <= 1)


def visits(indptr, col, seeds, R, T, table=None, termination_prob=0.5, base=0, reads=None, eids=None):
    """int32 [n, R * T]: entry [i, r * T + j - 1] is the vertex walk r of seed i reaches at step j, or -1 once the walk has ended.
    eids, if a list, collects per step the int64 [n * R] edge ids of the traversals (-1: no traversal; walk w = i * R + r)."""
    indptr = np.asarray(indptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int32)
    seeds = np.asarray(seeds, dtype=np.int32)
    n, node_num = seeds.size, indptr.size - 1
    W = n * R                                                      # walk w = i * R + r
    x = walk_ref.draws(base, W * T).reshape(W, T)                  # walk w, step j: draw index base + w * T + (j - 1)
    y = walk_ref.draws(base, W * T, 2 ** 31).reshape(W, T) if termination_prob > 0 else None
    v = np.repeat(seeds.astype(np.int64), R)
    out = np.full((W, T), -1, dtype=np.int32)
    for j in range(1, T + 1):
        if j == 1 or y is None:                                    # the first traversal takes no restart draw
            v, e = walk_ref.step(indptr, col, node_num, v, x[:, j - 1], table=table, reads=reads)
        else:
            v, e = walk_ref.step(indptr, col, node_num, v, x[:, j - 1], y[:, j - 1], table, termination_prob, reads)
        if eids is not None:
            eids.append(e)
        out[:, j - 1] = v
    return out.reshape(n, R * T)


def topk_loop(vis, k):
    """(neighbors, counts), int32 [n, k], of visit rows (entries < 0 are no visits): distinct vertices by count descending, id ascending;
    -1 / 0 past their number.  Row by row: the definition of topk."""
    n = vis.shape[0]
    nb = np.full((n, k), -1, dtype=np.int32)
    ct = np.zeros((n, k), dtype=np.int32)
    for i in range(n):
        row = vis[i][vis[i] >= 0]
        if row.size == 0:
            continue
        ids, c = np.unique(row, return_counts=True)               # ids ascending
        order = np.lexsort((ids, -c))[:k]
        nb[i, :order.size], ct[i, :order.size] = ids[order], c[order]
    return nb, ct


def topk(vis, k):
    """topk_loop over all rows at once: the rows sorted, run lengths from the run heads, one flat sort by (row, -count, id)
    packed in an int64."""
    vis = np.asarray(vis)
    n, V = vis.shape
    nb = np.full((n, k), -1, dtype=np.int32)
    ct = np.zeros((n, k), dtype=np.int32)
    if n == 0 or V == 0:
        return nb, ct
    s = np.sort(np.where(vis < 0, np.int64(2 ** 31), vis.astype(np.int64)), axis=1)      # no visit sorts last
    valid = (s < 2 ** 31).sum(axis=1)
    head = s < 2 ** 31
    head[:, 1:] &= s[:, 1:] != s[:, :-1]
    row, pos = np.nonzero(head)                                    # row-major: a row's heads are consecutive, positions ascending
    if row.size == 0:
        return nb, ct
    end = np.append(pos[1:], 0)
    last = np.append(row[1:] != row[:-1], True)                    # a row's last run ends where its visits do
    end[last] = valid[row[last]]
    count, ids = end - pos, s[row, pos]
    assert n < 2 ** 21 and V < 2 ** 11                              # one int64 key: row, V - count and id in 21, 11 and 31 bits
    key = np.sort((row.astype(np.int64) << 42) | ((V - count).astype(np.int64) << 31) | ids)
    row, count, ids = key >> 42, V - ((key >> 31) & 2047), key & (2 ** 31 - 1)
    first = np.nonzero(np.append(True, row[1:] != row[:-1]))[0]
    rank = np.arange(row.size) - np.repeat(first, np.diff(np.append(first, row.size)))
    keep = rank < k
    nb[row[keep], rank[keep]], ct[row[keep], rank[keep]] = ids[keep], count[keep]
    return nb, ct


def neighbors(indptr, col, seeds, R, T, k, table=None, termination_prob=0.5, base=0, reads=None, eids=None):
    return topk(visits(indptr, col, seeds, R, T, table, termination_prob, base, reads, eids), k)
