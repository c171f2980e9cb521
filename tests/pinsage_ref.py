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


def visits(indptr, col, seeds, R, T, table=None, termination_prob=0.5, base=0, reads=None):
    """int32 [n, R * T]: entry [i, r * T + j - 1] is the vertex walk r of seed i reaches at step j, or -1 once the walk has ended."""
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
            v, _ = walk_ref.step(indptr, col, node_num, v, x[:, j - 1], table=table, reads=reads)
        else:
            v, _ = walk_ref.step(indptr, col, node_num, v, x[:, j - 1], y[:, j - 1], table, termination_prob, reads)
        out[:, j - 1] = v
    return out.reshape(n, R * T)


def topk(vis, k):
    """(neighbors, counts), int32 [n, k], of visit rows (entries < 0 are no visits): distinct vertices by count descending, id ascending;
    -1 / 0 past their number."""
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


def neighbors(indptr, col, seeds, R, T, k, table=None, termination_prob=0.5, base=0, reads=None):
    return topk(visits(indptr, col, seeds, R, T, table, termination_prob, base, reads), k)
