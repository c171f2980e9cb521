"""legion_attention_rows (include/legion_hip.h) restated in numpy float64: the contract, not the kernel."""
import numpy as np


def attention(X, offsets, ids, queries=None, bias=None, scale=1.0, node_map=None, cache=None):
    """(out float64 [n, H, D], scores float64 [M, H], lse float64 [n, H], live int64 [n], mass float64 [n, H]: scale * sum |q x| of the
    segment's worst entry, for a bound).  X, cache: the tables' stored values; queries [n, H, D] or None; bias [M, H] or None."""
    N, n, D = X.shape[0], offsets.size - 1, X.shape[1]
    H = queries.shape[1] if queries is not None else bias.shape[1]
    out, scores, lse = np.zeros((n, H, D)), np.zeros((ids.size, H)), np.full((n, H), -np.inf)
    live, mass = np.zeros(n, np.int64), np.zeros((n, H))
    for d in range(n):
        e = np.arange(offsets[d], offsets[d + 1])
        e = e[(ids[e] >= 0) & (ids[e] < N)]
        if e.size == 0:
            continue                                                   # a row of zeros, lse -inf
        rows = X[ids[e]].astype(np.float64)
        if node_map is not None:
            hit = node_map[ids[e]] >= 0
            rows[hit] = cache[node_map[ids[e]][hit]]
        s = np.zeros((e.size, H))
        if queries is not None:
            q = queries[d].astype(np.float64)
            s += np.float64(np.float32(scale)) * (rows @ q.T)
            mass[d] = abs(float(np.float32(scale))) * (np.abs(rows) @ np.abs(q).T).max(axis=0)
        if bias is not None:
            s += bias[e].astype(np.float64)
        m = s.max(axis=0)
        p = np.exp(s - m)
        scores[e], lse[d], live[d] = s, m + np.log(p.sum(axis=0)), e.size
        out[d] = (p / p.sum(axis=0)).T @ rows
    return out, scores, lse, live, mass
