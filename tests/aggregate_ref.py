"""legion_aggregate_rows (include/legion_hip.h) restated in numpy float64: the contract, not the kernel."""
import numpy as np


def aggregate(X, offsets, ids, reduce="sum", weights=None, node_map=None, cache=None):
    """(float64 [n, D] sums or maxima before the mean's division, int64 [n] live entries).  X, cache: the tables' stored values."""
    N, n = X.shape[0], offsets.size - 1
    out, live = np.zeros((n, X.shape[1]), np.float64), np.zeros(n, np.int64)
    for d in range(n):
        e = np.arange(offsets[d], offsets[d + 1])
        e = e[(ids[e] >= 0) & (ids[e] < N)]
        if e.size == 0:
            continue                                                   # a row of zeros
        rows = X[ids[e]].astype(np.float64)
        if node_map is not None:
            hit = node_map[ids[e]] >= 0
            rows[hit] = cache[node_map[ids[e]][hit]]
        if weights is not None:
            rows = rows * weights[e].astype(np.float64)[:, None]
        out[d], live[d] = rows.max(axis=0) if reduce == "max" else rows.sum(axis=0), e.size
    return out, live


def final(out, live, reduce, bf16=False):
    """What out holds: float32, the mean by a correctly rounded float32 division; bf16: its round to nearest even, as float32."""
    v = out.astype(np.float32)
    if reduce == "mean":
        v = np.where(live[:, None] > 0, v / np.maximum(live, 1).astype(np.float32)[:, None], np.float32(0)).astype(np.float32)
    if bf16:
        u = v.view(np.uint32).astype(np.uint64)
        v = (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)
    return v
