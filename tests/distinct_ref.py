"""Sampling without replacement (MemoryPool replace = 0) restated in numpy on the CPU: the picks, and one whole batch as the
oracle's lgo_run_batch computes it with these picks in place of its draws (first touch in slot order, cumulative blocks,
counters through the oracle's own lgo_counter_update).  A helper of the tests, not a test file."""
import ctypes

import numpy as np

from oracle import ffi

C = 3                      # INTRABATCH_CON
M31 = 2147483647
_A = 48271


def _tables():
    t0 = np.empty(2048, np.uint64); t1 = np.empty(2048, np.uint64); t2 = np.empty(1024, np.uint64)
    v = 1
    for i in range(2048):
        t0[i] = v; v = v * _A % M31
    s1, v = v, 1
    for i in range(2048):
        t1[i] = v; v = v * s1 % M31
    s2, v = v, 1
    for i in range(1024):
        t2[i] = v; v = v * s2 % M31
    return t0, t1, t2


_T0, _T1, _T2 = _tables()


def minstd_pow(n):
    """48271^n mod 2^31-1, vectorised (n < 2^32)."""
    n = np.asarray(n, dtype=np.uint64)
    x = _T0[n & np.uint64(2047)] * _T1[(n >> np.uint64(11)) & np.uint64(2047)] % np.uint64(M31)
    return x * _T2[n >> np.uint64(22)] % np.uint64(M31)


def draw(idx, n):
    """The sampler's draw(idx, n) (oracle lgo_draw): uniform_int_distribution(0, n-1) over minstd_rand at position idx + 1."""
    x = minstd_pow(np.asarray(idx, dtype=np.int64).astype(np.uint64) + np.uint64(1))
    r = (x - np.uint64(1)).astype(np.float64) / 2147483646.0
    return (r * ((np.asarray(n, dtype=np.float64) - 1.0) + 1.0)).astype(np.int32)


def picks(base, deg, f):
    """Adjacency positions [n, f] of n frontier entries (first slot base[i] = q*f, degree deg[i]); -1 for k >= min(f, D)."""
    base = np.asarray(base, dtype=np.int64)
    D = np.maximum(np.asarray(deg, dtype=np.int64), 0)
    n = base.size
    k = np.arange(f, dtype=np.int64)[None, :]
    out = np.where(k < D[:, None], k, -1).astype(np.int32)
    big = np.nonzero(D > f)[0]
    if big.size:
        j = D[big, None] - f + k                               # j_k = D - f + k
        t = draw(base[big, None] + k, j + 1)
        p = np.empty_like(t)
        for kk in range(f):
            taken = np.any(p[:, :kk] == t[:, kk:kk + 1], axis=1) if kk else np.zeros(big.size, bool)
            p[:, kk] = np.where(taken, j[:, kk], t[:, kk])
        out[big] = p
    return out


def counter_update(nc, ec, op, size=0, hop_num=0):
    L = ffi.load()
    L.lgo_counter_update(nc.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ec.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                         int(op), int(size), int(hop_num))


def run_batch(indptr, col, all_ids, all_labels, batch_size, counter, fanout, serve=True, edge_access=None, node_access=None):
    """One batch in distinct mode, laid out as OraclePool.read_batch.  serve: the batch's gathers run (ops 3h+1 update the counters
    too; PreSC runs without them).  edge_access / node_access: PreSC's hotness counts, added to in place (train mode)."""
    indptr = np.asarray(indptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int32)
    total_cap = int(len(all_ids))
    hop_num = len(fanout)
    nc = np.zeros(16, np.int32); ec = np.zeros(16, np.int32)
    size = total_cap - batch_size * counter if batch_size * (counter + 1) >= total_cap else batch_size
    ids, labels, pos = [], [], {}
    for idx in range(max(size, 0)):
        at = size * counter + idx
        if at >= total_cap:
            ids.append(-1); labels.append(-1)
        else:
            v = int(all_ids[at % total_cap])
            ids.append(v); labels.append(int(all_labels[at % total_cap])); pos[v] = idx
    counter_update(nc, ec, 0, size, hop_num)
    if serve:
        counter_update(nc, ec, 1)
    src_ids, dst_ids = [], []
    for h, f in enumerate(fanout):
        op = C * (h + 1)
        frontier = np.array(ids[:max(int(nc[1]), 0)] if h == 0 else src_ids[ec[0]:ec[0] + ec[1]], dtype=np.int64)
        n_new = n_edge = 0
        if frontier.size:
            real = frontier >= 0
            fr = np.where(real, frontier, 0)
            D = np.where(real, indptr[fr + 1] - indptr[fr], 0)
            P = picks(np.arange(frontier.size, dtype=np.int64) * f, D, f)
            q, k = np.nonzero(P >= 0)                              # slot order: q-major, k-minor
            nb = col[indptr[fr[q]] + P[q, k]]
            for s, d in zip(frontier[q].tolist(), nb.tolist()):
                if d < 0:
                    continue
                if edge_access is not None:
                    edge_access[s] += 1
                if d not in pos:
                    pos[d] = len(ids); ids.append(d); n_new += 1
                src_ids.append(d); dst_ids.append(s); n_edge += 1
        nc[C * 2] += n_new
        ec[2] += n_edge
        counter_update(nc, ec, op)
        if serve:
            counter_update(nc, ec, op + 1)
    n_nodes = max(int(nc[C * 3 + hop_num]), 0)
    n_edges = max(int(ec[C * 3 + hop_num]), 0)
    if node_access is not None:
        for v in ids[:int(nc[C * 2 + 1])]:
            if v >= 0:
                node_access[v] += 1
    src = np.array(src_ids[:n_edges], dtype=np.int32)
    dst = np.array(dst_ids[:n_edges], dtype=np.int32)
    return {"node_counter": nc, "edge_counter": ec, "hop_num": hop_num,
            "sampled_ids": np.array(ids[:n_nodes], dtype=np.int32),
            "labels": np.array(labels[:max(int(nc[C * 3]), 0)], dtype=np.int32),
            "agg_src_ids": src, "agg_dst_ids": dst,
            "agg_src_off": np.array([pos[v] for v in src.tolist()], dtype=np.int32),
            "agg_dst_off": np.array([pos[v] for v in dst.tolist()], dtype=np.int32)}
