"""Weighted neighbour sampling (MemoryPool weighted = 1, with replacement) restated in numpy on the CPU: the per-row prefix-sum table,
the pick rule, and one whole batch laid out as tests/edge_ids_ref.run_batch lays it out (edge order = slot order, first touch = the
lowest slot, counters through the oracle's own lgo_counter_update) with agg_edge_ids, the serve and PreSC variants and PreSC's
hotness arrays.  The contract is in include/legion_hip.h (legion_graph_set_edge_weights).  A helper of the tests, not a test file."""
import numpy as np

from tests.distinct_ref import C, counter_update, minstd_pow


def sanitise(w):
    """w' = w where w is finite and > 0, else 0 (negative values, NaN, +-inf, -0)."""
    w = np.asarray(w, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(w) & (w > 0), w, np.float32(0)).astype(np.float32)


def cdf(indptr, w):
    """float32[E]: per row the inclusive prefix sums of the sanitised weights, summed in float64 and rounded once."""
    indptr = np.asarray(indptr, dtype=np.int64)
    ws = sanitise(w).astype(np.float64)
    out = np.zeros(ws.size, dtype=np.float32)
    for v in range(indptr.size - 1):
        s, e = int(indptr[v]), int(indptr[v + 1])
        if e > s:
            out[s:e] = np.cumsum(ws[s:e]).astype(np.float32)
    return out


def unit_r(idx):
    """The double the uniform draw forms for slot idx: (x - 1) / 2147483646 with x = minstd(idx + 1)."""
    x = minstd_pow(np.asarray(idx, dtype=np.int64).astype(np.uint64) + np.uint64(1))
    return (x - np.uint64(1)).astype(np.float64) / 2147483646.0


def pick_slots(idx, row_start, deg, table):
    """The pick of each slot idx[i] in the row {row_start[i], deg[i]} of the table; -1 for deg <= 0 or a row total of 0."""
    idx = np.asarray(idx, dtype=np.int64)
    row_start = np.asarray(row_start, dtype=np.int64)
    deg = np.asarray(deg, dtype=np.int64)
    t64 = np.asarray(table, dtype=np.float32).astype(np.float64)
    r = unit_r(idx)
    out = np.full(idx.size, -1, dtype=np.int32)
    live = np.nonzero(deg > 0)[0]                      # (rows with entries have distinct starts: one search call per row)
    if live.size == 0:
        return out
    live = live[np.argsort(row_start[live], kind="stable")]
    cuts = np.nonzero(np.diff(row_start[live]))[0] + 1
    for grp in np.split(live, cuts):
        s, D = int(row_start[grp[0]]), int(deg[grp[0]])
        row = t64[s:s + D]
        T = row[-1]
        if T == 0:
            continue
        out[grp] = np.searchsorted(row, r[grp] * T, side="right")
    return out


def picks(base, row_start, deg, f, table):
    """Adjacency positions [n, f] of n frontier entries (first slot base[i] = q*f, row {row_start[i], deg[i]}); -1 for
    k >= min(f, D) and for every slot of a row whose total is 0."""
    base = np.asarray(base, dtype=np.int64)
    row_start = np.asarray(row_start, dtype=np.int64)
    D = np.maximum(np.asarray(deg, dtype=np.int64), 0)
    n = base.size
    out = np.full((n, f), -1, dtype=np.int32)
    if n == 0:
        return out
    k = np.arange(f, dtype=np.int64)[None, :]
    live = k < D[:, None]
    q, kk = np.nonzero(live)
    out[q, kk] = pick_slots(base[q] + kk, row_start[q], D[q], table)
    return out


def run_batch(indptr, col, table, all_ids, all_labels, batch_size, counter, fanout, serve=True, edge_access=None, node_access=None):
    """One weighted batch with "agg_edge_ids" (int64) next to the usual keys.  serve: the batch's gathers run (ops 3h+1 update the
    counters too; PreSC runs without them).  edge_access / node_access: PreSC's hotness counts, added to in place (train mode)."""
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
    src_ids, dst_ids, eids = [], [], []
    for h, f in enumerate(fanout):
        op = C * (h + 1)
        frontier = np.array(ids[:max(int(nc[1]), 0)] if h == 0 else src_ids[ec[0]:ec[0] + ec[1]], dtype=np.int64)
        n_new = n_edge = 0
        if frontier.size:
            real = frontier >= 0
            fr = np.where(real, frontier, 0)
            D = np.where(real, indptr[fr + 1] - indptr[fr], 0)
            P = picks(np.arange(frontier.size, dtype=np.int64) * f, indptr[fr], D, f, table)
            q, k = np.nonzero(P >= 0)                              # slot order: q-major, k-minor
            at = indptr[fr[q]] + P[q, k]                           # int64 positions in the full column array
            nb = col[at]
            for s, d, e in zip(frontier[q].tolist(), nb.tolist(), at.tolist()):
                if d < 0:                                          # a dead column entry: no edge, no id, no hotness
                    continue
                if edge_access is not None:
                    edge_access[s] += 1
                if d not in pos:
                    pos[d] = len(ids); ids.append(d); n_new += 1
                src_ids.append(d); dst_ids.append(s); eids.append(e); n_edge += 1
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
            "agg_dst_off": np.array([pos[v] for v in dst.tolist()], dtype=np.int32),
            "agg_edge_ids": np.array(eids[:n_edges], dtype=np.int64)}


def check_edges(indptr, col, w, batch):
    """What holds for every edge whatever was drawn: the id lies in the row of the vertex sampled for, names the neighbour, and its
    weight is positive."""
    e = batch["agg_edge_ids"]
    assert e.dtype == np.int64 and e.shape == batch["agg_src_ids"].shape
    dst = batch["agg_dst_ids"].astype(np.int64)
    assert np.all((indptr[dst] <= e) & (e < indptr[dst + 1]))
    assert np.array_equal(np.asarray(col)[e], batch["agg_src_ids"])
    assert np.all(sanitise(w)[e] > 0)


def hash_weights(n, seed=1, eighths=True):
    """Deterministic per-edge weights: multiples of 1/8 in [0, 4] with about a fifth of them zero (exact prefix sums), or, with
    eighths=False, positive floats in (0, 1]."""
    i = np.arange(n, dtype=np.uint64)
    h = (i * np.uint64(2654435761) + np.uint64(seed) * np.uint64(40503)) % np.uint64(2147483647)
    h = (h * np.uint64(48271)) % np.uint64(2147483647)
    if eighths:
        v = (h % np.uint64(41)).astype(np.float32)
        return np.where(v > 32, np.float32(0), v / np.float32(8)).astype(np.float32)
    return ((h % np.uint64(1 << 20)).astype(np.float32) + np.float32(1)) / np.float32(1 << 20)
