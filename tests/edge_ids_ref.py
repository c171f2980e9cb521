"""The edge-id mode (MemoryPool edge_ids = 1) restated in numpy on the CPU: one whole batch in either sampling mode, laid out as
tests/distinct_ref.run_batch lays it out (edge order = slot order, first touch = the lowest slot, counters through the oracle's
own lgo_counter_update), plus agg_edge_ids: per edge, indptr[frontier vertex] + the adjacency position its slot drew -- with
replacement draw(q*f + k, D) for k < min(f, D) (oracle/legion_oracle.c lgo_random_sample), without it distinct_ref.picks.
A helper of the tests, not a test file."""
import numpy as np

from tests.distinct_ref import C, counter_update, draw, picks


def slot_picks(n_entries, deg, f, replace):
    """Adjacency positions [n, f] the slots q*f + k of n frontier entries draw; -1 for k >= min(f, D)."""
    base = np.arange(n_entries, dtype=np.int64) * f
    D = np.maximum(np.asarray(deg, dtype=np.int64), 0)
    if not replace:
        return picks(base, D, f)
    k = np.arange(f, dtype=np.int64)[None, :]
    live = k < D[:, None]
    p = draw(base[:, None] + k, np.where(live, D[:, None], 1))
    return np.where(live, p, -1).astype(np.int32)


def run_batch(indptr, col, all_ids, all_labels, batch_size, counter, fanout, replace=True):
    """One serve-mode batch (the gathers' counter updates included) with "agg_edge_ids" (int64) next to the usual keys."""
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
            P = slot_picks(frontier.size, D, f, replace)
            q, k = np.nonzero(P >= 0)                              # slot order: q-major, k-minor
            at = indptr[fr[q]] + P[q, k]                           # int64 positions in the full column array
            nb = col[at]
            for s, d, e in zip(frontier[q].tolist(), nb.tolist(), at.tolist()):
                if d < 0:                                          # a dead column entry: no edge, no id
                    continue
                if d not in pos:
                    pos[d] = len(ids); ids.append(d); n_new += 1
                src_ids.append(d); dst_ids.append(s); eids.append(e); n_edge += 1
        nc[C * 2] += n_new
        ec[2] += n_edge
        counter_update(nc, ec, op)
        counter_update(nc, ec, op + 1)
    n_nodes = max(int(nc[C * 3 + hop_num]), 0)
    n_edges = max(int(ec[C * 3 + hop_num]), 0)
    src = np.array(src_ids[:n_edges], dtype=np.int32)
    dst = np.array(dst_ids[:n_edges], dtype=np.int32)
    return {"node_counter": nc, "edge_counter": ec, "hop_num": hop_num,
            "sampled_ids": np.array(ids[:n_nodes], dtype=np.int32),
            "labels": np.array(labels[:max(int(nc[C * 3]), 0)], dtype=np.int32),
            "agg_src_ids": src, "agg_dst_ids": dst,
            "agg_src_off": np.array([pos[v] for v in src.tolist()], dtype=np.int32),
            "agg_dst_off": np.array([pos[v] for v in dst.tolist()], dtype=np.int32),
            "agg_edge_ids": np.array(eids[:n_edges], dtype=np.int64)}


def check_edge_ids(indptr, col, batch):
    """What holds for every edge whatever was drawn: the id lies in the row of the vertex sampled for and names the neighbour."""
    e = batch["agg_edge_ids"]
    assert e.dtype == np.int64 and e.shape == batch["agg_src_ids"].shape
    dst = batch["agg_dst_ids"].astype(np.int64)
    assert np.all((indptr[dst] <= e) & (e < indptr[dst + 1]))
    assert np.array_equal(np.asarray(col)[e], batch["agg_src_ids"])
