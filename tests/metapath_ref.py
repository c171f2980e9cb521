"""Metapath walks and PinSAGE over a metapath (GraphStorage.metapath_random_walk, pinsage_metapath_neighbors; legion_metapath_walk,
legion_pinsage_metapath_neighbors) restated in numpy on the CPU, as the contract in include/legion_hip.h writes them: tests/walk_ref's
draws, a row's type segment by np.searchsorted over (row, type) keys -- one transition for all walks at once -- and PinSAGE's visits fed
to tests/pinsage_ref.topk.  And the hand-made typed graph of the tests.  A helper of the tests, not a test file."""
import functools

import numpy as np

from tests import pinsage_ref, walk_ref


def row_keys(indptr, etype):
    """row * 256 + type of every entry: ascending over the whole of col when every row is sorted by type."""
    rows = np.repeat(np.arange(indptr.size - 1, dtype=np.int64), np.diff(indptr))
    keys = rows * 256 + etype
    assert np.all(np.diff(keys) >= 0), "the rows are sorted by type"
    return keys


def step(indptr, col, keys, v, t, x, y=None, restart_prob=0.0):
    """One transition of every walk at once with type t: (next vertex, edge id), both -1 where the walk has ended or ends."""
    nxt = np.full(v.size, -1, dtype=np.int64)
    eid = np.full(v.size, -1, dtype=np.int64)
    live = (v >= 0) & (v < indptr.size - 1)                      # 1. before any load
    if y is not None and restart_prob > 0:                       # 2.
        live &= ~(walk_ref.unit_of(y) < np.float64(np.float32(restart_prob)))
    at = np.nonzero(live)[0]
    lo = np.searchsorted(keys, v[at] * 256 + t, side="left")     # 3. / 4.: absolute positions; an empty row has lo == hi
    hi = np.searchsorted(keys, v[at] * 256 + t, side="right")
    at, lo, R = at[hi > lo], lo[hi > lo], (hi - lo)[hi > lo]
    pick = lo + (walk_ref.unit_of(x[at]) * R.astype(np.float64)).astype(np.int64)
    u = col[pick].astype(np.int64)                               # 5.
    nxt[at[u >= 0]], eid[at[u >= 0]] = u[u >= 0], pick[u >= 0]
    return nxt, eid


def walk(indptr, col, keys, seeds, metapath, length, restart_prob=0.0, base=0):
    """(traces int32 [n, length + 1], eids int64 [n, length]): step j uses metapath[(j - 1) % L]."""
    seeds = np.asarray(seeds, dtype=np.int32)
    n = seeds.size
    traces = np.full((n, length + 1), -1, dtype=np.int32)
    eids = np.full((n, length), -1, dtype=np.int64)
    traces[:, 0] = seeds
    x = walk_ref.draws(base, n * length).reshape(n, length)
    y = walk_ref.draws(base, n * length, 2 ** 31).reshape(n, length) if restart_prob > 0 else None
    v = seeds.astype(np.int64)
    for j in range(1, length + 1):
        v, e = step(indptr, col, keys, v, metapath[(j - 1) % len(metapath)], x[:, j - 1], None if y is None else y[:, j - 1], restart_prob)
        traces[:, j], eids[:, j - 1] = v, e
    return traces, eids


def visits(indptr, col, keys, seeds, metapath, R, Q, termination_prob=0.5, base=0):
    """int32 [n, R * Q]: entry [i, r * Q + q] is where walk r of seed i stands at the end of traversal q + 1, or -1."""
    seeds = np.asarray(seeds, dtype=np.int32)
    L, W = len(metapath), seeds.size * R
    x = walk_ref.draws(base, W * Q * L).reshape(W, Q * L)
    y = walk_ref.draws(base, W * Q * L, 2 ** 31).reshape(W, Q * L) if termination_prob > 0 else None
    v = np.repeat(seeds.astype(np.int64), R)
    out = np.full((W, Q), -1, dtype=np.int32)
    for j in range(1, Q * L + 1):
        draw = y is not None and j > 1 and (j - 1) % L == 0      # before the first step of traversals 2 .. Q
        v, _ = step(indptr, col, keys, v, metapath[(j - 1) % L], x[:, j - 1], y[:, j - 1] if draw else None, termination_prob)
        if j % L == 0:
            out[:, j // L - 1] = v
    return out.reshape(seeds.size, R * Q)


def neighbors(indptr, col, keys, seeds, metapath, R, Q, k, termination_prob=0.5, base=0):
    return pinsage_ref.topk(visits(indptr, col, keys, seeds, metapath, R, Q, termination_prob, base), k)


# ---- the hand-made typed graph ------------------------------------------------------------------------------------------------------
SHORT = 16                                                         # LG_METAPATH_SHORT: rows up to here are counted, longer ones searched
DEGREES = [0, 1, 2, 15, 16, 17, 63, 64, 65, 4097, 70001]           # vertices 0 .. 10; SHORT - 1, SHORT, SHORT + 1 among them
HUB, NODE_NUM = 10, 3000
A, B, C = 0, 32, 63                                                # the types the metapaths use, at T = 64
# the special rows at T = 64 as runs (type, entries); the rest of a row is filled with type 40
RUNS = {1: [(C, 1)], 2: [(A, 1), (C, 1)], 3: [(A, 7), (B, 1), (C, 7)], 4: [(A, 5), (B, 5), (C, 6)], 5: [(A, 8), (B, 1), (C, 8)],
        6: [(t, 1) for t in range(63)],                            # one entry of every type but the last
        7: [(A, 32), (B, 32)],                                     # the last type absent; a boundary on the search's first probe, 64 >> 1
        8: [(A, 30), (C, 35)],                                     # a middle type absent
        9: [(A, 1), (7, 2047), (B, 1000), (C, 1)],                 # one-entry segments at either end; a boundary at 4097 >> 1 = 2048
        HUB: [(5, 10000), (B, 25000), (C, 30000)]}                 # the first type absent


@functools.lru_cache(maxsize=None)
def hand_graph():
    """(indptr, col, etype at T = 64): the rows of DEGREES, then rows of 8 .. 20 entries whose types are 0, 32 and 63 nine times in ten
    -- most carry all three, some lack one -- one entry in fifty pointing at the special rows, and dead entries."""
    rng = np.random.RandomState(28)
    deg = rng.randint(8, 21, NODE_NUM).astype(np.int64)
    deg[:len(DEGREES)] = DEGREES
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    E = int(indptr[-1])
    col = rng.randint(0, NODE_NUM, E).astype(np.int32)
    near = rng.rand(E) < 0.02
    col[near] = rng.randint(0, len(DEGREES), int(near.sum()))
    etype = np.where(rng.rand(E) < 0.9, rng.choice([A, B, C], E), rng.randint(0, 64, E)).astype(np.uint8)
    for v, runs in RUNS.items():
        row = np.concatenate([np.full(c, t) for t, c in runs])
        etype[indptr[v]:indptr[v + 1]] = np.concatenate([row, np.full(DEGREES[v] - row.size, 40)])[:DEGREES[v]]
    rows = np.repeat(np.arange(NODE_NUM), deg)
    etype = etype[np.lexsort((etype, rows))]                       # every row sorted by type
    col[rng.rand(E) < 0.004] = -1
    col[indptr[9] + 2050], col[indptr[HUB] + 50000], col[indptr[8] + 40], col[indptr[4] + 12] = -1, -1, -1, -1      # in sampled segments
    for a in (indptr, col, etype):
        a.setflags(write=False)
    return indptr, col, etype


@functools.lru_cache(maxsize=None)
def types(T):
    """The graph's types at T in {1, 2, 64}: a monotone map of the 64, so every row stays sorted; A, B, C become types_of(T)."""
    etype = hand_graph()[2]
    return {1: np.zeros_like(etype), 2: (etype >= B).astype(np.uint8), 64: etype}[T]


def types_of(T):
    return {1: (0, 0, 0), 2: (0, 1, 1), 64: (A, B, C)}[T]


def metapath(T, L):
    """L entries: the first and the last type in turn, the middle one every fourth."""
    a, b, c = types_of(T)
    return [(a, c, a, b)[i % 4] for i in range(L)]


@functools.lru_cache(maxsize=None)
def keys(T):
    return row_keys(hand_graph()[0], types(T))


@functools.lru_cache(maxsize=None)
def seeds():
    """5 000 seeds: the special rows first, a -1 and a node_num behind them, then the whole graph with repeats.  Walk w draws at
    base + w * length whatever the number of walks: the walks of seeds()[:n] are the first n of the whole list's."""
    s = (np.arange(5000, dtype=np.int64) * 2654435761 % NODE_NUM).astype(np.int32)
    s[:len(DEGREES)] = np.arange(len(DEGREES))
    s[11], s[12], s[13:255:9] = -1, NODE_NUM, HUB
    s[254], s[256] = 9, 7                                          # the last walk of a tile and the first of the next
    s.setflags(write=False)
    return s


def assert_hand_graph():
    """What makes a wrong kernel fail on this graph, from the reference alone."""
    indptr, col, etype = hand_graph()
    seg = lambda v, t: (int(np.searchsorted(keys(64), v * 256 + t, "left") - indptr[v]), int(np.searchsorted(keys(64), v * 256 + t, "right") - indptr[v]))
    assert {SHORT - 1, SHORT, SHORT + 1} <= set(DEGREES) and np.diff(indptr)[:len(DEGREES)].tolist() == DEGREES
    assert seg(HUB, A) == (0, 0) and seg(8, B) == (30, 30) and seg(7, C) == (64, 64), "a type absent at the start, in the middle, at the end"
    assert seg(9, A) == (0, 1) and seg(9, C) == (4096, 4097) and seg(6, A) == (0, 1), "one-entry segments at either end"
    assert seg(9, B)[0] == 4097 >> 1 and seg(7, B)[0] == 64 >> 1, "a boundary on the search's first probe"
    assert etype.min() == 0 and etype.max() == 63
    for v, e in ((9, 2050), (HUB, 50000), (8, 40), (4, 12)):
        t = int(etype[indptr[v] + e])
        assert col[indptr[v] + e] == -1 and t in (A, B, C) and seg(v, t)[0] <= e < seg(v, t)[1], "a dead entry inside a sampled segment"
    for T in (1, 2, 64):
        traces, eids = walk(indptr, col, keys(T), seeds(), metapath(T, 2), 100)
        ended = (traces[:, :-1] >= 0) & (traces[:, 1:] < 0)
        assert (traces[:, 100] >= 0).sum() >= 20 and ended[13:].any(axis=0).all(), f"T {T}: walks survive 100 steps, and walks end at every position"
        took = etype[eids[eids >= 0]] if T == 64 else None
        assert T != 64 or set(np.unique(took).tolist()) == {A, C}, "every step stays inside its type"
