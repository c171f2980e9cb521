"""Graphs whose rows have at most one entry, and what walks and PinSAGE's neighbour sampler give on them, written without a draw: with
one entry draw_from_x(x, 1) is 0 and the weighted search over one positive entry is clamped to 0, so a walk is the iterated successor
in both pick modes whatever is drawn.  The content of a seed's visit segment is then chosen, not drawn: a path over a chosen id order
fills it in that order.  A helper of the tests, not a test file."""
import numpy as np

SLOTS = 2048                                                       # visit slots of a PinSAGE tile
ORDERS = ["ascending", "descending", "bit-reversed", "organ-pipe", "shuffled"]
PATH_T = [31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024]       # R = 1: both sides of every class edge, and a full segment
RUN_SHAPES = [(4, 8), (2, 32), (4, 64), (4, 256), (32, 32), (1024, 1)]      # (R, T): every vertex of a row counts R


def vpad(visits):
    """The class of R * T visits per seed: the slots of a seed's segment."""
    return next(c for c in (32, 64, 256, 1024) if visits <= c)


def id_order(name, n):
    """A permutation of 0 .. n - 1: the vertex ids along a path, from its first position to its last."""
    a = np.arange(n, dtype=np.int64)
    if name == "ascending":
        return a
    if name == "descending":
        return a[::-1].copy()
    if name == "bit-reversed":
        bits = max(int(n - 1).bit_length(), 1)
        rev = np.array([int(format(i, f"0{bits}b")[::-1], 2) for i in range(1 << bits)], dtype=np.int64)
        return rev[rev < n]
    if name == "organ-pipe":
        return np.concatenate([a[0::2], a[1::2][::-1]])
    if name == "shuffled":
        return np.random.RandomState(77).permutation(n).astype(np.int64)
    raise ValueError(name)


def path_succ(order):
    """succ[v]: the vertex after v on the path that visits `order` from front to back; -1 for the last."""
    succ = np.full(order.size, -1, dtype=np.int64)
    succ[order[:-1]] = order[1:]
    return succ


def graph_of(succ, zero_weight=()):
    """(indptr int64, col int32, weights float32) of the graph with the one edge v -> succ[v] where succ[v] >= 0.  Weights are
    arbitrary positive floats (the pick does not depend on them); the edges leaving the vertices of zero_weight weigh 0."""
    succ = np.asarray(succ, dtype=np.int64)
    has = succ >= 0
    indptr = np.concatenate([[0], np.cumsum(has)]).astype(np.int64)
    col = succ[has].astype(np.int32)
    w = (0.37 + (np.arange(col.size) % 11) * 1.3).astype(np.float32)
    for v in zero_weight:
        assert has[v]
        w[indptr[v]] = 0
    return indptr, col, w


def without(succ, vertices):
    """succ with the edges leaving `vertices` taken out: what a weighted walk sees where those edges weigh 0."""
    succ = np.array(succ, dtype=np.int64)
    succ[list(vertices)] = -1
    return succ


def iterate(succ, seeds, steps):
    """int64 [n, steps]: column j - 1 is the vertex step j reaches from each seed, -1 once there is no successor (or no such seed)."""
    succ = np.asarray(succ, dtype=np.int64)
    v = np.asarray(seeds, dtype=np.int64).copy()
    out = np.full((v.size, steps), -1, dtype=np.int64)
    for j in range(steps):
        ok = (v >= 0) & (v < succ.size)
        v = np.where(ok, succ[np.where(ok, v, 0)], -1)
        out[:, j] = v
    return out


def expected_walk(succ, indptr, seeds, length):
    """(traces int32 [n, length + 1], eids int64 [n, length]): the iterated successor; a row's one entry is edge indptr[v]."""
    seeds = np.asarray(seeds, dtype=np.int32)
    steps = iterate(succ, seeds, length)
    traces = np.concatenate([seeds[:, None].astype(np.int64), steps], axis=1)
    src = traces[:, :-1]
    eids = np.where(steps >= 0, np.asarray(indptr, dtype=np.int64)[np.where(steps >= 0, src, 0)], -1)
    return traces.astype(np.int32), eids.astype(np.int64)


def expected_neighbors(succ, seeds, R, T, k):
    """(neighbors, counts) int32 [n, k]: the R walks of a seed are the same walk, so the counts are R times those of one iteration of
    T steps; rows by (count descending, id ascending), -1 / 0 past the distinct vertices."""
    steps = iterate(succ, seeds, T)
    nb = np.full((steps.shape[0], k), -1, dtype=np.int32)
    ct = np.zeros((steps.shape[0], k), dtype=np.int32)
    for i, row in enumerate(steps):
        ids, c = np.unique(row[row >= 0], return_counts=True)
        order = sorted(range(ids.size), key=lambda a: (-int(c[a]), int(ids[a])))[:k]
        nb[i, :len(order)], ct[i, :len(order)] = ids[order], c[order] * R
    return nb, ct


def ks_for(T):
    return sorted({1, max(T - 1, 1), T, min(T + 1, 1024), 1024})


def path_case(order, R, T):
    """(succ, seeds) of a path case: 3 S + 1 seeds at consecutive path positions from the front and one -1, on a path long enough
    that the first seeds see R * T visits with no sentinel and the last ones run into the path's end (short rows: L < T visits),
    the very last being the end itself where the tile count allows; 3 S + 2 seeds end in a partial tile."""
    S = SLOTS // vpad(R * T)
    n = max(T + 1 + 2 * S, 3 * S + 1)
    ids = id_order(order, n)
    seeds = np.concatenate([ids[:3 * S + 1], [-1]]).astype(np.int32)
    return path_succ(ids), seeds


# ---- one small graph of the shapes a path does not have ----------------------------------------------------------------------------
MISC_NODES = 25
MISC_ZERO = (22,)                                                  # the edge 22 -> 23 weighs 0


def misc_succ():
    """0: a self-loop.  1 -> 9 -> 5 -> 1: a cycle of three whose first visit from 1 is its largest id.  10 -> 11 -> 12 -> 13 -> 14 -> 12:
    a tail into a cycle.  20 -> 21 -> 22 -> 23 -> 24: a path whose third edge weighs 0.  The rest have no successor."""
    succ = np.full(MISC_NODES, -1, dtype=np.int64)
    for a, b in ((0, 0), (1, 9), (9, 5), (5, 1), (10, 11), (11, 12), (12, 13), (13, 14), (14, 12), (20, 21), (21, 22), (22, 23), (23, 24)):
        succ[a] = b
    return succ


# (the pair of 0s at 20, 21 shares a tile in every class: two neighbouring segments full of one id)
MISC_SEEDS = np.array([0, 1, 9, 5, 10, 11, 12, 13, 14, 20, 21, 22, 23, 24, 2, -1, MISC_NODES, 0, 1, 20, 0, 0, 1], dtype=np.int32)
MISC_SHAPES = [(1, 1, 1), (1, 32, 1), (1, 32, 2), (2, 32, 3), (1, 64, 64), (4, 64, 5), (256, 1, 2), (1, 256, 4), (1024, 1, 1), (1, 1024, 3),
               (32, 32, 1024), (3, 5, 4), (1, 1024, 1024)]
