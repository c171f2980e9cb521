"""A graph whose live rows sit at a chosen edge offset: the layout of the far-row tests (tests/test_far_rows_cpu.py,
tests/test_gpu_*far_rows.py), host-only numpy but for device_world, which puts it on a device.  A helper of the tests, not a test file.

  * ballast: vertices 0 .. B - 1 own B rows of L entries each, the last one shortened, `offset` = boundary - k entries in all.  Nothing
    ever reads them: no seed is a ballast vertex and no live column entry names one.  Their column entries are 0 (non-decreasing: the
    rows stay sorted), their weights 1.0f;
  * live: vertices B .. B + n - 1, node2vec_ref.sym_graph at a thousand vertices (sorted symmetric rows, hubs, loops, parallel edges,
    dead -1 entries, empty rows, an all-zero-weight row, weights in eighths), its vertices renumbered round a circle so that the
    513-entry hub starts a quarter of the way into the live edges.  k is the middle of that hub's row: it is the one live row that
    straddles `boundary`, and about a quarter of the live edges lie below it;
  * the reference view: the same graph with the ballast rows replaced by zero-degree stand-ins -- indptr_ref[v] = 0 for v <= B, then the
    live prefix sums; col_ref and w_ref are the live tail only.  Vertex ids are unchanged; a true edge id is a reference edge id plus
    `offset`; the true table's tail is weighted_ref.cdf(indptr_ref, w_ref).  The existing reference modules run on the view as they are:
    they read only the rows that are read.  tests/test_far_rows_cpu.py proves the view against the whole graph where the host can
    hold it (boundary 5000).

Every `want_*` below computes one operation's reference ON THE VIEW, turns its edge ids into true ones, and asserts what makes the case
worth running at this boundary (edge ids on both sides of it, the straddling row left to both sides, ...).  An input that fails a
condition is replaced, never the condition."""
import contextlib
import functools
import time

import numpy as np

from tests import distinct_ref, edge_ids_ref, in_edges_ref, node2vec_ref, pinsage_ref, walk_ref, weighted_ref

LIVE_NODES = 1000
LIVE_HUBS = {0: 63, 1: 64, 2: 65, 3: 255, 4: 256, 5: 257, 6: 513}    # as node2vec_ref.HUBS, the longest row shorter
LIVE_EMPTY = (7, 40, 41, 234, 500, 998)
STRADDLER = 6                                                      # sym_graph's name of the row that straddles the boundary
BOUNDARIES = {"5000": (5000, 64), "2^31": (2 ** 31, 2 ** 20), "2^32": (2 ** 32, 2 ** 20)}      # name -> (boundary, L)
# how a failure at a boundary reads: the end of every assertion message of the GPU tests (world["why"])
WHY = {"5000": "fails at boundary 5000: the harness, or the kernel at any size",
       "2^31": "if only from boundary 2^31 on: a signed 32-bit truncation of an edge offset",
       "2^32": "if at boundary 2^32 only: an unsigned 32-bit truncation of an edge offset"}


def rotate(indptr, col, w, shift):
    """The graph with vertex v renamed (v + shift) mod n: rows moved, column entries renamed (dead ones stay -1), every row sorted again
    (stable: parallel edges keep their order, and their weights)."""
    n = indptr.size - 1
    rows = (np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr)) + shift) % n
    cols = np.where(col >= 0, (col.astype(np.int64) + shift) % n, -1)
    order = np.lexsort((cols, rows))
    deg = np.bincount(rows, minlength=n).astype(np.int64)
    return np.concatenate([[0], np.cumsum(deg)]).astype(np.int64), cols[order].astype(np.int32), w[order]


@functools.lru_cache(maxsize=None)
def live_graph():
    """(indptr, col, w, shift) over LIVE_NODES vertices numbered from 0; sym_graph's vertex v is (v + shift) mod LIVE_NODES here.  shift is
    the smallest at which the middle of the straddler's row has a quarter of the edges below it."""
    indptr, col, w = node2vec_ref.sym_graph(LIVE_NODES, LIVE_HUBS, LIVE_EMPTY, chords=500)
    deg = np.diff(indptr)
    E = int(indptr[-1])
    before = int(indptr[STRADDLER]) + LIVE_HUBS[STRADDLER] // 2     # edges below the middle of the row at shift 0
    tail = np.concatenate([[0], np.cumsum(deg[::-1])])             # tail[s]: the entries of the last s rows, which a shift of s puts first
    shift = int(np.nonzero(before + tail >= E // 4)[0][0])
    out = rotate(indptr, col, w, shift)
    assert node2vec_ref.rows_sorted(out[0], out[1])
    for a in out:
        a.setflags(write=False)
    return out + (shift,)


class FarRows:
    """The layout at one boundary.  Host arrays only of the sizes the host can hold at any boundary: row pointers and the live tail."""

    def __init__(self, boundary, L):
        indptr, col, w, shift = live_graph()
        self.boundary, self.L, self.n = int(boundary), int(L), LIVE_NODES
        hub = (STRADDLER + shift) % self.n
        self.k = int(indptr[hub]) + LIVE_HUBS[STRADDLER] // 2      # live entries below the boundary
        self.offset = self.boundary - self.k                       # ballast entries: a true edge id is a reference edge id + offset
        assert self.offset > 0, "the boundary lies inside the live graph"
        self.B = -(-self.offset // self.L)                         # ballast rows, the last one of offset - (B - 1) L entries
        self.hub = self.B + hub
        self.node_num = self.B + self.n
        self.E = self.offset + int(indptr[-1])
        self.live_E = int(indptr[-1])
        self.indptr_ref = np.concatenate([np.zeros(self.B, np.int64), indptr])
        self.col_ref = np.where(col >= 0, col + self.B, -1).astype(np.int32)
        self.w_ref = w.copy()
        ballast = np.minimum(np.arange(self.B, dtype=np.int64) * self.L, self.offset)
        self.indptr = np.concatenate([ballast, indptr + self.offset])      # the true row pointers: B + n + 1 entries at any boundary
        self.deg = np.diff(self.indptr)
        self.table_ref = weighted_ref.cdf(self.indptr_ref, self.w_ref)
        # the layout's own promises
        assert self.indptr[self.B] == self.offset and self.indptr[-1] == self.E and np.all(self.deg[:self.B - 1] == self.L)
        assert 0 < self.deg[self.B - 1] <= self.L
        straddle = np.nonzero((self.indptr[:-1] < self.boundary) & (self.indptr[1:] > self.boundary))[0]
        assert straddle.tolist() == [self.hub] and self.deg[self.hub] >= 64, "exactly one live row, a hub, straddles the boundary"
        assert 0.2 < self.k / self.live_E < 0.3, "about a quarter of the live edges lie below the boundary"
        assert self.col_ref[self.col_ref >= 0].min() >= self.B, "no live column entry names a ballast vertex"
        for a in (self.indptr_ref, self.col_ref, self.w_ref, self.indptr, self.table_ref):
            a.setflags(write=False)

    # ---- the whole graph, where the host can hold it -------------------------------------------------------------------------------
    def full(self):
        """(indptr, col, w) with the ballast materialised."""
        assert self.E < 1 << 24, "the whole graph is for the small boundary only"
        col = np.concatenate([np.zeros(self.offset, np.int32), self.col_ref])
        w = np.concatenate([np.ones(self.offset, np.float32), self.w_ref])
        return self.indptr, col, w

    # ---- inputs --------------------------------------------------------------------------------------------------------------------
    def vertex(self, v):
        """The id here of sym_graph's vertex v."""
        return self.B + (v + live_graph()[3]) % self.n

    def seeds(self, count):
        """count walk seeds over the live vertices: sym_graph's hubs and special rows first, the straddler every fifth, a repeat, a -1 and
        a node_num (count >= 4).  None is a ballast vertex."""
        s = self.B + (np.arange(count, dtype=np.int64) * 2654435761 % self.n)
        s[:min(count, 12)] = [self.vertex(v) for v in range(12)][:min(count, 12)]
        s[12:count:5] = self.hub
        if count >= 4:
            s[count // 2] = s[0]
            s[count - 1] = -1
            s[count - 2] = self.node_num
        s = s.astype(np.int32)
        assert np.all((s < 0) | (s >= self.B))
        return s

    def train_ids(self):
        """(ids, labels) of the neighbour sampler's seed set: every live vertex once, the straddler and sym_graph's special rows in the
        first batch."""
        first = np.array([self.vertex(v) for v in range(12)], dtype=np.int64)
        rest = self.B + np.random.RandomState(11).permutation(self.n)
        ids = np.concatenate([first, rest[~np.isin(rest, first)]]).astype(np.int32)
        return ids, (ids.astype(np.int64) * 2654435761 % 47).astype(np.int32)

    def arrays(self, whole=False):
        """(indptr, col, table, what to add to an edge id to make it a true one) of the view, or of the whole graph."""
        if not whole:
            return self.indptr_ref, self.col_ref, self.table_ref, self.offset
        indptr, col, w = self.full()
        return indptr, col, weighted_ref.cdf(indptr, w), 0

    @staticmethod
    def true_eids(e, add):
        e = np.asarray(e, dtype=np.int64)
        return np.where(e >= 0, e + add, -1)

    # ---- the conditions ------------------------------------------------------------------------------------------------------------
    def assert_no_ballast_read(self, reads, view=False):
        """From a reference's reads= on the whole graph (or, view=True, on the view, whose column positions start at 0): no index lies in
        a ballast row (of indptr: none below B, so that the pair {indptr[v], indptr[v + 1]} is a live row's), and none outside the arrays."""
        off = 0 if view else self.offset
        base = {"indptr": self.B, "col": off, "edge_cdf": off}
        size = {"indptr": self.node_num + 1, "col": off + self.live_E, "edge_cdf": off + self.live_E}
        for name, chunks in reads.items():
            for i in chunks:
                assert i.size == 0 or (int(i.min()) >= base[name] and int(i.max()) < size[name]), (name, int(i.min()), int(i.max()))

    def assert_straddles(self, left, eids, what):
        """left [..]: the vertex each traversal leaves; eids [..]: its TRUE edge id, -1 where none.  Edge ids occur on both sides of the
        boundary, and the straddling row is stepped from to both sides."""
        left, eids = np.asarray(left).reshape(-1), np.asarray(eids).reshape(-1)
        took = eids >= 0
        low, high = took & (eids < self.boundary), took & (eids >= self.boundary)
        assert low.sum() >= 10 and high.sum() >= 10, f"{what}: edge ids on one side of the boundary only ({low.sum()} / {high.sum()})"
        hub = left == self.hub
        assert (low & hub).sum() >= 3 and (high & hub).sum() >= 3, \
            f"{what}: the straddling row is not left to both sides ({(low & hub).sum()} / {(high & hub).sum()})"
        assert np.all(self.indptr[left[took]] <= eids[took]) and np.all(eids[took] < self.indptr[left[took] + 1])

    # ---- the references, on the view (whole=True: on the whole graph, which must give the same) -------------------------------------
    def want_walk(self, count, length, weighted, restart, base=0, reads=None, whole=False):
        """(traces, true eids) of random_walk."""
        indptr, col, table, add = self.arrays(whole)
        traces, eids = walk_ref.walk(indptr, col, self.seeds(count), length, table=table if weighted else None, restart_prob=restart,
                                     base=base, reads=reads)
        eids = self.true_eids(eids, add)
        self.assert_straddles(traces[:, :-1], eids, f"walk {count} x {length} weighted {weighted} restart {restart}")
        return traces, eids

    def want_node2vec(self, count, length, p, q, weighted, max_tries, base=0, reads=None, whole=False):
        """(traces, true eids) of node2vec_random_walk; at least one membership search runs on a row that starts beyond the boundary."""
        indptr, col, table, add = self.arrays(whole)
        stats = node2vec_ref.new_stats()
        traces, eids = node2vec_ref.walk(indptr, col, self.seeds(count), length, p, q, table=table if weighted else None,
                                         max_tries=max_tries, base=base, reads=reads, stats=stats)
        eids = self.true_eids(eids, add)
        what = f"node2vec {count} x {length} p {p} q {q} weighted {weighted} tries {max_tries}"
        self.assert_straddles(traces[:, :-1], eids, what)
        rows = np.array(sorted(stats["searched_rows"]), dtype=np.int64)
        far = rows[self.indptr[rows] > self.boundary] if rows.size else rows
        assert stats["searches"] >= 10 and far.size >= 1, f"{what}: no row search beyond the boundary ({stats['searches']} searches)"
        return traces, eids

    def want_pinsage(self, count, R, T, k, weighted, termination, base=0, reads=None, whole=False):
        """(neighbours, counts) of pinsage_neighbors; at least one seed's walks cross the boundary."""
        indptr, col, table, add = self.arrays(whole)
        seeds, steps = self.seeds(count), []
        vis = pinsage_ref.visits(indptr, col, seeds, R, T, table=table if weighted else None, termination_prob=termination, base=base,
                                 reads=reads, eids=steps)
        eids = self.true_eids(np.stack(steps, axis=1), add).reshape(count, R * T)     # [seed, r * T + j - 1]
        left = np.concatenate([np.repeat(seeds.astype(np.int64), R)[:, None], vis.reshape(count * R, T)[:, :-1]], axis=1).reshape(count, R * T)
        what = f"pinsage {count} seeds {R} x {T} weighted {weighted} termination {termination}"
        self.assert_straddles(left, eids, what)
        crossing = ((eids >= 0) & (eids < self.boundary)).any(axis=1) & (eids >= self.boundary).any(axis=1)
        assert crossing.sum() >= 1, f"{what}: no seed's walks cross the boundary"
        return pinsage_ref.topk(vis, k)

    def want_batch(self, mode, it, batch, fanout, whole=False):
        """One batch of the neighbour sampler (mode: "replace", "distinct" or "weighted") with true agg_edge_ids: the straddling row is
        sampled for, to both sides, and no ballast row is."""
        indptr, col, table, add = self.arrays(whole)
        ids, labels = self.train_ids()
        if mode == "weighted":
            out = weighted_ref.run_batch(indptr, col, table, ids, labels, batch, it, fanout)
        else:
            out = edge_ids_ref.run_batch(indptr, col, ids, labels, batch, it, fanout, replace=mode == "replace")
            if mode == "distinct":
                plain = distinct_ref.run_batch(indptr, col, ids, labels, batch, it, fanout)
                assert all(np.array_equal(plain[key], out[key]) for key in plain if key != "hop_num")
        out["agg_edge_ids"] = self.true_eids(out["agg_edge_ids"], add)
        self.assert_straddles(out["agg_dst_ids"].astype(np.int64), out["agg_edge_ids"], f"{mode} batch {it} {fanout}")
        assert out["sampled_ids"].min() >= self.B
        return out

    def want_picks(self, per=256, whole=False):
        """(idx, true row_start, deg, want) of legion_draw_weighted_batch: `per` slots in every live row that starts beyond the boundary and
        in the straddling row."""
        rows = np.nonzero((self.indptr[1:] > self.boundary) & (np.arange(self.node_num) >= self.B))[0]
        assert rows[0] == self.hub and np.all(self.indptr[rows[1:]] >= self.boundary)
        idx = (np.arange(rows.size * per, dtype=np.int64) * 7 + 3).astype(np.int32)
        row_start, deg = np.repeat(self.indptr[rows], per), np.repeat(self.deg[rows], per).astype(np.int32)
        table, add = self.arrays(whole)[2:]
        want = weighted_ref.pick_slots(idx, row_start - add, deg, table)
        at = (row_start + want)[want >= 0]
        assert (at < self.boundary).sum() >= 10 and (at >= self.boundary).sum() >= 10 and (want < 0).any()
        return idx, row_start, deg, want


@functools.lru_cache(maxsize=None)
def layout(name):
    return FarRows(*BOUNDARIES[name])


def expand_rows(g, ballast_row, m=None):
    """(rows, offsets, i, r, eid, is_live, src) of the row expansion in_edges and labor_edges share: the live seeds of the layout with the
    straddler every fifth, one whole ballast row in the middle and every live row once behind it.  Over the first m slots (None: every
    slot): i the seed a slot belongs to, r its row, eid its TRUE edge id, src its entry -- the reference view's in a live row, 0 in the
    ballast row."""
    live = np.arange(g.B, g.node_num, dtype=np.int32)
    rows = np.concatenate([g.seeds(300), [ballast_row], live, [g.hub, -1, g.node_num]]).astype(np.int32)
    offsets = in_edges_ref.row_offsets(g.indptr, rows)
    p = np.arange(int(offsets[-1]) if m is None else m, dtype=np.int64)
    i = np.searchsorted(offsets, p, side="right") - 1
    r = rows[i].astype(np.int64)
    eid = g.indptr[r] + (p - offsets[i])
    is_live = r >= g.B
    src = np.zeros(p.size, dtype=np.int32)
    src[is_live] = g.col_ref[eid[is_live] - g.offset]
    return rows, offsets, i, r, eid, is_live, src


@contextlib.contextmanager
def device_world(lib, boundary, weights=False):
    """The whole graph of layout(boundary) on the device, the only place one is put there: col zeros of E entries (weights: and w ones)
    with the live tail written from the host, the row pointers, and the graph (weights: with its table).  Yields what the GPU tests read:
    g, graph, indptr, col, (w,) L = lib, why, name.  Closed and freed on the way out, in the order that lets the next boundary's 16 GiB
    fit: synchronise, close the graph, clear the dict, drop the tensors, empty the cache."""
    import torch
    from legion_amd import engine
    dev = "cuda:0"
    g = layout(boundary)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    col = torch.zeros(g.E, dtype=torch.int32, device=dev)
    col[g.offset:] = torch.from_numpy(g.col_ref.copy()).to(dev)
    w = None
    if weights:
        w = torch.ones(g.E, dtype=torch.float32, device=dev)
        w[g.offset:] = torch.from_numpy(g.w_ref.copy()).to(dev)
    indptr = torch.from_numpy(g.indptr.copy()).to(dev)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    graph = engine.GraphStorage(1, indptr, col)
    if weights:
        graph.set_edge_weights(w)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    print(f"\nfar rows at {boundary}: E = {g.E}, B = {g.B}; arrays {t1 - t0:.3f} s, graph{' and table build' * weights} {t2 - t1:.3f} s")
    out = dict(g=g, graph=graph, indptr=indptr, col=col, L=lib, why=" -- " + WHY[boundary], name=boundary)
    if weights:
        out["w"] = w
    try:
        yield out
    finally:
        torch.cuda.synchronize()
        graph.close()
        out.clear()
        del graph, col, w, indptr
        torch.cuda.empty_cache()


# ---- the cases both test files run -------------------------------------------------------------------------------------------------
WALK_CASES = [(count, length, weighted, restart) for count in (257, 5000) for length in (17, 100)
              for weighted, restart in ((False, 0.0), (True, 0.0), (False, 0.3), (True, 0.3))]
# (p, q) x weights x max_tries; the walks 257 x 100 and 5000 x 17 in turn: both chunk sizes' last partial chunk, one tile and twenty
NODE2VEC_CASES = [((257, 100) if (a + b + c) % 2 == 0 else (5000, 17)) + (pq[0], pq[1], weighted, tries)
                  for a, pq in enumerate(((0.5, 2.0), (4.0, 0.25))) for b, weighted in enumerate((False, True)) for c, tries in enumerate((256, 3))]
PINSAGE_CASES = [(count, R, T, k, weighted, termination) for count, R, T, k in ((65, 64, 16, 10), (257, 10, 2, 3))
                 for weighted in (False, True) for termination in (0.0, 0.5)]
SAMPLER_MODES = ["replace", "distinct", "weighted"]
SAMPLER_SHAPES = [[25, 10], [4, 3, 2]]
SAMPLER_BATCH = 64
