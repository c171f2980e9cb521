"""One compaction, three readers: labor_edges with a fan-out of at least the largest degree, induced_edges against a set of every vertex
(src_local mapped back through nodes) and in_edges with its dead entries removed are the same list of entries, and that list is numpy's,
entry for entry.  The graph is small and has dead entries; the row lists hold M = 1, 1 023, 1 024, 1 025 (the tile's edge) and 262 145
slots (the first M with two second-level sums).  Through the C ABI the capacity is K - 1 (the guard), K (the exact fit) and K + 5 (the -1
fill); with a set of half the vertices some tiles keep nothing and are skipped.  What makes a wrong kernel fail is asserted from numpy
before any launch."""
import numpy as np
import pytest
import torch

from tests.compare import same_arrays
from tests.test_gpu_induced import abi as induced_abi
from tests.test_gpu_labor import abi as labor_abi

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = 1200
DEGREES = {0: 1, 1: 1022, 2: 1, 3: 1, 4: 257}                 # every other vertex has no entries
FANOUT = 1022
SALT = 5
TILE = 1024
# M -> rows.  The last: 128 tiles that hold rows 0, 1 and 2 each, then 128 and a bit that hold nothing but rows 1 and 4
ROWS = {1: [0], 1023: [0, 1], 1024: [0, 1, 2], 1025: [0, 1, 2, 3], 262145: [0, 1, 2] * 128 + [1] * 128 + [4]}
NAMES = ("dst", "src", "eid")


def make_graph():
    """(indptr, col): the sources of vertex 1's and 4's rows lie in the upper half of the vertices, all others in the lower; every 37th
    entry of a long row is dead."""
    rng = np.random.RandomState(30)
    deg = np.zeros(N, np.int64)
    for v, d in DEGREES.items():
        deg[v] = d
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = rng.randint(0, N // 2, int(indptr[-1])).astype(np.int32)
    for v in (1, 4):
        row = col[indptr[v]:indptr[v + 1]]
        row += N // 2
        row[5::37] = -1
    return indptr, col


def all_nodes():
    return np.random.RandomState(31).permutation(N).astype(np.int32)


def lower_half():
    return np.random.RandomState(32).permutation(N // 2).astype(np.int32)


def expand(indptr, col, rows):
    """(offsets, dst, src, eid) of every slot of rows, dead entries included."""
    rows = np.asarray(rows, np.int64)
    deg = indptr[rows + 1] - indptr[rows]
    off = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    dst = np.repeat(np.arange(rows.size), deg).astype(np.int32)
    eid = (np.arange(int(off[-1])) - off[dst] + indptr[rows[dst]]).astype(np.int64)
    return off, dst, col[eid], eid


def kept(indptr, col, rows, nodes=None):
    """(offsets, slot mask, dst, src, eid) of the live entries whose source is in nodes (None: of every live entry)."""
    off, dst, src, eid = expand(indptr, col, rows)
    mask = src >= 0 if nodes is None else (src >= 0) & np.isin(src, nodes)
    return off, mask, dst[mask], src[mask], eid[mask]


def positions(nodes, src):
    where = np.full(N, -1, np.int32)
    where[nodes] = np.arange(nodes.size, dtype=np.int32)
    return where[src]


def capped(want, cap):
    return [np.concatenate([w, np.full(max(cap - w.size, 0), -1, w.dtype)])[:cap] for w in want]


@pytest.fixture(scope="module")
def world(hip):
    from legion_amd import engine
    indptr, col = make_graph()
    graph = engine.GraphStorage(1, torch.from_numpy(indptr).to(DEV), torch.from_numpy(col).to(DEV))
    yield dict(graph=graph, indptr=indptr, col=col, L=hip)
    torch.cuda.synchronize()
    graph.close()


def test_the_inputs_hold_their_conditions_before_any_launch():
    indptr, col = make_graph()
    assert (col < 0).sum() == 35 and np.diff(indptr).max() <= FANOUT, "dead entries, and a fan-out that keeps every live entry"
    for M, rows in ROWS.items():
        off, mask, dst, src, eid = kept(indptr, col, rows)
        assert off[-1] == M and 0 < mask.sum() and (M < 1023 or mask.sum() < M), (M, mask.sum())
    assert (262145 + 1023) // 1024 == 257, "two second-level sums of 256 tile counts"
    nodes = all_nodes()
    assert not np.array_equal(nodes, np.arange(N)) and np.array_equal(np.sort(nodes), np.arange(N)), "local != global"
    off, mask, dst, src, eid = kept(indptr, col, ROWS[262145], lower_half())
    tiles = np.add.reduceat(mask, np.arange(0, mask.size, TILE))
    assert tiles.size == 257 and (tiles == 0).sum() >= 100 and (tiles > 0).sum() >= 100, "tiles that keep nothing between tiles that keep"


@pytest.mark.parametrize("M", sorted(ROWS))
def test_three_readers_of_one_compaction(world, M):
    from legion_amd import engine
    g, indptr, col = world["graph"], world["indptr"], world["col"]
    rows = np.array(ROWS[M], np.int32)
    off, mask, dst, src, eid = kept(indptr, col, rows)
    nodes = all_nodes()
    labor = g.labor_edges(rows, FANOUT, salt=SALT, return_eids=True)
    induced = g.induced_edges(rows, engine.NodeSet(torch.from_numpy(nodes).to(DEV)), return_eids=True)
    whole = g.in_edges(rows, return_eids=True)
    torch.cuda.synchronize()
    same_arrays(list(labor), [dst, src, eid], f"labor_edges, M {M}", names=NAMES)
    same_arrays(list(induced), [dst, positions(nodes, src), eid], f"induced_edges, M {M}", names=NAMES)
    same_arrays(nodes[induced[1].cpu().numpy()], src, f"nodes[src_local], M {M}")
    live = (whole[2] >= 0).cpu().numpy()
    same_arrays(whole[0], off, f"offsets, M {M}")
    same_arrays([x.cpu().numpy()[live] for x in whole[1:]], [dst, src, eid], f"in_edges without its dead entries, M {M}", names=NAMES)


@pytest.mark.parametrize("M", [1025, 262145])
def test_the_capacity_through_the_c_abi(world, M):
    g, indptr, col, L = world["graph"], world["indptr"], world["col"], world["L"]
    rows = np.array(ROWS[M], np.int32)
    off, mask, dst, src, eid = kept(indptr, col, rows)
    nodes, K = all_nodes(), int(mask.sum())
    for cap in (K - 1, K, K + 5):
        k, *out = labor_abi(L, g, rows, off, M, FANOUT, SALT, cap)
        assert k == K, "the count does not depend on cap"
        same_arrays(out, capped([dst, src, eid], cap), f"labor, cap {cap - K:+d}", names=NAMES)
        k, *out = induced_abi(L, g, rows, off, M, nodes, cap)
        assert k == K
        same_arrays(out, capped([dst, positions(nodes, src), eid], cap), f"induced, cap {cap - K:+d}", names=NAMES)


@pytest.mark.parametrize("M", [1025, 262145])
def test_half_the_vertices_and_tiles_that_keep_nothing(world, M):
    g, indptr, col, L = world["graph"], world["indptr"], world["col"], world["L"]
    rows, nodes = np.array(ROWS[M], np.int32), lower_half()
    off, mask, dst, src, eid = kept(indptr, col, rows, nodes)
    want = [dst, positions(nodes, src), eid]
    K = int(mask.sum())
    assert 0 < K < int((expand(indptr, col, rows)[2] >= 0).sum())
    got = g.induced_edges(rows, nodes, return_eids=True)
    torch.cuda.synchronize()
    same_arrays(list(got), want, f"half the vertices, M {M}", names=NAMES)
    for cap in (K - 1, K, K + 5):
        k, *out = induced_abi(L, g, rows, off, M, nodes, cap)
        assert k == K
        same_arrays(out, capped(want, cap), f"half the vertices, cap {cap - K:+d}", names=NAMES)
