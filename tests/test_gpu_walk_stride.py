"""One stride of the grid and a bit: random_walk_kernel, node2vec_walk_kernel and pinsage_neighbors_kernel cap their grids at 2 048 workgroups, so a call of
more than 2 048 tiles sends workgroups 0 and 1 through the tile loop a second time -- the staging arrays reused, the visit array
refilled, `live` and the per-trip n1 / w0 formed again.  Here every instance family runs 2 050 tiles (the last with one live row) on
the hand-built graph of tests/walk_ref.py, whole arrays bit for bit against the references.

Before the GPU runs, each test checks from the reference alone that a wrong second trip could not pass:
  1. the expected rows of every second-trip tile t differ from those of tile t - 2048 (a stale tile shows);
  2. PinSAGE: at some slot the seed of tile 0 has visits and the seed of tile 2048 lies outside the graph (a missed refill shows as
     visits where -1 / 0 belongs).  The tile-0 seed has at least R visits -- every walk's first step; all R * T of them cannot be
     asked for: beyond the first step each visit survives a termination draw that depends on the draw index alone, and the shapes
     here leave 56 to 960 such draws per seed at p >= 0.3;
  3. PinSAGE: of the second-trip seeds inside the graph at most 10 % have an empty expected row.  (The seeds placed outside the graph
     are not counted: the 1 024 class has three second-trip seeds, one of them the -1 of condition 2.  A walk's row is never empty:
     it starts with its seed.)"""
import numpy as np
import pytest
import torch

from tests import functional_ref
from tests import node2vec_ref
from tests import pinsage_ref
from tests import walk_ref
from tests import weighted_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MAX_WG = 2048                                                      # LG_WALK_MAX_WG
BASE = 40
# what goes into tile 2048 from its slot 1 on, in this order, as far as the second trip has room before its last seed: the seeds
# outside the graph first (slot 1 of tile 0 is vertex 1, one entry: R visits), then the special rows, the empty ones (0; 10 when
# weighted) last
PLACED = [-1, walk_ref.NODE_NUM, 9, 3, 4, 5, 6, 7, 8, 1, 2, 11, 0, 10]


def stride_seeds(S):
    """n = 2048 S + S + 1 seeds in the multiplicative pattern of walk_ref.seeds_for over the whole graph, the special rows at the front
    and, with a -1 and a NODE_NUM, inside the second trip.  Short second trips (8 or 2 seeds to a tile) take the part of PLACED that
    leaves fewer than a tenth of their seeds with an empty row."""
    n = MAX_WG * S + S + 1
    s = (np.arange(n, dtype=np.int64) * 2654435761 % walk_ref.NODE_NUM).astype(np.int32)
    s[:12] = np.arange(12, dtype=np.int32)
    s[n // 2] = s[0]                                               # a repeat
    room = S - 1                                                   # slots 1 .. of tile 2048 (and on into tile 2049), never the last seed
    placed = PLACED[:room] if S >= 32 else PLACED[:min(room, 12)]
    s[MAX_WG * S + 1:MAX_WG * S + 1 + len(placed)] = placed
    return s


def _second_trip(n, S):
    """[(tile, first row, live rows)] of the tiles from 2 048 on."""
    return [(t, t * S, min(S, n - t * S)) for t in range(MAX_WG, (n + S - 1) // S)]


def _name(i, S):
    t = i // S
    return f"row {i}: tile {t}, slot {i % S}, {'second' if t >= MAX_WG else 'first'} trip of workgroup {t % MAX_WG}"


def _assert_same(got, want, S, ctx):
    """Whole arrays; a failure names the first rows that differ with their tiles and trips."""
    for g, w, what in zip(got, want, ctx[1]):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (ctx[0], what)
        if np.array_equal(g, w):
            continue
        rows = np.nonzero((g != w).any(axis=1))[0]
        late = int((rows >= MAX_WG * S).sum())
        raise AssertionError(f"{ctx[0]}: {what} differ in {rows.size} rows, {late} of them on a second trip; first " +
                             "; ".join(f"{_name(int(i), S)}: got {g[i][:8]} want {w[i][:8]}" for i in rows[:3]))


@pytest.fixture(scope="module")
def world(hip):
    from legion_amd import engine
    indptr, col, w = walk_ref.hand_graph()
    g = engine.GraphStorage(1, torch.from_numpy(indptr).to(DEV), torch.from_numpy(col).to(DEV))
    g.set_edge_weights(w)
    torch.cuda.synchronize()
    table = weighted_ref.cdf(indptr, w)
    assert np.array_equal(g.edge_cdf().cpu().numpy().view(np.uint32), table.view(np.uint32)), "edge_cdf"
    yield dict(graph=g, indptr=indptr, col=col, table=table)
    g.close()


# ---- walks ------------------------------------------------------------------------------------------------------------------------
def walk_case(indptr, col, table, length, weighted):
    """(seeds, reference) of a walk case, its conditions checked."""
    S = 256
    seeds = stride_seeds(S)
    assert seeds.size == 524545 and (seeds.size + S - 1) // S == 2050
    reads = {} if length == 2 else None                            # (the vertices a walk can stand on do not depend on its length)
    want = walk_ref.walk(indptr, col, seeds, length, table=table if weighted else None, restart_prob=0.3 if weighted else 0.0, base=BASE,
                         reads=reads)
    walk_ref.assert_reads_in_bounds(reads or {}, walk_ref.NODE_NUM, col.size)
    for t, r0, live in _second_trip(seeds.size, S):
        old = r0 - MAX_WG * S
        assert not np.array_equal(want[0][r0:r0 + live], want[0][old:old + live]), f"tile {t} expects what tile {t - MAX_WG} does"
        assert (want[0][r0:r0 + live, 1] >= 0).any(), f"no walk of tile {t} takes a step"
    late = seeds[MAX_WG * S:]
    assert -1 in late and walk_ref.NODE_NUM in late and set(range(12)) <= set(late.tolist())
    return seeds, want


@pytest.mark.parametrize("weighted", [False, True], ids=["uniform-plain", "weighted-restart-edge-ids"])
@pytest.mark.parametrize("length", [2, 17])
def test_walks_over_one_grid_stride_and_a_bit(world, length, weighted):
    """2 050 tiles of 256 walks; length 2 is one chunk, 17 two chunks plain and three with edge ids."""
    seeds, want = walk_case(world["indptr"], world["col"], world["table"], length, weighted)
    ctx = f"{seeds.size} walks x {length}, {'weighted, restart 0.3, edge ids' if weighted else 'uniform'}"
    if weighted:
        got = world["graph"].random_walk(seeds, length, weighted=True, restart_prob=0.3, return_eids=True, base=BASE)
        torch.cuda.synchronize()
        _assert_same(got, want, 256, (ctx, ("traces", "edge ids")))
    else:
        got = world["graph"].random_walk(seeds, length, base=BASE)
        torch.cuda.synchronize()
        _assert_same((got,), want[:1], 256, (ctx, ("traces",)))


# ---- node2vec: the same tile code, on the world with every row sorted ---------------------------------------------------------------
N2V_WALKS = (MAX_WG + 2) * 256                                     # 2 050 full tiles
N2V_TILES = (0, MAX_WG - 1, MAX_WG, MAX_WG + 1)                    # a first trip's first and last tile, both second-trip tiles


@pytest.fixture(scope="module")
def sorted_world(hip):
    """The hand-built graph with the entries of every row (and their weights) in ascending order, dead entries first: what node2vec's
    search of a row needs."""
    from legion_amd import engine
    indptr, col, w = walk_ref.hand_graph()
    rows = np.repeat(np.arange(walk_ref.NODE_NUM), np.diff(indptr))
    order = np.lexsort((col, rows))
    col, w = col[order], w[order]
    assert node2vec_ref.rows_sorted(indptr, col)
    g = engine.GraphStorage(1, torch.from_numpy(indptr).to(DEV), torch.from_numpy(col).to(DEV))
    g.set_edge_weights(w)
    torch.cuda.synchronize()
    table = weighted_ref.cdf(indptr, w)
    assert np.array_equal(g.edge_cdf().cpu().numpy().view(np.uint32), table.view(np.uint32)), "edge_cdf"
    seeds = (np.arange(N2V_WALKS, dtype=np.int64) * 2654435761 % walk_ref.NODE_NUM).astype(np.int32)
    for t in N2V_TILES:                                            # the special rows lead each checked tile; the long rows often: walks
        seeds[t * 256:t * 256 + 12] = np.arange(12)                # leave them and search them on the step after
        seeds[t * 256 + 12:(t + 1) * 256:5] = [9, 8, 7, 6, 5][t % 5]
    seeds[MAX_WG * 256 + 1:MAX_WG * 256 + 3] = [-1, walk_ref.NODE_NUM]
    yield dict(graph=g, indptr=indptr, col=col, table=table, seeds=seeds)
    g.close()


@pytest.mark.parametrize("length, full", [(2, False), (17, True)], ids=["2-uniform-plain", "17-weighted-edge-ids"])
def test_node2vec_walks_over_one_grid_stride_and_a_bit(sorted_world, length, full):
    """2 050 tiles of 256 walks through node2vec_walk_kernel.  p = q = 1: every walk is random_walk's (the rule says so), whole arrays
    against walk_ref.  p = 0.25, q = 4: the walks of four tiles against node2vec_ref, computed for those walks alone at their own
    draw indices (a walk depends only on its seed and its draw indices)."""
    w = sorted_world
    g, indptr, col, seeds = w["graph"], w["indptr"], w["col"], w["seeds"]
    table = w["table"] if full else None
    assert seeds.size == 524800 and seeds.size // 256 == MAX_WG + 2
    plain = walk_ref.walk(indptr, col, seeds, length, table=table, base=BASE)
    for t, r0, live in _second_trip(seeds.size, 256):
        old = r0 - MAX_WG * 256
        assert not np.array_equal(plain[0][r0:r0 + live], plain[0][old:old + live]), f"tile {t} expects what tile {t - MAX_WG} does"
    stats, reads, biased = node2vec_ref.new_stats(), {}, {}
    for t in N2V_TILES:
        r0 = t * 256
        biased[t] = node2vec_ref.walk(indptr, col, seeds[r0:r0 + 256], length, 0.25, 4.0, table=table, base=BASE + r0 * length, reads=reads,
                                      stats=stats)
    walk_ref.assert_reads_in_bounds(reads, walk_ref.NODE_NUM, col.size)
    print("rejected", stats["rejected"], "searches", stats["searches"])
    assert sum(stats["rejected"]) > 0 and stats["searches"] > 0, "no walk of the four tiles rejects a candidate, or none searches a row"
    kw = dict(weighted=full, return_eids=full, base=BASE)
    what = ("traces", "edge ids") if full else ("traces",)
    got = g.node2vec_random_walk(seeds, 1.0, 1.0, length, **kw)
    torch.cuda.synchronize()
    _assert_same(got if full else (got,), plain[:len(what)], 256, (f"{seeds.size} walks x {length}, p = q = 1", what))
    got = g.node2vec_random_walk(seeds, 0.25, 4.0, length, **kw)
    torch.cuda.synchronize()
    got = got if full else (got,)
    for t in N2V_TILES:
        for x, want, name in zip(got, biased[t], what):
            x = x[t * 256:(t + 1) * 256].cpu().numpy()
            assert x.dtype == want.dtype and np.array_equal(x, want), \
                f"p = 0.25, q = 4, length {length}: {name} of tile {t} differ in rows {np.nonzero((x != want).any(axis=1))[0][:8]}"


# ---- PinSAGE ----------------------------------------------------------------------------------------------------------------------
SHAPES = [(32, 10, 2, 3, 131137), (64, 7, 9, 5, 65569), (256, 65, 3, 200, 16393), (1024, 64, 16, 10, 4099)]


def pinsage_case(indptr, col, table, shape, weighted):
    """(seeds, reference) of a PinSAGE case, its conditions checked."""
    vpad, R, T, k, n = shape
    S = 2048 // vpad
    seeds = stride_seeds(S)
    assert seeds.size == n == MAX_WG * S + S + 1 and (n + S - 1) // S == MAX_WG + 2 and (n - 1) % S == 0
    assert functional_ref.vpad(R * T) == vpad
    reads = {}
    vis = pinsage_ref.visits(indptr, col, seeds, R, T, table=table if weighted else None, termination_prob=0.3 if weighted else 0.5,
                             base=BASE, reads=reads)
    walk_ref.assert_reads_in_bounds(reads, walk_ref.NODE_NUM, col.size)
    want = pinsage_ref.topk(vis, k)
    for t, r0, live in _second_trip(n, S):                         # 1.
        old = r0 - MAX_WG * S
        assert not (np.array_equal(want[0][r0:r0 + live], want[0][old:old + live]) and
                    np.array_equal(want[1][r0:r0 + live], want[1][old:old + live])), f"tile {t} expects what tile {t - MAX_WG} does"
    visits = (vis >= 0).sum(axis=1)
    r0 = MAX_WG * S                                                # 2.
    outside = (seeds[r0:r0 + S] < 0) | (seeds[r0:r0 + S] >= walk_ref.NODE_NUM)
    assert (outside & (visits[:S] >= R)).any(), "no slot with visits in tile 0 and a seed outside the graph in tile 2048"
    assert np.all(want[0][r0:r0 + S][outside] == -1) and np.all(want[1][r0:r0 + S][outside] == 0)
    late = seeds[r0:]                                              # 3.
    inside = (late >= 0) & (late < walk_ref.NODE_NUM)
    empty = int((visits[r0:][inside] == 0).sum())
    assert inside.any() and empty * 10 <= int(inside.sum()), f"{empty} of {int(inside.sum())} second-trip seeds have an empty row"
    assert visits[n - 1] > 0, "the one live row of the last tile is empty"
    return seeds, want


@pytest.mark.parametrize("weighted", [False, True], ids=["uniform-0.5", "weighted-0.3"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"class{s[0]}-{s[1]}x{s[2]}x{s[3]}")
def test_neighbours_over_one_grid_stride_and_a_bit(world, shape, weighted):
    """2 050 tiles of S seeds per visit class, the last with one live seed."""
    vpad, R, T, k, n = shape
    seeds, want = pinsage_case(world["indptr"], world["col"], world["table"], shape, weighted)
    got = world["graph"].pinsage_neighbors(seeds, R, T, k, termination_prob=0.3 if weighted else 0.5, weighted=weighted, base=BASE)
    torch.cuda.synchronize()
    ctx = f"{n} seeds, class {vpad}, (R, T, k) = {(R, T, k)}, {'weighted, 0.3' if weighted else 'uniform, 0.5'}"
    _assert_same(got, want, 2048 // vpad, (ctx, ("neighbours", "counts")))
