"""One stride of the grid and a bit: node2vec_walk_kernel caps its grid at 2 048 workgroups, so a call of more than 2 048 tiles sends
workgroups 0 and 1 through the tile loop a second time -- the staging arrays reused, and the lane state of the first trip (the previous
vertex and its row, the try counter, the draw) formed again.  Here 524 545 walks (2 050 tiles, the last with one live row) run on the
symmetric graph of tests/node2vec_ref.py at lengths 2 and 17, (0.5, 2) uniform without edge ids and (4, 0.25) weighted with them, whole
arrays bit for bit against the reference.

Before the GPU runs, each test checks from the reference alone that a wrong second trip could not pass: the expected rows of every
second-trip tile differ from those of the tile 2 048 before it, some walk of the tile takes a step, and the seeds outside the graph
and the hub rows are among the second trip's."""
import numpy as np
import pytest
import torch

from tests import node2vec_ref as ref
from tests import walk_ref
from tests import weighted_ref
from tests.test_gpu_walk_stride import MAX_WG, _assert_same, _second_trip, stride_seeds

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BASE = 40
assert ref.NODE_NUM == walk_ref.NODE_NUM                           # stride_seeds places a node_num of walk_ref's


@pytest.fixture(scope="module")
def world(hip):
    from legion_amd import engine
    indptr, col, w = ref.sym_graph()
    g = engine.GraphStorage(1, torch.from_numpy(indptr).to(DEV), torch.from_numpy(col).to(DEV))
    g.set_edge_weights(w)
    torch.cuda.synchronize()
    table = weighted_ref.cdf(indptr, w)
    assert np.array_equal(g.edge_cdf().cpu().numpy().view(np.uint32), table.view(np.uint32)), "edge_cdf"
    yield dict(graph=g, indptr=indptr, col=col, table=table)
    g.close()


def stride_case(indptr, col, table, length, weighted):
    """(seeds, reference) of a case, its conditions checked."""
    S = 256
    seeds = stride_seeds(S)
    assert seeds.size == 524545 and (seeds.size + S - 1) // S == 2050
    reads = {} if length == 2 else None                            # (the vertices a walk can stand on do not depend on its length)
    p, q = (4.0, 0.25) if weighted else (0.5, 2.0)
    stats = ref.new_stats()
    want = ref.walk(indptr, col, seeds, length, p, q, table=table if weighted else None, base=BASE, reads=reads, stats=stats)
    walk_ref.assert_reads_in_bounds(reads or {}, ref.NODE_NUM, col.size)
    for t, r0, live in _second_trip(seeds.size, S):
        old = r0 - MAX_WG * S
        assert not np.array_equal(want[0][r0:r0 + live], want[0][old:old + live]), f"tile {t} expects what tile {t - MAX_WG} does"
        assert (want[0][r0:r0 + live, 1] >= 0).any(), f"no walk of tile {t} takes a step"
    late = seeds[MAX_WG * S:]
    assert -1 in late and ref.NODE_NUM in late and set(range(12)) <= set(late.tolist())
    if length > 1:
        assert sum(stats["rejected"]) > 1000 and stats["searches"] > 1000      # the loop rejects and searches on both trips
    return seeds, want


@pytest.mark.parametrize("weighted", [False, True], ids=["uniform-plain", "weighted-edge-ids"])
@pytest.mark.parametrize("length", [2, 17])
def test_walks_over_one_grid_stride_and_a_bit(world, length, weighted):
    """2 050 tiles of 256 walks; length 2 is one chunk, 17 two chunks plain and three with edge ids."""
    seeds, want = stride_case(world["indptr"], world["col"], world["table"], length, weighted)
    ctx = f"{seeds.size} walks x {length}, {'(4, 0.25) weighted, edge ids' if weighted else '(0.5, 2) uniform'}"
    if weighted:
        got = world["graph"].node2vec_random_walk(seeds, 4.0, 0.25, length, weighted=True, return_eids=True, base=BASE)
        torch.cuda.synchronize()
        _assert_same(got, want, 256, (ctx, ("traces", "edge ids")))
    else:
        got = world["graph"].node2vec_random_walk(seeds, 0.5, 2.0, length, base=BASE)
        torch.cuda.synchronize()
        _assert_same((got,), want[:1], 256, (ctx, ("traces",)))
