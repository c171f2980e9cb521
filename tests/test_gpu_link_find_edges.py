"""GraphStorage.find_edges / legion_find_edges on the GPU, bit for bit against tests/link_ref.py on the symmetric graph of
tests/node2vec_ref.py: every workgroup boundary in the count, edge ids outside the graph, the ends of every hub row, the rows right
after empty rows (two of them adjacent: a lower-bound search names an empty row there), every dead entry and the last edge.  The counts
include every boundary at which one of a lane's four edge ids (256 apart in a tile of 1 024) goes dead for some lanes and not for others.
And every edge id from -2 to E + 2 on the small graphs of link_ref.small_graphs(): one to three vertices, N + 1 row pointers a power of
two and either side, leading and trailing empty rows, every edge in one row."""
import numpy as np
import pytest
import torch

from tests import link_ref as ref
from tests import node2vec_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
COUNTS = [1, 63, 64, 65, 256, 257, 512, 513, 768, 769, 1023, 1024, 1025, 2049, 5000]


@pytest.fixture(scope="module")
def world(hip):
    from legion_amd import engine
    indptr, col, _ = node2vec_ref.sym_graph()
    graph = engine.GraphStorage(1, torch.from_numpy(indptr).to(DEV), torch.from_numpy(col).to(DEV))
    yield dict(graph=graph, indptr=indptr, col=col)
    torch.cuda.synchronize()
    graph.close()


def test_the_edge_ids_exercise_every_case_before_any_launch(world):
    indptr, col = world["indptr"], world["col"]
    E = col.size
    for n in COUNTS[1:]:
        e = ref.eids_for(indptr, col, n)
        have = set(e.tolist())
        assert e.size == n and {-1, E, E + 5, E - 1} <= have
        assert all(int(indptr[h]) in have and int(indptr[h + 1]) - 1 in have for h in node2vec_ref.HUBS)
        dead = np.nonzero(col < 0)[0]
        assert dead.size == 30 and set(dead.tolist()) <= have
        assert indptr[40] == indptr[41] == indptr[42] < indptr[43] and int(indptr[42]) in have      # rows 40 and 41 are empty
        row, c = ref.find_edges(indptr, col, e)
        at = e.tolist().index(int(indptr[42]))
        assert row[at] == 42 and np.searchsorted(indptr, indptr[42], side="left") == 40              # what a lower bound would say
        assert (row < 0).sum() >= 33 and np.array_equal(row < 0, c < 0)
    assert ref.eids_for(indptr, col, 1).tolist() == [E - 1]


@pytest.mark.parametrize("n", COUNTS)
def test_find_edges_is_the_reference_bit_for_bit(world, n):
    eids = ref.eids_for(world["indptr"], world["col"], n)
    want = ref.find_edges(world["indptr"], world["col"], eids)
    got = world["graph"].find_edges(torch.from_numpy(eids).to(DEV))
    host = world["graph"].find_edges(eids)                             # eids from the host
    torch.cuda.synchronize()
    for name, g, h, w in zip(("row", "col"), got, host, want):
        g = g.cpu().numpy()
        assert g.dtype == np.int32 and g.shape == (n,)
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, f"n {n}: {bad.size} entries of {name} differ, first at {bad[0]} (eid {eids[bad[0]]}): got {g[bad[0]]} want {w[bad[0]]}"
        assert np.array_equal(h.cpu().numpy(), w), f"n {n}: {name} from host eids"


def small_case(name):
    """(indptr, col, every edge id in [-2, E + 2], reference) of a small graph.  Checked: the first and the last edge name the first and
    the last row with entries, and where an empty row precedes a row with entries a lower-bound search names an empty row."""
    indptr, col = ref.small_graphs()[name]
    E, deg = col.size, np.diff(indptr)
    eids = np.arange(-2, E + 3, dtype=np.int64)
    want = ref.find_edges(indptr, col, eids)
    full = np.nonzero(deg > 0)[0]
    live = np.nonzero(col >= 0)[0]
    owner = np.repeat(np.arange(deg.size), deg)
    assert np.array_equal(want[0][live + 2], owner[live]) and np.array_equal(want[1][live + 2], col[live])
    assert np.all(want[0][[0, 1, E + 2, E + 3, E + 4]] == -1) and np.all(want[1][[0, 1, E + 2, E + 3, E + 4]] == -1)
    assert (col[0] < 0 or want[0][2] == full[0]) and (col[E - 1] < 0 or want[0][E + 1] == full[-1])
    if np.any((deg[:-1] == 0) & (deg[1:] > 0)):
        wrong = ref.find_edges_lower_bound(indptr, col, eids)[0]
        named = wrong[wrong != want[0]]
        assert named.size >= 1 and np.all(deg[named] == 0), name
    return indptr, col, eids, want


@pytest.mark.parametrize("name", sorted(ref.small_graphs()))
def test_every_edge_id_of_a_small_graph(hip, name):
    from legion_amd import engine
    indptr, col, eids, want = small_case(name)
    g = engine.GraphStorage(1, torch.from_numpy(indptr).to(DEV), torch.from_numpy(col).to(DEV))
    try:
        got = g.find_edges(torch.from_numpy(eids).to(DEV))
        torch.cuda.synchronize()
        for what, x, w in zip(("row", "col"), got, want):
            x = x.cpu().numpy()
            bad = np.nonzero(x != w)[0]
            assert x.dtype == np.int32 and x.shape == w.shape and bad.size == 0, \
                f"{name} (N {indptr.size - 1}, E {col.size}): {what} differs at edge ids {eids[bad][:5]}: got {x[bad][:5]} want {w[bad][:5]}"
    finally:
        torch.cuda.synchronize()
        g.close()


def test_an_empty_call_returns_empty_arrays(world):
    row, col = world["graph"].find_edges(np.zeros(0, np.int64))
    assert row.shape == (0,) and col.shape == (0,) and row.dtype == torch.int32 and col.dtype == torch.int32
