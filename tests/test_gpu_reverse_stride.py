"""The reverse CSR past its grid caps, bit for bit against tests/reverse_ref.py.  Every kernel of the build strides a grid of at most
2 048 workgroups: the count and the scatter over tiles of 1 024 entries, the wave sort over 64 rows a wave, the workgroup sorts over
listed rows and runs, the merge over pieces of 2 048 outputs.  One graph of 5.3 million live entries takes all of them past one trip --
three trips of count and scatter, more rows of a workgroup's class than 2 048, more runs and more merge pieces than 2 048 -- with a hub
of 70 000 entries that lie in every trip.  And the scan of the counts at 2^20 - 1, 2^20 and 2^20 + 257 vertices, where it goes from one
level to two, on graphs of low degrees in which every other vertex has no out-edge.  Each input's conditions are asserted from the
reference before any launch."""
import numpy as np
import pytest
import torch

from tests import reverse_ref as ref
from tests.compare import same_arrays

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMES = ("rindptr", "rcol", "reid")
HUB = 70000
SCAN_NODES = [2 ** 20 - 1, 2 ** 20, 2 ** 20 + 257]
GRID = 2048


def stride_lengths():
    return np.array([HUB] + [ref.TILE + 4] * 1250 + [70] * 2100 + [3] * 50 + [0] * 20, dtype=np.int64)


def stride_case():
    """(indptr, col, the reference): the graph of the first test."""
    lengths = stride_lengths()
    indptr, col = ref.class_graph(lengths, 31)
    want = ref.reverse(indptr, col)
    E1 = want[2].size
    assert col.size > 2 * ref.ENTRY_STRIDE and E1 > 2 * ref.ENTRY_STRIDE, "count and scatter take three trips"
    got = np.diff(want[0])
    assert np.array_equal(np.sort(got), np.sort(lengths))
    hub = int(np.argmax(got))
    at = want[2][want[0][hub]:want[0][hub + 1]]
    trips = np.bincount(at // ref.ENTRY_STRIDE, minlength=3)
    assert got[hub] == HUB and np.all(trips >= 10000), "the hub's entries lie in every trip"
    classes = [ref.sort_class(int(x)) for x in got]
    assert classes.count("tile") > GRID, "the listed rows stride"
    long_rows = got[got > ref.TILE]
    assert sum(ref.runs(int(x)) for x in long_rows) > GRID, "the runs stride"
    assert sum(-(-min(2 * ref.TILE, int(x)) // ref.CHUNK) * 1 for x in long_rows) > GRID, "the first pass's pieces stride"
    assert (N := indptr.size - 1) > 64 * 4 and N == lengths.size
    stale = ref.stale_second_trip(indptr, col)
    assert (stale[0] != want[0]).sum() > 1000, "a stale second trip counts other entries for most vertices"
    assert not np.array_equal(ref.rows_in_scatter_order(indptr, col)[2], want[2])
    return indptr, col, want


def scan_case(N):
    """(indptr, col, the reference): N vertices, about as many entries, out-edges from the even vertices only."""
    rng = np.random.RandomState(N % 1000)
    E = N + 77
    col = (2 * rng.randint(0, (N + 1) // 2, E)).astype(np.int32)
    col[rng.randint(0, E, 500)] = -1
    row = np.sort(rng.randint(0, N, E))
    indptr = np.searchsorted(row, np.arange(N + 1), side="left").astype(np.int64)
    want = ref.reverse(indptr, col)
    lengths = np.diff(want[0])
    assert np.all(lengths[1::2] == 0) and lengths.max() <= 16 and (lengths >= 2).sum() > 10 ** 5, "low degrees, every other vertex none"
    assert ref.scan_levels(N) == (1 if N <= 2 ** 20 else 2)
    assert N > 64 * 4 * GRID, "the wave sort strides"
    assert not np.array_equal(ref.rows_in_scatter_order(indptr, col)[2], want[2])
    return indptr, col, want


def build(indptr, col):
    from legion_amd import engine
    return engine.GraphStorage(1, torch.from_numpy(indptr).to(DEV), torch.from_numpy(col).to(DEV))


def test_every_grid_strides(hip):
    indptr, col, want = stride_case()
    g = build(indptr, col)
    rev = g.reverse()
    same_arrays([rev.indptr, rev.col, rev.eids], want, "stride", NAMES)
    nodes = np.array([int(np.argmax(np.diff(want[0]))), 5, -1, indptr.size - 1, 5], dtype=np.int32)
    same_arrays(g.out_edges(nodes, return_eids=True), ref.out_edges(indptr, col, nodes), "stride out_edges", ("src", "dst", "eid"))
    torch.cuda.synchronize()
    g.close()


@pytest.mark.parametrize("N", SCAN_NODES)
def test_the_scan_from_one_level_to_two(hip, N):
    indptr, col, want = scan_case(N)
    g = build(indptr, col)
    rev = g.reverse()
    same_arrays([rev.indptr, rev.col, rev.eids], want, f"scan {N}", NAMES)
    torch.cuda.synchronize()
    g.close()
