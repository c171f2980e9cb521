"""row_offsets and in_edges past one trip of the capped grid (2 048 workgroups), bit for bit against tests/in_edges_ref.py on the
symmetric graph of tests/node2vec_ref.py.  seeds_for(5000) gives 4 126 670 slots, more than one stride of 2 048 x 1 024 with 999 copies
of the hub: a second trip that repeats the tile one stride earlier differs in most of its slots.  524 289, 524 545 and 2^20 rows of low
degree, every other one without entries, cross the offsets kernels' stride of 2 048 x 256 rows (the second trip holds a hub, empty and
out-of-graph seeds) and take the scan's runs of tiles from 1 through 2 and 9 to 16."""
import functools

import numpy as np
import pytest
import torch

from tests import in_edges_ref as ref
from tests import node2vec_ref
from tests.compare import same_arrays

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = node2vec_ref.NODE_NUM
HUB = 6
ROW_COUNTS = [65536, 65537, 524289, 524545, 2 ** 20]
BIG_M = 4126670


@pytest.fixture(scope="module")
def world(hip):
    from legion_amd import engine
    indptr, col, _ = node2vec_ref.sym_graph()
    graph = engine.GraphStorage(1, torch.from_numpy(indptr).to(DEV), torch.from_numpy(col).to(DEV))
    yield dict(graph=graph, indptr=indptr, col=col)
    torch.cuda.synchronize()
    graph.close()


def slot_case(indptr, col):
    """(rows, reference) of seeds_for(5000), and the share of the second trip's slots a stale trip gets wrong."""
    rows = node2vec_ref.seeds_for(5000)
    want = ref.in_edges_full(indptr, col, rows)
    M = int(want[0][-1])
    assert M == BIG_M > ref.STRIDE and (rows == HUB).sum() == 999
    late = M - ref.STRIDE
    for w in want[1:]:
        assert (ref.stale_second_trip(w, ref.STRIDE) != w).sum() * 2 >= late, "half of the second trip's slots at least"
    second = rows[np.unique(want[1][ref.STRIDE:])]
    assert HUB in second and (second != HUB).sum() >= 100
    return rows, want


def low_rows(indptr, n):
    """n rows of degree 1 .. 12, every other one without entries (an empty row, -1, node_num); past the rows' stride a hub first."""
    deg = np.diff(indptr)
    plain = np.nonzero((deg >= 1) & (deg <= 12))[0]
    i = np.arange(n, dtype=np.int64)
    rows = plain[i * 2654435761 % plain.size]
    none = np.array(list(node2vec_ref.EMPTY) + [-1, N], dtype=np.int64)
    rows[1::2] = none[(i[1::2] // 2) % none.size]
    if n > ref.ROW_STRIDE:
        rows[ref.ROW_STRIDE] = HUB
    return rows.astype(np.int32)


def row_case(indptr, n):
    rows = low_rows(indptr, n)
    want = ref.row_offsets(indptr, rows)
    tiles = (n + ref.ROW_TILE - 1) // ref.ROW_TILE
    per = (tiles + 255) // 256
    assert (n, per) in ((65536, 1), (65537, 2), (524289, 9), (524545, 9), (2 ** 20, 16))
    if n > ref.ROW_STRIDE:
        late = rows[ref.ROW_STRIDE:]
        assert late[0] == HUB and (n < ref.ROW_STRIDE + 4 or ({-1, N, 7} <= set(late.tolist())))
        assert not np.array_equal(ref.stale_second_trip(want[:-1], ref.ROW_STRIDE), want[:-1])
        deg = np.diff(want)
        assert not np.array_equal(ref.stale_second_trip(deg, ref.ROW_STRIDE), deg), "the degree kernel's second trip"
    if n == 2 ** 20:
        assert ref.STRIDE < want[-1] < 2.2 * ref.STRIDE, "near four million slots"
    return rows, want


def test_the_cases_hold_their_conditions_before_any_launch(world):
    slot_case(world["indptr"], world["col"])
    for n in ROW_COUNTS:
        row_case(world["indptr"], n)


same_in_edges = functools.partial(same_arrays, names=("offsets", "dst", "src", "eid"))


def test_more_slots_than_one_stride(world):
    rows, want = slot_case(world["indptr"], world["col"])
    got = world["graph"].in_edges(torch.from_numpy(rows).to(DEV), return_eids=True)
    torch.cuda.synchronize()
    same_in_edges(got, want, "5 000 seeds")
    got = world["graph"].in_edges(torch.from_numpy(rows).to(DEV))
    torch.cuda.synchronize()
    same_in_edges(got, want[:3], "5 000 seeds, no edge ids")


@pytest.mark.parametrize("n", ROW_COUNTS)
def test_more_rows_than_one_stride(world, n):
    indptr, col = world["indptr"], world["col"]
    rows, off = row_case(indptr, n)
    if n < ref.ROW_STRIDE:
        got = world["graph"].row_offsets(torch.from_numpy(rows).to(DEV))
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), off)
        return
    want = (off,) + ref.in_edges(indptr, col, rows, off, int(off[-1]))
    got = world["graph"].in_edges(torch.from_numpy(rows).to(DEV), return_eids=True)
    torch.cuda.synchronize()
    same_in_edges(got, want, f"{n} rows")
    assert np.array_equal(np.unique(want[1]), np.nonzero(np.diff(off) > 0)[0]), "no row with entries is skipped"
