"""Layer-neighbour sampling past one trip of the capped grid (2 048 workgroups) and past one run of the scan, bit for bit against
tests/labor_ref.py.  Two inputs:
  * seeds_for(5000) on the symmetric graph of tests/node2vec_ref.py: 4 126 670 slots, more than one stride of 2 048 x 1 024, with 999
    copies of the hub: a second trip that repeats the tile one stride earlier keeps other slots;
  * 2^17 + 1 copies of one row of 1 030 entries: 135 005 190 slots, 131 842 tiles and 516 second-level sums, so a scan thread's run
    holds three of them, and since 1 030 is no divisor of 1 024 the tile boundaries drift through the rows.  The reference tiles one
    row's mask: numpy never expands the slots."""
import functools

import numpy as np
import pytest
import torch

from tests import in_edges_ref
from tests import labor_ref as ref
from tests import node2vec_ref
from tests.compare import same_arrays

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HUB = 6
BIG_M = 4126670
WIDE, COPIES = 1030, 2 ** 17 + 1


def slot_case(indptr, col, fanout=25, salt=0):
    """(rows, offsets, kept mask, K, dst, src, eid) of seeds_for(5000)."""
    rows = node2vec_ref.seeds_for(5000)
    off = in_edges_ref.row_offsets(indptr, rows)
    M = int(off[-1])
    assert M == BIG_M > ref.STRIDE and (rows == HUB).sum() == 999
    kept = ref.slot_mask(indptr, col, rows, off, M, fanout, salt)[0]
    K, dst, src, eid = ref.edges(indptr, col, rows, off, M, fanout, salt)
    stale = ref.stale_second_trip(kept)
    assert (stale != kept).sum() >= 1000 and int(stale.sum()) != K, "a stale second trip keeps other slots, and another number of them"
    assert int(kept[ref.STRIDE:].sum()) >= 1000, "the second trip keeps entries"
    return rows, off, kept, K, dst, src, eid


def wide_graph():
    """One row of 1 030 entries (vertex 0: the vertices 1 .. 1 030, five of them dead) and a ring over the rest."""
    n = WIDE + 1
    row0 = np.arange(1, n, dtype=np.int32)
    row0[[0, 100, 511, 512, 1029]] = -1
    ring = np.stack([(np.arange(1, n) - 1) % n, (np.arange(1, n) + 1) % n], axis=1).astype(np.int32)
    ring.sort(axis=1)
    indptr = np.concatenate([[0], [WIDE], WIDE + 2 * np.arange(1, n)]).astype(np.int64)
    return indptr, np.concatenate([row0, ring.reshape(-1)]).astype(np.int32)


def wide_case(fanout=10, salt=5):
    """(indptr, col, rows, K, dst, src, eid): COPIES copies of row 0, the reference by tiling one row's mask."""
    indptr, col = wide_graph()
    one = np.zeros(1, dtype=np.int32)
    kept, _, src, eid = ref.slot_mask(indptr, col, one, np.array([0, WIDE], np.int64), WIDE, fanout, salt)
    k = int(kept.sum())
    assert 3 <= k <= 20 and WIDE % ref.TILE != 0
    M = COPIES * WIDE
    tiles = ref.tiles_of(M)
    groups = (tiles + ref.GROUP - 1) // ref.GROUP
    assert (M, tiles, groups) == (135005190, 131842, 516) and (groups + 255) // 256 == 3 and M <= ref.MAX_SLOTS
    assert ref.scratch_bytes(M) == 8 * (tiles + 1 + groups)
    rows = np.zeros(COPIES, dtype=np.int32)
    dst = np.repeat(np.arange(COPIES, dtype=np.int32), k)
    return indptr, col, rows, COPIES * k, dst, np.tile(src[kept], COPIES), np.tile(eid[kept], COPIES)


def test_the_cases_hold_their_conditions_before_any_launch():
    indptr, col, _ = node2vec_ref.sym_graph()
    slot_case(indptr, col)
    indptr, col, rows, K, dst, src, eid = wide_case()
    small = ref.edges_full(indptr, col, rows[:7], 10, 5)               # the tiling is the reference on a few copies
    k = K // COPIES
    assert np.array_equal(small[0], dst[:7 * k]) and np.array_equal(small[1], src[:7 * k]) and np.array_equal(small[2], eid[:7 * k])


same_labor = functools.partial(same_arrays, names=("dst", "src", "eid"))


def test_more_slots_than_one_stride(hip):
    from legion_amd import engine
    indptr, col, _ = node2vec_ref.sym_graph()
    rows, off, kept, K, dst, src, eid = slot_case(indptr, col)
    g = engine.GraphStorage(1, torch.from_numpy(indptr).to(DEV), torch.from_numpy(col).to(DEV))
    try:
        got = g.labor_edges(torch.from_numpy(rows).to(DEV), 25, return_eids=True)
        torch.cuda.synchronize()
        same_labor(got, (dst, src, eid), "5 000 seeds")
        got = g.labor_edges(torch.from_numpy(rows).to(DEV), 25)
        torch.cuda.synchronize()
        same_labor(got, (dst, src), "5 000 seeds, no edge ids")
    finally:
        torch.cuda.synchronize()
        g.close()


def test_more_tiles_than_one_run_of_the_scan(hip):
    from legion_amd import engine
    indptr, col, rows, K, dst, src, eid = wide_case()
    g = engine.GraphStorage(1, torch.from_numpy(indptr).to(DEV), torch.from_numpy(col).to(DEV))
    try:
        got = g.labor_edges(torch.from_numpy(rows).to(DEV), 10, salt=5, return_eids=True)
        torch.cuda.synchronize()
        assert got[0].shape == (K,)
        same_labor(got, (dst, src, eid), f"{COPIES} copies of a row of {WIDE}")
    finally:
        torch.cuda.synchronize()
        g.close()
