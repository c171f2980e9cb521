"""find_edges and negative_sample at edge offsets beyond 2^31 and 2^32: the layout of tests/far_rows.py, whose live rows straddle the
boundary behind ballast rows of L zeros, put on the device by far_rows.device_world (without the weights: neither op reads them).  The
references run on the reference view; the whole column array exists on the device only.  A failure at 5000 is a fault at any size; at
2^31 but not at 5000 an offset that went through a signed 32-bit value; at 2^32 only, through an unsigned one."""
import numpy as np
import pytest
import torch

from tests import far_rows
from tests import link_ref as ref
from tests.compare import same_arrays

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module", params=list(far_rows.BOUNDARIES))
def world(hip, request):
    """The whole graph on the device at one boundary (far_rows.device_world)."""
    with far_rows.device_world(hip, request.param) as w:
        yield w


def far_eids(g):
    """(true eids, want row, want col): live edge ids on both sides of the boundary, both ends of the straddling row, ballast edge ids
    (the answer is (e // L, 0)), a dead entry, and ids outside the graph."""
    live = (np.arange(400, dtype=np.int64) * 2654435761 % g.live_E)
    live = np.concatenate([live, [0, g.live_E - 1, g.k - 1, g.k, int(g.indptr[g.hub]) - g.offset, int(g.indptr[g.hub + 1]) - 1 - g.offset],
                           np.nonzero(g.col_ref < 0)[0][:5]])
    row, c = ref.find_edges(g.indptr_ref, g.col_ref, live)
    true = live + g.offset
    took = row >= 0
    assert (took & (true < g.boundary)).sum() >= 10 and (took & (true >= g.boundary)).sum() >= 10, "live edge ids on both sides"
    assert (~took).sum() >= 5 and np.all(row[took] >= g.B), "dead entries; every live edge's row is a live vertex"
    ends = [int(g.indptr[g.hub]), int(g.indptr[g.hub + 1]) - 1]
    assert ends[0] < g.boundary <= ends[1] and all(row[true.tolist().index(e)] in (g.hub, -1) for e in ends), "both ends of the straddler"
    ballast = np.array([0, 1, g.L - 1, g.L, g.L + 1, g.offset // 2, g.offset - g.L, g.offset - 2, g.offset - 1] +
                       [min(b, g.offset - 1) for b in (2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1)], dtype=np.int64)
    assert np.all((ballast >= 0) & (ballast < g.offset))
    b_row = (ballast // g.L).astype(np.int32)
    assert np.all((g.indptr[b_row] <= ballast) & (ballast < g.indptr[b_row.astype(np.int64) + 1])) and b_row.max() == g.B - 1
    outside = np.array([-1, g.E, g.E + 5, -2 ** 40], dtype=np.int64)
    eids = np.concatenate([true, ballast, outside])
    want_row = np.concatenate([row, b_row, np.full(outside.size, -1, np.int32)])
    want_col = np.concatenate([c, np.zeros(ballast.size, np.int32), np.full(outside.size, -1, np.int32)])
    order = np.random.RandomState(5).permutation(eids.size)
    return eids[order], want_row[order], want_col[order]


def test_find_edges(world):
    g = world["g"]
    eids, want_row, want_col = far_eids(g)
    row, c = world["graph"].find_edges(torch.from_numpy(eids).to(DEV))
    torch.cuda.synchronize()
    row, c = row.cpu().numpy(), c.cpu().numpy()
    bad = np.nonzero((row != want_row) | (c != want_col))[0]
    assert bad.size == 0, f"{bad.size} edges differ, first eid {eids[bad[0]]}: got ({row[bad[0]]}, {c[bad[0]]}) want " \
                          f"({want_row[bad[0]]}, {want_col[bad[0]]})" + world["why"]


def want_negatives(g, count, k, tries, base):
    """The reference on the view, with the true node_num; the searches and hits in rows that start beyond the boundary."""
    rows = g.seeds(count)
    stats, reads = ref.new_stats(g.node_num), {}
    want = ref.negative_sample(g.indptr_ref, g.col_ref, rows, k, 3, tries, base, reads=reads, stats=stats)
    assert g.indptr_ref.size == g.node_num + 1
    g.assert_no_ballast_read(reads, view=True)
    beyond = g.indptr[:-1] > g.boundary
    far_searches, far_hits = int(stats["searches_of_row"][beyond].sum()), int(stats["hits_of_row"][beyond].sum())
    assert far_searches >= 10 and far_hits >= 10, f"{far_searches} searches and {far_hits} hits beyond the boundary"
    assert stats["hits_of_row"][g.hub] >= 10, "the straddling row is hit"
    return rows, want


@pytest.mark.parametrize("count, k, tries, base", [(5000, 5, 256, 0), (5000, 5, 2, 1234567890)])
def test_negative_sample(world, count, k, tries, base):
    g = world["g"]
    rows, want = want_negatives(g, count, k, tries, base)
    got = world["graph"].negative_sample(torch.from_numpy(rows).to(DEV), k, max_tries=tries, base=base)
    torch.cuda.synchronize()
    same_arrays(got, want, f"negative_sample {count} x {k} tries {tries} base {base}" + world["why"], names=["negatives (row, slot)"])
