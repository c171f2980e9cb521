"""row_offsets and in_edges at edge offsets beyond 2^31 and 2^32: the layout of tests/far_rows.py, whose live rows straddle the boundary
behind ballast rows of L zeros, put on the device by far_rows.device_world.  The seeds are live rows on both sides of the
boundary, the straddling hub and one ballast row (its expected entries are all 0), so the edge ids lie on both sides of the boundary and
col is read beyond it; every row of the graph at once takes the offsets themselves past the boundary.  The whole column array exists on
the device only.  A failure at 5000 is a fault at any size; at 2^31 but not at 5000 an offset that went through a signed 32-bit value; at
2^32 only, through an unsigned one."""
import numpy as np
import pytest
import torch

from tests import far_rows
from tests import in_edges_ref as ref
from tests.compare import same_arrays

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module", params=list(far_rows.BOUNDARIES))
def world(hip, request):
    """The whole graph on the device at one boundary (far_rows.device_world)."""
    with far_rows.device_world(hip, request.param) as w:
        yield w


def want_in_edges(g, ballast_row):
    """(rows, offsets, dst, src, true eids): the live seeds of the layout with the straddler every fifth, one whole ballast row in the
    middle and every live row once behind it.  The live entries come from the reference view, the ballast row's are 0."""
    rows, offsets, i, r, eid, is_live, src = far_rows.expand_rows(g, ballast_row)
    M = int(offsets[-1])
    # what makes the case worth running at this boundary
    assert (~is_live).sum() == g.deg[ballast_row] >= 64 and np.all(r[~is_live] == ballast_row), "one ballast row, whole"
    low, high = is_live & (eid < g.boundary), is_live & (eid >= g.boundary)
    assert low.sum() >= 10 and high.sum() >= 10, "live edge ids on both sides"
    hub = r == g.hub
    assert (hub & low).sum() >= 10 and (hub & high).sum() >= 10, "the straddling row is read on both sides"
    assert np.all((eid >= g.indptr[r]) & (eid < g.indptr[r + 1])) and (src < 0).sum() >= 5
    assert M < 2 ** 21 + 2 ** 16
    return rows, offsets, i.astype(np.int32), src, eid


def test_in_edges(world):
    g = world["g"]
    for ballast_row in (g.B - 2, 0):                                   # a row close under the boundary, and the very first
        rows, *want = want_in_edges(g, ballast_row)
        got = world["graph"].in_edges(torch.from_numpy(rows).to(DEV), return_eids=True)
        torch.cuda.synchronize()
        same_arrays(got, want, f"ballast row {ballast_row}" + world["why"], names=("offsets", "dst", "src", "eid"))


def test_offsets_past_the_boundary(world):
    """Every row of the graph: the offsets are its row pointers, past the boundary.  A scan with 32-bit tile sums differs there."""
    g = world["g"]
    rows = np.arange(g.node_num, dtype=np.int32)
    want = ref.row_offsets(g.indptr, rows)
    assert np.array_equal(want, g.indptr) and want[-1] == g.E > g.boundary
    if g.boundary >= 2 ** 31:
        assert not np.array_equal(ref.row_offsets_int32_tiles(g.indptr, rows), want)
    got = world["graph"].row_offsets(torch.from_numpy(rows).to(DEV))
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want), "row_offsets over every row" + world["why"]
    if g.E > 2 ** 31 - 1:
        with pytest.raises(ValueError, match="2\\^31"):
            world["graph"].in_edges(torch.from_numpy(rows).to(DEV))
