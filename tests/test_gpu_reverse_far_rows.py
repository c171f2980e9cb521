"""The reverse CSR of a graph whose live rows sit at edge offsets of 5 000, 2^31 and 2^32 (tests/far_rows.py's layout), bit for bit
against tests/reverse_ref.py on the layout's reference view.  The device world is this file's own: the ballast entries are -1, dead, not
far_rows.device_world's zeros, which would make vertex 0 a reverse hub of 2^32 entries.  So the build counts and scatters every tile of
the ballast and drops it: E' is the live tail's live entries, every edge id of the reverse is a true one -- a view's edge id plus the
ballast -- with values on both sides of the boundary, and the entries of the straddling hub's row lie on both.  At 5 000 the whole
graph is also materialised on the host and reversed there."""
import numpy as np
import pytest
import torch

from tests import far_rows
from tests import reverse_ref as ref
from tests.compare import same_arrays

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMES = ("rindptr", "rcol", "reid")


def want_reverse(g):
    """The reference from the view, its edge ids made true ones, and the conditions of the boundary."""
    rindptr, rcol, reid = ref.reverse(g.indptr_ref, g.col_ref)
    reid = reid + g.offset
    live = int(((g.col_ref >= 0) & (g.col_ref < g.node_num)).sum())
    assert reid.size == live and live == g.live_E - int((g.col_ref < 0).sum()) and (g.col_ref < 0).sum() >= 3, "the ballast and the dead are dropped"
    assert np.all(rindptr[:g.B + 1] == 0), "nothing points at a ballast vertex"
    low, high = reid < g.boundary, reid >= g.boundary
    assert low.sum() >= 100 and high.sum() >= 100, "edge ids on both sides of the boundary"
    hub = rcol == g.hub                                            # the entries of the straddling hub's row
    assert (hub & low).sum() >= 10 and (hub & high).sum() >= 10, "the straddling row's entries lie on both sides"
    assert np.all(g.indptr[rcol] <= reid) and np.all(reid < g.indptr[rcol.astype(np.int64) + 1])
    wrong = ref.e32(rindptr, rcol, reid)[2]
    assert np.array_equal(wrong, reid) == (g.boundary < 2 ** 31), "e in 32 bits differs from 2^31 on"
    return rindptr, rcol, reid


@pytest.mark.parametrize("boundary", ["5000", "2^31", "2^32"])
def test_reverse_at_a_far_boundary(hip, boundary):
    from legion_amd import engine
    g = far_rows.layout(boundary)
    want = want_reverse(g)
    torch.cuda.synchronize()
    col = torch.full((g.E,), -1, dtype=torch.int32, device=DEV)
    col[g.offset:] = torch.from_numpy(g.col_ref.copy()).to(DEV)
    indptr = torch.from_numpy(g.indptr.copy()).to(DEV)
    graph = engine.GraphStorage(1, indptr, col)
    why = " -- " + far_rows.WHY[boundary]
    try:
        rev = graph.reverse()
        same_arrays([rev.indptr, rev.col, rev.eids], want, boundary + why, NAMES)
        nodes = np.concatenate([g.seeds(64), [0, g.B - 1]]).astype(np.int32)
        src, dst, eid = ref.out_edges(g.indptr_ref, g.col_ref, nodes)
        same_arrays(graph.out_edges(nodes, return_eids=True), (src, dst, eid + g.offset), boundary + " out_edges" + why, ("src", "dst", "eid"))
        same_arrays(graph.out_degrees(nodes), ref.out_degrees(g.indptr_ref, g.col_ref, nodes), boundary + " out_degrees" + why)
        if boundary == "5000":
            whole = np.concatenate([np.full(g.offset, -1, np.int32), g.col_ref])
            same_arrays([rev.indptr, rev.col, rev.eids], ref.reverse(g.indptr, whole), "the whole graph on the host", NAMES)
    finally:
        torch.cuda.synchronize()
        graph.close()
        del graph, col, indptr
        torch.cuda.empty_cache()
