"""Seed-edge exclusion on a graph whose live rows sit at edge offsets of 5 000, 2^31 and 2^32 (tests/far_rows.py's layout), bit for bit
against tests/exclude_ref.py on the layout's reference view.  The device world is this file's own, as the reverse CSR's far-row test
has one: the ballast entries are -1, dead, so that the rows stay sorted and the reverse holds the live tail only.  Every live edge id,
ballast ids, -1, E and E + 5 go through both search paths; input ids and answers lie on both sides of the boundary, the straddling hub's
entries among them.  A set built from those ids answers for ids that differ from members only above bit 31, and the filter drops them
from a list of the same ids."""
import numpy as np
import pytest
import torch

from tests import exclude_ref as ref
from tests import far_rows
from tests.compare import same_arrays

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LIVE_FIGURES = dict(entries=10065, live=10059, no_reverse=6, loops=141, loops_fixed=141, not_involution=110, longest=513)


def want_reverse_ids(g):
    """(true ids, want) from the view, and the conditions of the boundary."""
    view = np.arange(g.live_E, dtype=np.int64)
    want = ref.reverse_edge_ids(g.indptr_ref, g.col_ref, view)
    want = np.where(want >= 0, want + g.offset, -1)
    ids = np.concatenate([view + g.offset, [0, g.offset - 1, g.offset // 2, -1, g.E, g.E + 5]])
    want = np.concatenate([want, np.full(6, -1, dtype=np.int64)])  # a ballast entry is dead
    have = want >= 0
    for name, x in (("input ids", ids[have]), ("answers", want[have])):
        assert (x < g.boundary).sum() >= 100 and (x >= g.boundary).sum() >= 100, f"{name} on both sides of the boundary"
    crossing = have & ((ids < g.boundary) != (want < g.boundary))
    assert crossing.sum() >= 100, "edges whose reverse lies on the other side"
    hub = have & (g.indptr[g.hub] <= ids) & (ids < g.indptr[g.hub + 1])
    assert (hub & (ids < g.boundary)).sum() >= 10 and (hub & (ids >= g.boundary)).sum() >= 10, "the straddling hub's entries, both sides"
    into = have & (g.indptr[g.hub] <= want) & (want < g.indptr[g.hub + 1])
    assert (into & (want < g.boundary)).sum() >= 10 and (into & (want >= g.boundary)).sum() >= 10, "answers inside the straddling row"
    wrong = np.where(want >= 0, ((want + 2 ** 31) % 2 ** 32) - 2 ** 31, -1)
    assert np.array_equal(wrong, want) == (g.boundary < 2 ** 31), "an answer formed in 32 bits differs from 2^31 on"
    return ids, want


def set_case(g, ids, want):
    """(members, queries, want): the set of the answers; queries that differ from members only above bit 31."""
    members = want[::3].copy()
    live = members[members >= 0]
    queries = np.concatenate([ids, live ^ (1 << 32), live ^ (1 << 31), live + (1 << 33), [-1, -5]])
    answer = ref.contains(members, queries)
    assert answer.sum() >= 1000 and (answer == 0).sum() >= 1000
    assert (ref.contains_key32(members, queries) != answer).sum() >= 1000, "a key cut to 32 bits differs"
    return members, queries, answer


@pytest.mark.parametrize("boundary", ["5000", "2^31", "2^32"])
def test_exclusion_at_a_far_boundary(hip, boundary):
    from legion_amd import engine
    g = far_rows.layout(boundary)
    ids, want = want_reverse_ids(g)
    members, queries, answer = set_case(g, ids, want)
    torch.cuda.synchronize()
    col = torch.full((g.E,), -1, dtype=torch.int32, device=DEV)
    col[g.offset:] = torch.from_numpy(g.col_ref.copy()).to(DEV)
    indptr = torch.from_numpy(g.indptr.copy()).to(DEV)
    graph = engine.GraphStorage(1, indptr, col)
    why = " -- " + far_rows.WHY[boundary]
    try:
        d_ids = torch.from_numpy(ids).to(DEV)
        out = torch.full((ids.size,), -7, dtype=torch.int64, device=DEV)
        s = torch.cuda.current_stream().cuda_stream
        assert graph.rows_sorted() is True
        same_arrays(graph.reverse_edge_ids(d_ids), want, boundary + " the Python op" + why)
        assert hip.legion_reverse_edge_ids(s, graph.handle, d_ids.data_ptr(), ids.size, 0, out.data_ptr()) == 0
        same_arrays(out, want, boundary + " via 0" + why)
        out.fill_(-7)
        graph.reverse()
        assert hip.legion_reverse_edge_ids(s, graph.handle, d_ids.data_ptr(), ids.size, 1, out.data_ptr()) == 0
        same_arrays(out, want, boundary + " via 1" + why)
        excl = engine.EdgeIdSet(members)
        same_arrays(excl.contains(queries), answer, boundary + " contains" + why)
        dst = (np.arange(ids.size) // 9).astype(np.int32)
        src = np.arange(ids.size, dtype=np.int32)
        got = engine.exclude_edges(dst, src, ids, excl)
        same_arrays(got, ref.exclude_edges(dst, src, ids, members)[:3], boundary + " exclude_edges" + why, ("dst", "src", "eid"))
        if boundary == "5000":
            whole = np.concatenate([np.full(g.offset, -1, np.int32), g.col_ref])
            same_arrays(graph.reverse_edge_ids(ids), ref.reverse_edge_ids(g.indptr, whole, ids), "the whole graph on the host")
    finally:
        torch.cuda.synchronize()
        graph.close()
        del graph, col, indptr
        torch.cuda.empty_cache()
