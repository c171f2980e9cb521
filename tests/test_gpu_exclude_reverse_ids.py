"""GraphStorage.reverse_edge_ids and the C ABI's legion_reverse_edge_ids on the GPU, bit for bit against tests/exclude_ref.py: every
edge id of the symmetric graph of tests/node2vec_ref.py plus -1, E and E + 5 through both search paths (via 0: the graph's sorted rows;
via 1: the reverse CSR), which must agree; an unsorted directed graph (reverse_ref.class_graph) through the reverse CSR, where the
graph's own rows are refused; n at 0, 1 and either side of a quarter tile and of a tile; one n past the capped grid; the refusals; another
stream.  What makes a wrong kernel fail is asserted from the numpy reference alone before any launch; an input that fails a condition
is replaced, never the condition."""
import numpy as np
import pytest
import torch

from tests import exclude_ref as ref
from tests import node2vec_ref, reverse_ref
from tests.compare import same_arrays

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = [0, 1, 255, 256, 257, 1023, 1024, 1025]
STRIDE_N = ref.IDS_STRIDE + 1025                                   # 2 048 workgroups x 1 024 ids, + 1 025
SYM_FIGURES = dict(entries=53448, live=53418, no_reverse=29, loops=856, loops_fixed=856, not_involution=603, longest=4097)


def sym():
    return node2vec_ref.sym_graph()[:2]


def directed():
    """An unsorted directed graph: forty vertices, parallel edges, dead entries and entries outside the graph."""
    return reverse_ref.class_graph(reverse_ref.class_lengths(), 7)


def all_ids(col):
    E = col.size
    return np.concatenate([np.arange(E, dtype=np.int64), [-1, E, E + 5]])


def ids_for(indptr, col, n):
    """n edge ids: -1, E and E + 5, dead entries, entries without a reverse, parallel edges and self-loops first, then a spread."""
    E = col.size
    rev = ref.reverse_edge_ids(indptr, col, np.arange(E))
    back = ref.reverse_edge_ids(indptr, col, rev)
    special = [np.array([E - 1, -1, E, E + 5]), np.nonzero(col < 0)[0][:3], np.nonzero((rev < 0) & (col >= 0))[0][:3],
               np.nonzero((rev >= 0) & (back != np.arange(E)))[0][:5], np.nonzero(rev == np.arange(E))[0][:3]]
    rest = np.arange(max(n, 1), dtype=np.int64) * 2654435761 % E
    return np.concatenate(special + [rest]).astype(np.int64)[:n]


def sym_conditions(indptr, col):
    """The figures of the symmetric graph, and that each model of a wrong kernel differs on all its ids.  Returns the reference."""
    assert ref.figures(indptr, col) == SYM_FIGURES and node2vec_ref.rows_sorted(indptr, col)
    ids = all_ids(col)
    want = ref.reverse_edge_ids(indptr, col, ids)
    assert (want[-3:] == -1).all() and (want[:-3][col < 0] == -1).all()
    first = ref.reverse_first_probed(indptr, col, ids)
    assert (first != want).sum() >= 100, "the first probed match is not the least e' over parallel edges"
    return ids, want                                               # (a dead entry given a reverse: the directed graph's to catch)


def directed_conditions(indptr, col):
    assert not node2vec_ref.rows_sorted(indptr, col)
    N = indptr.size - 1
    ids = all_ids(col)
    want = ref.reverse_edge_ids(indptr, col, ids)
    live = reverse_ref.live_entries(indptr, col)
    none = (want[live] < 0).sum()
    assert 0.3 * live.size < none < 0.9 * live.size, "many live edges without a reverse, and many with one"
    assert (col == -1).sum() >= 10 and (col >= N).sum() >= 10
    assert (ref.reverse_dead_given(indptr, col, ids) != want).sum() >= 5, "a dead or out-of-graph entry given a reverse differs"
    return ids, want


def stride_case():
    """(ids, want) over the symmetric graph past the capped grid: the ids of the second trip differ from those a stride before them."""
    indptr, col = sym()
    ids = np.arange(STRIDE_N, dtype=np.int64) * 40503 % col.size
    ids[:4] = [-1, col.size, col.size + 5, col.size - 1]
    want = ref.reverse_edge_ids(indptr, col, ids)
    stale = ref.stale_second_trip(want, ref.IDS_STRIDE)
    assert (stale[ref.IDS_STRIDE:] != want[ref.IDS_STRIDE:]).sum() >= 500, "a stale second trip differs"
    return ids, want


def make(indptr, col):
    from legion_amd import engine
    return engine.GraphStorage(1, torch.from_numpy(indptr).to(DEV), torch.from_numpy(col).to(DEV))


def call(L, graph, ids, via, stream=None):
    """legion_reverse_edge_ids through the C ABI: (rc, out)."""
    d_ids = torch.from_numpy(np.asarray(ids, dtype=np.int64)).to(DEV)
    out = torch.full((max(len(ids), 1),), -7, dtype=torch.int64, device=DEV)
    s = stream if stream is not None else torch.cuda.current_stream()
    rc = L.legion_reverse_edge_ids(s.cuda_stream, graph.handle, d_ids.data_ptr(), len(ids), via, out.data_ptr())
    torch.cuda.synchronize()
    return rc, out[:len(ids)]


@pytest.fixture(scope="module")
def world(hip):
    made = {}
    for name, build, cond in (("sym", sym, sym_conditions), ("directed", directed, directed_conditions)):
        indptr, col = build()
        ids, want = cond(indptr, col)
        made[name] = dict(indptr=indptr, col=col, ids=ids, want=want, graph=make(indptr, col))
    yield made
    torch.cuda.synchronize()
    for w in made.values():
        w["graph"].close()


def test_an_unsorted_graph_is_refused_before_its_reverse_is_built(world, hip):
    """On a graph object of its own: no check of its rows yet, no reverse."""
    w = world["directed"]
    g = make(w["indptr"], w["col"])
    ids = w["ids"][:300]
    for via in (0, 1):                                             # rows never checked, no reverse
        rc, out = call(hip, g, ids, via)
        assert rc == -1 and (out == -7).all(), via
    assert g.rows_sorted() is False
    rc, out = call(hip, g, ids, 0)
    assert rc == -1 and (out == -7).all(), "rows found unsorted"
    rc, out = call(hip, g, ids, 1)
    assert rc == -1 and (out == -7).all(), "still no reverse"
    assert ref.reverse_refused(300, 0, 0, False) and ref.reverse_refused(300, 1, 0, False) and not ref.reverse_refused(300, 1, 0, True)
    g.close()


def test_every_edge_of_the_symmetric_graph_by_both_paths(world, hip):
    w = world["sym"]
    g = make(w["indptr"], w["col"])                                # (an object of its own: no reverse yet)
    assert g.rows_sorted() is True
    same_arrays(g.reverse_edge_ids(w["ids"]), w["want"], "sym, the Python op")
    assert getattr(g, "_reverse", None) is None, "sorted rows: the Python op searches the graph itself"
    rc, via0 = call(hip, g, w["ids"], 0)
    assert rc == 0
    same_arrays(via0, w["want"], "sym via 0")
    rc, out = call(hip, g, w["ids"], 1)
    assert rc == -1 and (out == -7).all(), "via 1 before the reverse is built"
    g.reverse()
    rc, via1 = call(hip, g, w["ids"], 1)
    assert rc == 0
    same_arrays(via1, w["want"], "sym via 1")
    assert torch.equal(via0, via1)
    same_arrays(call(hip, g, w["ids"], 0)[1], w["want"], "sym via 0 again: bit-identical from run to run")
    g.close()


def test_an_unsorted_graph_through_the_reverse_csr(world, hip):
    w = world["directed"]
    g = w["graph"]
    same_arrays(g.reverse_edge_ids(w["ids"]), w["want"], "directed, the Python op (builds the reverse)")
    rc, out = call(hip, g, w["ids"], 1)
    assert rc == 0
    same_arrays(out, w["want"], "directed via 1")
    rc, out = call(hip, g, w["ids"], 0)
    assert rc == -1 and (out == -7).all(), "via 0 on unsorted rows stays refused"


@pytest.mark.parametrize("n", SIZES)
def test_sizes_either_side_of_a_tile(world, hip, n):
    for name in ("sym", "directed"):
        w = world[name]
        ids = ids_for(w["indptr"], w["col"], n)
        assert ids.size == n
        want = ref.reverse_edge_ids(w["indptr"], w["col"], ids)
        if n >= 255:
            assert (want < 0).sum() >= 5 and (want >= 0).sum() >= 20, "answers of both kinds"
        same_arrays(w["graph"].reverse_edge_ids(ids), want, f"{name} n {n}")


def test_past_the_grid_cap(world, hip):
    ids, want = stride_case()
    g = world["sym"]["graph"]
    assert g.rows_sorted() is True
    g.reverse()
    for via in (0, 1):
        rc, out = call(hip, g, ids, via)
        assert rc == 0
        same_arrays(out, want, f"{STRIDE_N} ids via {via}")


def test_refusals(world, hip):
    g = world["sym"]["graph"]
    assert g.rows_sorted() is True
    g.reverse()
    ids = torch.zeros(8, dtype=torch.int64, device=DEV)
    out = torch.full((8,), -7, dtype=torch.int64, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    L = hip
    assert L.legion_reverse_edge_ids(s, None, ids.data_ptr(), 8, 0, out.data_ptr()) == -1
    assert L.legion_reverse_edge_ids(s, g.handle, None, 8, 0, out.data_ptr()) == -1
    assert L.legion_reverse_edge_ids(s, g.handle, ids.data_ptr(), 8, 0, None) == -1
    for n, via in ((-1, 0), (2 ** 31, 0), (8, 2), (8, -1), (-1, 1), (2 ** 31, 1)):
        assert L.legion_reverse_edge_ids(s, g.handle, ids.data_ptr(), n, via, out.data_ptr()) == -1, (n, via)
        assert ref.reverse_refused(n, via, 1, True)
    assert L.legion_reverse_edge_ids(s, g.handle, ids.data_ptr(), 0, 0, out.data_ptr()) == 0
    torch.cuda.synchronize()
    assert (out == -7).all(), "a refused call and n == 0 touch no buffer"


def test_on_another_stream(world, hip):
    w = world["sym"]
    side = torch.cuda.Stream()
    ids = w["ids"][:5000]
    got = w["graph"].reverse_edge_ids(ids, stream=side)
    side.synchronize()
    same_arrays(got, w["want"][:5000], "another stream")
