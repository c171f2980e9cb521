"""GraphStorage.reverse / out_degrees / out_edges and the C ABI's legion_graph_build_reverse / legion_graph_reverse_csr on the GPU, bit
for bit against tests/reverse_ref.py: a graph whose reverse rows have 0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2T, 2T + 1, 3T + 5 and
5T - 1 entries (T = LG_REVERSE_TILE = 4 096: every class boundary of the sort, and merges of 2, 3, 4 and 5 runs with a short last run),
the symmetric graph of tests/node2vec_ref.py, one vertex without entries, a graph whose entries are all dead, the small graphs of
link_ref; two builds on two objects, a second reverse(), another stream, the reverse of the reverse, rows_sorted() on the reverse,
out_degrees and out_edges with seeds repeated, without entries, -1 and N, and every refusal of the C ABI.  What makes a wrong kernel
fail is asserted from the numpy reference alone before any launch; an input that fails a condition is replaced, never the condition."""
import ctypes

import numpy as np
import pytest
import torch

from tests import link_ref, node2vec_ref
from tests import reverse_ref as ref
from tests.compare import same_arrays

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMES = ("rindptr", "rcol", "reid")
FIGURES = {"classes": (40, 61819, 61759), "sym": (6000, 53448, 53418), "one-vertex": (1, 0, 0), "all-dead": (5, 300, 0)}      # N, E, E'


def all_dead():
    col = np.resize(np.array([-1, 5, -1, 6, 2 ** 31 - 1, -7], dtype=np.int32), 300)
    return np.array([0, 100, 100, 250, 300, 300], dtype=np.int64), col


def graphs():
    """name -> (indptr, col)."""
    g = {"classes": ref.class_graph(ref.class_lengths(), 7), "sym": node2vec_ref.sym_graph()[:2],
         "one-vertex": (np.zeros(2, dtype=np.int64), np.zeros(0, dtype=np.int32)), "all-dead": all_dead()}
    g.update(link_ref.small_graphs())
    g["complete"], g["ring"] = link_ref.complete_graph(), link_ref.ring_graph()
    return g


def conditions(name, indptr, col):
    """What the graph must hold for a wrong kernel to fail on it; returns the reference (rindptr, rcol, reid)."""
    want = ref.reverse(indptr, col)
    if name in FIGURES:
        assert (indptr.size - 1, col.size, want[2].size) == FIGURES[name], (name, indptr.size - 1, col.size, want[2].size)
    if name == "classes":
        lengths = np.diff(want[0])
        assert set(ref.CLASS_LENGTHS) <= set(lengths.tolist()), "every class boundary"
        assert ref.classes_of(want[0]) == ({"none", "wave", "tile", "long"}, [2, 3, 4, 5]), "every class, merges of 2 to 5 runs"
        assert sorted({ref.passes(int(x)) for x in lengths if x > ref.TILE}) == [1, 2, 3], "rows that start in either buffer"
        assert (col == -1).sum() >= 10 and (col >= indptr.size - 1).sum() >= 10, "dead entries and entries outside the graph"
        pairs = want[1].astype(np.int64) * indptr.size + np.repeat(np.arange(indptr.size - 1), lengths)
        assert np.unique(pairs).size < pairs.size, "parallel edges"
        unsorted, late = ref.rows_in_scatter_order(indptr, col), ref.merge_off_by_one(indptr, col)
        for u in range(lengths.size):                              # no sort: the rows of every class differ; a late run: every long row
            row = slice(int(want[0][u]), int(want[0][u + 1]))
            if lengths[u] <= 1 or lengths[u] >= 63:                # (a shuffle of a handful of entries may be the identity)
                assert np.array_equal(unsorted[2][row], want[2][row]) == (lengths[u] <= 1), u
            assert np.array_equal(late[2][row], want[2][row]) == (lengths[u] <= ref.TILE + 1), u
        assert not np.array_equal(ref.dead_kept(indptr, col)[0], want[0])
    if name == "sym":
        assert (col == -1).sum() == 30 and np.diff(want[0]).max() == 4083 and np.diff(want[0]).min() == 0
        assert not np.array_equal(ref.dead_kept(indptr, col)[0], want[0])
        assert not np.array_equal(ref.rows_in_scatter_order(indptr, col)[2], want[2])
    return want


def seeds_for(indptr, col, n):
    """n nodes: the longest and the empty reverse rows first, repeats, a -1 and an N."""
    N = indptr.size - 1
    lengths = np.diff(ref.reverse(indptr, col)[0])
    s = (np.arange(n, dtype=np.int64) * 2654435761 % max(N, 1)).astype(np.int32)
    head = np.concatenate([np.argsort(-lengths, kind="stable")[:3], np.nonzero(lengths == 0)[0][:2]]).astype(np.int32)[:n]
    s[:head.size] = head
    if n >= 4:
        s[n // 2] = s[0]
        s[n - 1], s[n - 2] = -1, N
    return s


def make(indptr, col):
    from legion_amd import engine
    d_col = torch.from_numpy(col).to(DEV) if col.size else torch.zeros(0, dtype=torch.int32, device=DEV)
    return engine.GraphStorage(1, torch.from_numpy(indptr).to(DEV), d_col)


def triple(rev):
    return [rev.indptr, rev.col, rev.eids]


@pytest.fixture(scope="module")
def world(hip):
    made = {}
    for name, (indptr, col) in graphs().items():
        want = conditions(name, indptr, col)
        made[name] = dict(indptr=indptr, col=col, want=want, graph=make(indptr, col))
    yield made
    torch.cuda.synchronize()
    for w in made.values():
        w["graph"].close()


def getter(L, handle):
    a, b, c = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    return int(L.legion_graph_reverse_csr(handle, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))), (a.value, b.value, c.value)


@pytest.mark.parametrize("name", sorted(graphs()))
def test_reverse_is_the_reference(world, hip, name):
    w = world[name]
    g = w["graph"]
    if getattr(g, "_reverse", None) is None:
        assert getter(hip, g.handle) == (-1, (None, None, None)), "the getter before a build"
    rev = g.reverse()
    same_arrays(triple(rev), w["want"], name, NAMES)
    live, ptrs = getter(hip, g.handle)
    assert live == w["want"][2].size and ptrs[0] and (live == 0 or (ptrs[1] and ptrs[2]))
    assert hip.legion_graph_reverse_csr(g.handle, None, None, None) == live, "any out-pointer may be null"
    assert rev.parent is g and g.reverse() is rev and rev.node_num == g.node_num and rev.edge_num == live
    assert hip.legion_graph_build_reverse(g.handle, None) == 0, "a second call returns 0 without work"
    assert getter(hip, g.handle) == (live, ptrs)
    same_arrays(triple(rev), w["want"], name + " after a second build", NAMES)


@pytest.mark.parametrize("name", ["classes", "sym"])
def test_two_builds_are_identical_and_another_stream_builds_the_same(world, name):
    w = world[name]
    first = [x.clone() for x in triple(w["graph"].reverse())]
    stream = torch.cuda.Stream(device=DEV)
    for s in (None, stream, stream):
        g = make(w["indptr"], w["col"])
        if s is not None:
            s.wait_stream(torch.cuda.current_stream())
        rev = g.reverse(stream=s)
        torch.cuda.synchronize()
        for a, b in zip(triple(rev), first):
            assert torch.equal(a, b)
        same_arrays(triple(rev), w["want"], f"{name} on {s}", NAMES)
        g.close()


@pytest.mark.parametrize("name", ["classes", "sym", "ring", "degrees-257"])
def test_rows_of_the_reverse_are_sorted(world, name):
    w = world[name]
    assert node2vec_ref.rows_sorted(w["want"][0], w["want"][1])
    assert w["graph"].reverse().rows_sorted() is True


@pytest.mark.parametrize("name", ["sym", "complete", "ring"])
def test_the_reverse_of_the_reverse_is_the_live_graph(world, name):
    indptr, col = ref.live_graph(world[name]["indptr"], world[name]["col"])
    assert node2vec_ref.rows_sorted(indptr, col) and np.all((col >= 0) & (col < indptr.size - 1)), "sorted rows, no dead entries"
    g = make(indptr, col)
    rev = g.reverse()
    back = rev.reverse()
    same_arrays([back.indptr, back.col], [indptr, col], name + ": the reverse of the reverse")
    same_arrays(rev.eids[back.eids], np.arange(col.size, dtype=np.int64), name + ": the edge ids composed")
    assert back.parent is rev and rev.parent is g
    torch.cuda.synchronize()
    g.close()


@pytest.mark.parametrize("name", ["classes", "sym", "all-dead", "one-vertex", "ends-empty"])
@pytest.mark.parametrize("n", [0, 1, 5, 257])
def test_out_degrees_and_out_edges(world, name, n):
    w = world[name]
    nodes = seeds_for(w["indptr"], w["col"], n)
    g = w["graph"]
    same_arrays(g.out_degrees(nodes), ref.out_degrees(w["indptr"], w["col"], nodes), f"{name} {n}: out_degrees")
    want = ref.out_edges(w["indptr"], w["col"], nodes)
    same_arrays(g.out_edges(nodes, return_eids=True), want, f"{name} {n}", ("src", "dst", "eid"))
    same_arrays(g.out_edges(torch.from_numpy(nodes).to(DEV)), want[:2], f"{name} {n} without eids", ("src", "dst"))
    if want[2].size:
        assert np.array_equal(w["col"][want[2]], nodes[want[0]]), "col[eid] is the node left"
        assert np.array_equal(link_ref.find_edges(w["indptr"], w["col"], want[2])[0], want[1]), "find_edges' row is dst"


def test_out_edges_on_another_stream(world):
    w = world["classes"]
    nodes = seeds_for(w["indptr"], w["col"], 65)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())
    got = w["graph"].out_edges(nodes, return_eids=True, stream=stream)
    deg = w["graph"].out_degrees(nodes, stream=stream)
    stream.synchronize()
    same_arrays(got, ref.out_edges(w["indptr"], w["col"], nodes), "stream", ("src", "dst", "eid"))
    same_arrays(deg, ref.out_degrees(w["indptr"], w["col"], nodes), "stream: out_degrees")


def test_the_c_abi_refuses(hip):
    from legion_amd import engine
    assert hip.legion_graph_build_reverse(None, None) == -1
    assert getter(hip, None) == (-1, (None, None, None))
    assert hip.legion_graph_reverse_csr(None, None, None, None) == -1
    N = ref.MAX_NODES + 1
    assert ref.refused(True, N) and not ref.refused(True, N - 1) and ref.refused(False, 5)
    big = engine.GraphStorage(1, torch.zeros(N + 1, dtype=torch.int64, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV))
    free = torch.cuda.mem_get_info()[0]
    assert hip.legion_graph_build_reverse(big.handle, None) == -1
    assert getter(hip, big.handle) == (-1, (None, None, None)), "nothing built"
    assert torch.cuda.mem_get_info()[0] >= free, "nothing allocated"
    with pytest.raises(ValueError, match="at most"):
        big.reverse()
    torch.cuda.synchronize()
    big.close()
