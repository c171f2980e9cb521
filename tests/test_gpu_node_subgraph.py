"""GraphStorage.node_subgraph on the GPU, bit for bit against tests/induced_ref.py: the first four rows of the table of
tests/test_gpu_induced.py (every third vertex, every vertex, the hub's neighbourhood, a shuffled half) on the symmetric graph of
tests/node2vec_ref.py, the ring and the complete graph; the ValueErrors for a repeat, -1 and node_num.  Then the use end to end, as
ClusterGCN and ShaDow-GNN make it: for ascending nodes GraphStorage(1, indptr_sub, col_sub) has sorted rows, its random walks are
tests/walk_ref.py's on the reference's subgraph arrays, its in_edges return col_sub back, and one mean aggregation over the subgraph in
torch equals the dense numpy result to the bit on small-integer features."""
import numpy as np
import pytest
import torch

from tests import induced_ref as ref
from tests import link_ref, node2vec_ref, walk_ref
from tests.compare import same_arrays
from tests.test_gpu_induced import table

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SUB = ("indptr_sub", "col_sub", "eids")
TABLE_ROWS = ("third", "identity", "hubs", "shuffled")
ASCENDING = ("third", "identity", "hubs")


def graphs():
    """name -> (indptr, col, nodes)."""
    indptr, col, _ = node2vec_ref.sym_graph()
    t = table(indptr, col)
    out = {name: (indptr, col, t[name][1]) for name in TABLE_ROWS}
    out["ring"] = link_ref.ring_graph(8) + (np.array([0, 1, 2, 4, 5, 7], dtype=np.int32),)
    out["complete"] = link_ref.complete_graph(8) + (np.array([6, 1, 3, 0], dtype=np.int32),)
    return out


def conditions(name, indptr, col, nodes):
    """The reference's subgraph, and what the case is there for."""
    indptr_sub, col_sub, eids = ref.node_subgraph(indptr, col, nodes)
    k = nodes.size
    assert indptr_sub.shape == (k + 1,) and indptr_sub[0] == 0 and indptr_sub[-1] == col_sub.size == eids.size
    assert col_sub.size == 0 or (col_sub.min() >= 0 and col_sub.max() < k)
    assert np.array_equal(nodes[col_sub], col[eids]), "nodes[col_sub] is the original source"
    rows = np.repeat(np.arange(k), np.diff(indptr_sub))
    assert np.all(indptr[nodes[rows]] <= eids) and np.all(eids < indptr[nodes[rows] + 1]), "an entry of row j comes from the row of nodes[j]"
    if name in TABLE_ROWS:
        assert col_sub.size == table(indptr, col)[name][3]
    if name in ASCENDING:
        assert np.all(np.diff(nodes) > 0) and node2vec_ref.rows_sorted(indptr_sub, col_sub), "a monotone map keeps sorted rows sorted"
    if name == "ring":
        assert np.diff(indptr_sub).tolist() == [2, 2, 1, 1, 1, 1], "0 - 1 - 2, 4 - 5, and 7 - 0"
    if name == "complete":
        assert np.all(np.diff(indptr_sub) == k - 1), "K_4"
    return indptr_sub, col_sub, eids


def test_the_inputs_hold_their_conditions_before_any_launch():
    for name, (indptr, col, nodes) in graphs().items():
        conditions(name, indptr, col, nodes)


_GRAPHS = {}


def graphs_once():
    if not _GRAPHS:
        _GRAPHS.update(graphs())
    return _GRAPHS


@pytest.fixture(scope="module")
def cases(hip):
    """name -> (graph on the device, indptr, col, nodes): the symmetric graph once for its four cases."""
    from legion_amd import engine
    held, out = {}, {}
    for name, (indptr, col, nodes) in graphs_once().items():
        key = (indptr.size, col.size)
        if key not in held:
            held[key] = engine.GraphStorage(1, torch.from_numpy(indptr).to(DEV), torch.from_numpy(col).to(DEV))
        out[name] = (held[key], indptr, col, nodes)
    yield out
    torch.cuda.synchronize()
    for g in held.values():
        g.close()


@pytest.mark.parametrize("name", TABLE_ROWS + ("ring", "complete"))
def test_node_subgraph_is_the_reference(cases, name):
    from legion_amd import engine
    g, indptr, col, nodes = cases[name]
    want = conditions(name, indptr, col, nodes)
    got = g.node_subgraph(nodes, return_eids=True)
    torch.cuda.synchronize()
    assert len(got) == 3 and all(x.is_cuda for x in got)
    same_arrays(list(got), list(want), name, names=SUB)
    got = g.node_subgraph(engine.NodeSet(torch.from_numpy(nodes).to(DEV)))           # a NodeSet, no edge ids
    torch.cuda.synchronize()
    assert len(got) == 2
    same_arrays(list(got), list(want[:2]), name + ", a NodeSet", names=SUB)


def test_the_empty_subgraph_and_one_without_edges(cases):
    g, indptr, col, _ = cases["third"]
    got = g.node_subgraph(np.zeros(0, np.int32), return_eids=True)
    torch.cuda.synchronize()
    same_arrays(list(got), [np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int64)], "no nodes", names=SUB)
    lonely = np.array([7, 40, 41, 3000], dtype=np.int32)                             # rows without entries, and nothing points at them
    want = ref.node_subgraph(indptr, col, lonely)
    assert want[1].size == 0
    got = g.node_subgraph(lonely, return_eids=True)
    torch.cuda.synchronize()
    same_arrays(list(got), list(want), "no edges", names=SUB)


def test_nodes_that_are_no_distinct_vertices_are_value_errors(cases):
    g, indptr, col, _ = cases["third"]
    N = indptr.size - 1
    for bad in ([5, 9, 5], [3, -1, 4], [3, N, 4], [N + 100], [0, 0]):
        with pytest.raises(ValueError, match="distinct vertices of the graph"):
            g.node_subgraph(np.array(bad, dtype=np.int32))
    g.node_subgraph(np.array([N - 1, 0], dtype=np.int32))


@pytest.mark.parametrize("name", ASCENDING)
def test_the_subgraph_is_a_graph_this_library_samples_and_walks(cases, name):
    from legion_amd import engine
    g, indptr, col, nodes = cases[name]
    indptr_sub, col_sub, eids = conditions(name, indptr, col, nodes)
    k = nodes.size
    got = g.node_subgraph(nodes)
    g2 = engine.GraphStorage(1, got[0], got[1])
    try:
        assert g2.rows_sorted() is True
        # the walks of the subgraph are the reference's walks on the reference's arrays
        seeds = (np.arange(300, dtype=np.int64) * 2654435761 % k).astype(np.int32)
        seeds[:3] = [0, k - 1, -1]
        traces, walked = g2.random_walk(seeds, 9, return_eids=True)
        want_traces, want_eids = walk_ref.walk(indptr_sub, col_sub, seeds, 9)
        torch.cuda.synchronize()
        same_arrays([traces, walked], [want_traces, want_eids], name + ": walks", names=("traces", "eids"))
        assert (want_traces[:, -1] >= 0).sum() >= 100, "most walks run their whole length"
        # in_edges of every row gives col_sub back
        offsets, dst, src = g2.in_edges(np.arange(k, dtype=np.int32))
        torch.cuda.synchronize()
        same_arrays([offsets, src], [indptr_sub, col_sub], name + ": in_edges", names=("offsets", "src"))
        # one mean aggregation over the subgraph: small integers, exact in float32
        x = ((np.arange(k * 4, dtype=np.int64) * 7 % 13) - 6).astype(np.float32).reshape(k, 4)
        dense = np.zeros((k, k), dtype=np.float32)
        np.add.at(dense, (np.repeat(np.arange(k), np.diff(indptr_sub)), col_sub), 1.0)
        deg = np.maximum(np.diff(indptr_sub), 1).astype(np.float32)
        want = (dense @ x) / deg[:, None]
        assert np.abs(dense @ x).max() < 2 ** 24, "every sum is exact in float32, in any order"
        dx = torch.from_numpy(x).to(DEV)
        agg = torch.zeros((k, 4), dtype=torch.float32, device=DEV).index_add_(0, dst.long(), dx[src.long()])
        d_deg = (offsets[1:] - offsets[:-1]).clamp(min=1).to(torch.float32)
        same_arrays(agg / d_deg[:, None], want.astype(np.float32), name + ": mean aggregation")
    finally:
        torch.cuda.synchronize()
        g2.close()
