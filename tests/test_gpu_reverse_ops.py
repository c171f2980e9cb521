"""The existing ops on GraphStorage.reverse(): each equals its numpy reference run on the reversed arrays of tests/reverse_ref.py --
random_walk uniform and with the parent's weights carried over by rev.set_edge_weights(w[rev.eids]), node2vec_random_walk (the reverse's
rows are sorted), full_neighbor_block and sample_distinct.  On the symmetric graph of tests/node2vec_ref.py.  A walk on the reverse
follows the parent's edges backwards: its return_eids mapped through .eids name parent edges whose column entry is the vertex left and
whose row is the vertex reached."""
import numpy as np
import pytest
import torch

from tests import in_edges_ref, link_ref, node2vec_ref, topk_ref, walk_ref, weighted_ref
from tests import reverse_ref as ref
from tests.compare import same_arrays

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = node2vec_ref.NODE_NUM


@pytest.fixture(scope="module")
def world(hip):
    from legion_amd import engine
    indptr, col, w = node2vec_ref.sym_graph()
    rindptr, rcol, reid = ref.reverse(indptr, col)
    rw = w[reid]
    assert (rw > 0).sum() > 10000 and (rw == 0).sum() > 1000, "weights and zero weights travel"
    assert node2vec_ref.rows_sorted(rindptr, rcol)
    graph = engine.GraphStorage(1, torch.from_numpy(indptr).to(DEV), torch.from_numpy(col).to(DEV))
    rev = graph.reverse()
    rev.set_edge_weights(torch.from_numpy(w).to(DEV)[rev.eids])     # the documented line
    torch.cuda.synchronize()
    yield dict(graph=graph, rev=rev, indptr=indptr, col=col, w=w, rindptr=rindptr, rcol=rcol, reid=reid, rw=rw,
               table=weighted_ref.cdf(rindptr, rw))
    torch.cuda.synchronize()
    graph.close()


@pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "weighted"])
def test_random_walk_on_the_reverse(world, weighted):
    seeds = node2vec_ref.seeds_for(1000)
    want = walk_ref.walk(world["rindptr"], world["rcol"], seeds, 9, table=world["table"] if weighted else None, base=3)
    got = world["rev"].random_walk(seeds, 9, weighted=weighted, return_eids=True, base=3)
    same_arrays(got, want, f"walk weighted {weighted}", ("traces", "eids"))
    traces, steps = want
    took = steps >= 0
    assert took.sum() > 3000
    parent = world["reid"][steps[took]]                            # the parent's edges the walk went along, backwards
    left, reached = traces[:, :-1][took], traces[:, 1:][took]
    assert np.array_equal(world["col"][parent], left), "the parent edge's column entry is the vertex left"
    assert np.array_equal(link_ref.find_edges(world["indptr"], world["col"], parent)[0], reached), "and its row the vertex reached"
    mapped = world["rev"].eids[got[1].clamp(min=0)].cpu().numpy()[took]
    assert np.array_equal(mapped, parent)


@pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "weighted"])
def test_node2vec_on_the_reverse(world, weighted):
    seeds = node2vec_ref.seeds_for(700)
    want = node2vec_ref.walk(world["rindptr"], world["rcol"], seeds, 8, 0.5, 2.0, table=world["table"] if weighted else None, base=11)
    rev = world["rev"]
    assert rev.rows_sorted() is True
    got = rev.node2vec_random_walk(seeds, 0.5, 2.0, 8, weighted=weighted, return_eids=True, base=11)
    same_arrays(got, want, f"node2vec weighted {weighted}", ("traces", "eids"))


def test_full_neighbor_block_on_the_reverse(world):
    seeds = np.array([6, 0, 1, 2, 3, 4, 5, 7, 100, 5999, 1234, 10], dtype=np.int32)
    b = in_edges_ref.full_neighbor_block(world["rindptr"], world["rcol"], seeds)
    got = world["rev"].full_neighbor_block(seeds, return_eids=True)
    same_arrays(got, [b["input_nodes"], b["dst_local"], b["src_local"], b["offsets"], b["eids"]], "block",
                ("input_nodes", "dst_local", "src_local", "offsets", "eids"))
    assert b["eids"].size > 4000 and np.array_equal(world["col"][world["reid"][b["eids"]]], seeds[b["dst_local"]])


@pytest.mark.parametrize("weights", [False, True], ids=["uniform", "weighted"])
def test_sample_distinct_on_the_reverse(world, weights):
    rows = node2vec_ref.seeds_for(300)
    rw = world["rw"] if weights else None
    want = topk_ref.row_topk(world["rindptr"], world["rcol"], rw, rows, 10, topk_ref.SAMPLE, 5)
    got = world["rev"].sample_distinct(rows, 10, weights=rw, salt=5, return_eids=True)
    same_arrays(got, [want[0], want[2], want[1]], f"sample_distinct weights {weights}", ("src", "counts", "eids"))
    assert (want[2] == 10).sum() > 50 and (want[2] < 10).sum() > 5
