"""GraphStorage.full_neighbor_block on the GPU (DGL's MultiLayerFullNeighborSampler(1)): against tests/in_edges_ref.py -- the seeds first
and in order, input_nodes[src_local] the sources, dst_local the position of the seed -- both ValueErrors, a mean aggregation over the block
in torch against the dense numpy result, and input_nodes handed on to FeatureStorage.set_ids: a batch's sampled_ids start with them in
order, so the block's local indices address the batch's rows."""
import numpy as np
import pytest
import torch

from tests import edge_ids_ref
from tests import in_edges_ref as ref
from tests import link_ref, node2vec_ref
from tests.gpu_harness import GpuSide
from tests.helpers import Workload, compare_batches

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def graphs():
    """name -> (indptr, col, distinct seeds)."""
    indptr, col, _ = node2vec_ref.sym_graph()
    third = np.arange(0, node2vec_ref.NODE_NUM, 3, dtype=np.int32)
    third = np.concatenate([third[1000:], third[:1000]])           # not in ascending order: the hub (6) is the 1 003rd seed
    ring, complete = link_ref.ring_graph(8), link_ref.complete_graph(8)
    return {"sym-every-third": (indptr, col, third), "ring": ring + (np.array([5, 0, 3], dtype=np.int32),),
            "complete": complete + (np.arange(8, dtype=np.int32)[::-1].copy(),)}


def block_conditions(indptr, col, seeds):
    b = ref.full_neighbor_block(indptr, col, seeds)
    n, nodes = seeds.size, b["input_nodes"]
    assert np.array_equal(nodes[:n], seeds) and np.unique(nodes).size == nodes.size and nodes.min() >= 0
    live = b["src"] >= 0
    assert np.array_equal(nodes[b["src_local"][live]], b["src"][live]) and np.all(b["src_local"][~live] == -1)
    assert np.array_equal(b["dst_local"], b["dst"]) and np.array_equal(seeds[b["dst"]], np.repeat(seeds, np.diff(b["offsets"])))
    return b


@pytest.fixture(scope="module")
def world(hip):
    from legion_amd import engine
    made = {}
    for name, (indptr, col, seeds) in graphs().items():
        made[name] = dict(indptr=indptr, col=col, seeds=seeds, want=block_conditions(indptr, col, seeds),
                          graph=engine.GraphStorage(1, torch.from_numpy(indptr).to(DEV), torch.from_numpy(col).to(DEV)))
    yield made
    torch.cuda.synchronize()
    for c in made.values():
        c["graph"].close()


def test_the_inputs_hold_their_conditions_before_any_launch(world):
    c = world["sym-every-third"]
    b = c["want"]
    assert c["seeds"].size == 2000 and 6 in c["seeds"] and (b["src"] < 0).sum() >= 3 and b["input_nodes"].size > 4000
    assert (np.diff(b["offsets"]) == 0).sum() >= 1, "a seed without entries"
    assert (b["src_local"][b["src"] >= 0] < 2000).sum() >= 100, "sources that are seeds themselves"


@pytest.mark.parametrize("eids", [False, True], ids=["no-eids", "eids"])
@pytest.mark.parametrize("name", sorted(graphs()))
def test_the_block_is_the_reference(world, name, eids):
    c = world[name]
    got = c["graph"].full_neighbor_block(torch.from_numpy(c["seeds"]).to(DEV), return_eids=eids)
    torch.cuda.synchronize()
    assert len(got) == (5 if eids else 4)
    for key, x in zip(("input_nodes", "dst_local", "src_local", "offsets", "eids"), got):
        x, w = x.cpu().numpy(), c["want"][key]
        assert x.dtype == w.dtype and np.array_equal(x, w), f"{name}: {key}"


def test_both_value_errors(world, hip):
    from legion_amd import engine
    g = world["sym-every-third"]["graph"]
    N = node2vec_ref.NODE_NUM
    for seeds in ([5, 9, 5], [5, -1, 9], [5, N, 9], [N + 3]):
        with pytest.raises(ValueError, match="distinct vertices"):
            g.full_neighbor_block(np.array(seeds, dtype=np.int32))
    g.full_neighbor_block(np.array([5, 9], dtype=np.int32))
    # one row of 2^20 entries: with its seed one id more than unique_ids takes
    big = 2 ** 20
    indptr = np.array([0, big, big + 2, big + 2], dtype=np.int64)
    col = torch.zeros(big + 2, dtype=torch.int32, device=DEV)
    wide = engine.GraphStorage(1, torch.from_numpy(indptr).to(DEV), col)
    try:
        assert 1 + big > engine.UNIQUE_MAX_IDS
        with pytest.raises(ValueError, match="at most"):
            wide.full_neighbor_block(np.array([0], dtype=np.int32))
        nodes, dst, src, off = wide.full_neighbor_block(np.array([2, 1], dtype=np.int32))
        torch.cuda.synchronize()
        assert nodes.cpu().tolist() == [2, 1, 0] and dst.cpu().tolist() == [1, 1] and src.cpu().tolist() == [2, 2] and off.cpu().tolist() == [0, 0, 2]
    finally:
        torch.cuda.synchronize()
        wide.close()


@pytest.mark.parametrize("name", sorted(graphs()))
def test_mean_aggregation_over_the_block_is_the_dense_result(world, name):
    """Integer-valued features: every sum is exact in float32 in any order, so the two means agree to the bit."""
    c = world[name]
    indptr, col, seeds = c["indptr"], c["col"], c["seeds"]
    N, D = indptr.size - 1, 4
    X = (np.arange(N * D, dtype=np.int64) * 2654435761 % 17).astype(np.float32).reshape(N, D)
    want = np.zeros((seeds.size, D), dtype=np.float32)
    for i, v in enumerate(seeds.tolist()):
        row = col[indptr[v]:indptr[v + 1]]
        row = row[row >= 0]
        if row.size:
            want[i] = X[row].sum(axis=0, dtype=np.float32) / np.float32(row.size)
    assert np.abs(X).max() * np.diff(indptr).max() < 2 ** 24
    nodes, dst, src, _ = c["graph"].full_neighbor_block(seeds)
    feats = torch.from_numpy(X).to(DEV)[nodes.long()]                  # the block's input features
    live = src >= 0
    h = torch.zeros((seeds.size, D), dtype=torch.float32, device=DEV).index_add_(0, dst[live].long(), feats[src[live].long()])
    cnt = torch.zeros(seeds.size, dtype=torch.float32, device=DEV).index_add_(0, dst[live].long(), torch.ones(int(live.sum()), device=DEV))
    h = torch.where(cnt[:, None] > 0, h / cnt[:, None].clamp(min=1), torch.zeros_like(h))
    torch.cuda.synchronize()
    assert np.array_equal(h.cpu().numpy(), want), name


def test_the_input_nodes_start_a_sampled_batch(world):
    """input_nodes through the host to FeatureStorage.set_ids; one batch of U with fan-out [3, 2]: sampled_ids[:U] are input_nodes in
    order, so src_local and dst_local address the batch's rows, and the batch is edge_ids_ref's."""
    c = world["sym-every-third"]
    indptr, col = c["indptr"], c["col"]
    seeds = c["seeds"][990:1030]                                       # the hub among them
    want = block_conditions(indptr, col, seeds)
    nodes, dst, src, _ = c["graph"].full_neighbor_block(seeds)
    torch.cuda.synchronize()
    ids = nodes.cpu().numpy()
    U = ids.size
    assert np.array_equal(ids, want["input_nodes"]) and 6 in seeds and U > 4000
    fanout = [3, 2]
    wl = Workload(dim=4, indptr=indptr, col=col, n_seeds=64, n_valid=8, n_test=8)
    wl.sets[(0, 0)] = (np.ascontiguousarray(ids), np.ascontiguousarray(wl.labels_all[ids]))
    gpu = GpuSide(wl, U, fanout, edge_ids=True)
    try:
        got = gpu.run(0, 0, 0)
        rows = got["sampled_ids"]
        assert np.array_equal(rows[:U], ids), "the batch's first rows are the block's input nodes, in order"
        s, d = src.cpu().numpy(), dst.cpu().numpy()
        assert np.array_equal(rows[s[s >= 0]], want["src"][s >= 0]) and np.array_equal(rows[d], seeds[want["dst"]])
        ref_batch = edge_ids_ref.run_batch(indptr, col, ids, wl.labels_all[ids], U, 0, fanout, True)
        compare_batches(got, ref_batch, "block input nodes: ")
        assert gpu.pools[0].error() == 0
    finally:
        torch.cuda.synchronize()
        gpu.close()
