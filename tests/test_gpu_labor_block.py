"""GraphStorage.labor_block on the GPU (DGL's LaborSampler with one fan-out): against tests/labor_ref.py -- the seeds first and in order,
input_nodes[src_local] the kept sources, dst_local the position of the seed -- both ValueErrors, a fan-out of the largest degree against
full_neighbor_block without its dead entries, two layers with one salt (a vertex kept for a seed of degree d is kept for every seed of
degree <= d that has it as a neighbour), a mean aggregation over the block in torch against the dense numpy result, and input_nodes
handed on to FeatureStorage.set_ids: a batch's sampled_ids start with them in order."""
import numpy as np
import pytest
import torch

from tests import edge_ids_ref
from tests import labor_ref as ref
from tests import link_ref, node2vec_ref
from tests.gpu_harness import GpuSide
from tests.helpers import Workload, compare_batches

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FANOUT = {"sym-every-third": 5, "ring": 1, "complete": 3}
SALT = 11


def graphs():
    """name -> (indptr, col, distinct seeds)."""
    indptr, col, _ = node2vec_ref.sym_graph()
    third = np.arange(0, node2vec_ref.NODE_NUM, 3, dtype=np.int32)
    third = np.concatenate([third[1000:], third[:1000]])           # not in ascending order: the hub (6) is the 1 003rd seed
    ring, complete = link_ref.ring_graph(8), link_ref.complete_graph(8)
    return {"sym-every-third": (indptr, col, third), "ring": ring + (np.array([5, 0, 3], dtype=np.int32),),
            "complete": complete + (np.arange(8, dtype=np.int32)[::-1].copy(),)}


def block_conditions(indptr, col, seeds, fanout, salt=SALT):
    b = ref.block(indptr, col, seeds, fanout, salt)
    n, nodes = seeds.size, b["input_nodes"]
    assert np.array_equal(nodes[:n], seeds) and np.unique(nodes).size == nodes.size and nodes.min() >= 0
    assert np.all(b["src"] >= 0) and np.array_equal(nodes[b["src_local"]], b["src"]), "dead entries are never kept"
    assert np.array_equal(b["dst_local"], b["dst"]) and np.all(np.diff(b["dst"]) >= 0)
    assert np.array_equal(col[b["eids"]], b["src"])
    return b


@pytest.fixture(scope="module")
def world(hip):
    from legion_amd import engine
    made = {}
    for name, (indptr, col, seeds) in graphs().items():
        made[name] = dict(indptr=indptr, col=col, seeds=seeds, want=block_conditions(indptr, col, seeds, FANOUT[name]),
                          graph=engine.GraphStorage(1, torch.from_numpy(indptr).to(DEV), torch.from_numpy(col).to(DEV)))
    yield made
    torch.cuda.synchronize()
    for c in made.values():
        c["graph"].close()


def test_the_inputs_hold_their_conditions_before_any_launch(world):
    c = world["sym-every-third"]
    b = c["want"]
    full = int(np.diff(c["indptr"])[c["seeds"]].sum())
    assert c["seeds"].size == 2000 and 6 in c["seeds"] and 2000 < b["src"].size < full and b["input_nodes"].size > 3000
    assert (b["src_local"] < 2000).sum() >= 100, "sources that are seeds themselves"
    assert np.unique(b["dst"]).size < 2000, "a seed that keeps nothing"
    for name in ("ring", "complete"):
        w = world[name]["want"]
        assert 0 < w["src"].size < int(np.diff(world[name]["indptr"])[world[name]["seeds"]].sum()), name


@pytest.mark.parametrize("eids", [False, True], ids=["no-eids", "eids"])
@pytest.mark.parametrize("name", sorted(graphs()))
def test_the_block_is_the_reference(world, name, eids):
    c = world[name]
    got = c["graph"].labor_block(torch.from_numpy(c["seeds"]).to(DEV), FANOUT[name], salt=SALT, return_eids=eids)
    torch.cuda.synchronize()
    assert len(got) == (4 if eids else 3)
    for key, x in zip(("input_nodes", "dst_local", "src_local", "eids"), got):
        x, w = x.cpu().numpy(), c["want"][key]
        assert x.dtype == w.dtype and np.array_equal(x, w), f"{name}: {key}"


def test_both_value_errors(world, hip):
    from legion_amd import engine
    g = world["sym-every-third"]["graph"]
    N = node2vec_ref.NODE_NUM
    for seeds in ([5, 9, 5], [5, -1, 9], [5, N, 9], [N + 3]):
        with pytest.raises(ValueError, match="distinct vertices"):
            g.labor_block(np.array(seeds, dtype=np.int32), 5)
    g.labor_block(np.array([5, 9], dtype=np.int32), 5)
    # one row of 2^20 entries: a fan-out of its degree keeps them all, with the seed one id more than unique_ids takes
    big = 2 ** 20
    indptr = np.array([0, big, big + 2, big + 2], dtype=np.int64)
    col = torch.zeros(big + 2, dtype=torch.int32, device=DEV)
    wide = engine.GraphStorage(1, torch.from_numpy(indptr).to(DEV), col)
    try:
        assert 1 + big > engine.UNIQUE_MAX_IDS
        with pytest.raises(ValueError, match="at most"):
            wide.labor_block(np.array([0], dtype=np.int32), big)
        assert not ref.keep_one(ref.hashes([0], 0)[0], big, 1000), "every entry is vertex 0: at a small fan-out none is kept"
        nodes, dst, src = wide.labor_block(np.array([0], dtype=np.int32), 1000)
        assert nodes.cpu().tolist() == [0] and dst.shape == (0,) and src.shape == (0,)
        nodes, dst, src = wide.labor_block(np.array([2, 1], dtype=np.int32), 2)      # (degree 2: every entry)
        torch.cuda.synchronize()
        assert nodes.cpu().tolist() == [2, 1, 0] and dst.cpu().tolist() == [1, 1] and src.cpu().tolist() == [2, 2]
    finally:
        torch.cuda.synchronize()
        wide.close()


@pytest.mark.parametrize("name", sorted(graphs()))
def test_the_largest_degree_as_fanout_is_the_full_block_without_dead_entries(world, name):
    c = world[name]
    fanout = int(np.diff(c["indptr"]).max())
    seeds = torch.from_numpy(c["seeds"]).to(DEV)
    nodes, dst, src, eids = c["graph"].labor_block(seeds, fanout, salt=SALT, return_eids=True)
    f_nodes, f_dst, f_src, _, f_eids = c["graph"].full_neighbor_block(seeds, return_eids=True)
    torch.cuda.synchronize()
    live = f_src >= 0
    assert name != "sym-every-third" or int((~live).sum()) >= 3
    assert torch.equal(nodes, f_nodes) and torch.equal(dst, f_dst[live]) and torch.equal(src, f_src[live]) and torch.equal(eids, f_eids[live])


def two_layer_case(indptr, col, seeds):
    """The reference blocks of two layers at fan-out 5: the inner one, the outer one (its seeds are the inner layer's input nodes) with
    the same salt, and the outer one with another salt.  With one salt a source vertex has the same number in both layers, so a vertex
    kept for a seed of degree d is kept for every seed of degree <= d that has it as a neighbour, in either layer; with a salt per
    layer that fails somewhere, and the outer layer needs more input nodes."""
    deg = np.diff(indptr)
    inner = block_conditions(indptr, col, seeds, 5)
    outer = block_conditions(indptr, col, inner["input_nodes"], 5)
    other = block_conditions(indptr, col, inner["input_nodes"], 5, salt=SALT + 1)
    layers = {"inner": (seeds, inner), "outer": (inner["input_nodes"], outer), "other": (inner["input_nodes"], other)}
    pairs = {k: set(zip(s[b["dst"]].tolist(), b["src"].tolist())) for k, (s, b) in layers.items()}      # (seed vertex, kept neighbour)
    top = {}                                                       # vertex -> the largest degree of a seed it was kept for, one salt
    for k in ("inner", "outer"):
        for s, t in pairs[k]:
            top[t] = max(top.get(t, 0), int(deg[s]))

    def broken(k):
        """the (seed, neighbour) pairs of layer k that the rule says are kept but are not"""
        return sum(1 for s in layers[k][0].tolist() for t in col[indptr[s]:indptr[s + 1]].tolist()
                   if t >= 0 and deg[s] <= top.get(t, 0) and (s, t) not in pairs[k])

    assert len(top) > 500 and broken("inner") == 0 and broken("outer") == 0
    assert broken("other") > 0, "a salt per layer draws anew"
    assert other["input_nodes"].size > outer["input_nodes"].size, "and needs more input nodes"
    return inner, outer, other


def test_two_layers_with_one_salt(world):
    c = world["sym-every-third"]
    g, seeds = c["graph"], c["seeds"][:300]
    inner, outer, other = two_layer_case(c["indptr"], c["col"], seeds)
    nodes1 = g.labor_block(seeds, 5, salt=SALT)[0]
    got = {"inner": g.labor_block(seeds, 5, salt=SALT), "outer": g.labor_block(nodes1, 5, salt=SALT),
           "other": g.labor_block(nodes1, 5, salt=SALT + 1)}
    torch.cuda.synchronize()
    for name, want in (("inner", inner), ("outer", outer), ("other", other)):
        for key, x in zip(("input_nodes", "dst_local", "src_local"), got[name]):
            assert np.array_equal(x.cpu().numpy(), want[key]), f"{name}: {key}"


@pytest.mark.parametrize("name", sorted(graphs()))
def test_mean_aggregation_over_the_block_is_the_dense_result(world, name):
    """Integer-valued features: every sum is exact in float32 in any order, so the two means agree to the bit."""
    c = world[name]
    indptr, col, seeds, fanout = c["indptr"], c["col"], c["seeds"], FANOUT[name]
    N, D = indptr.size - 1, 4
    X = (np.arange(N * D, dtype=np.int64) * 2654435761 % 17).astype(np.float32).reshape(N, D)
    want = np.zeros((seeds.size, D), dtype=np.float32)
    for i, v in enumerate(seeds.tolist()):
        row = col[indptr[v]:indptr[v + 1]]
        d = row.size
        row = np.array([t for t in row.tolist() if t >= 0 and ref.keep_one(ref.hashes([t], SALT)[0], d, fanout)], dtype=np.int64)
        if row.size:
            want[i] = X[row].sum(axis=0, dtype=np.float32) / np.float32(row.size)
    assert np.abs(X).max() * np.diff(indptr).max() < 2 ** 24 and np.any(want != 0)
    nodes, dst, src = c["graph"].labor_block(seeds, fanout, salt=SALT)
    feats = torch.from_numpy(X).to(DEV)[nodes.long()]                  # the block's input features
    h = torch.zeros((seeds.size, D), dtype=torch.float32, device=DEV).index_add_(0, dst.long(), feats[src.long()])
    cnt = torch.zeros(seeds.size, dtype=torch.float32, device=DEV).index_add_(0, dst.long(), torch.ones(int(dst.numel()), device=DEV))
    h = torch.where(cnt[:, None] > 0, h / cnt[:, None].clamp(min=1), torch.zeros_like(h))
    torch.cuda.synchronize()
    assert np.array_equal(h.cpu().numpy(), want), name


def test_the_input_nodes_start_a_sampled_batch(world):
    """input_nodes through the host to FeatureStorage.set_ids; one batch of U with fan-out [3, 2]: sampled_ids[:U] are input_nodes in
    order, so src_local and dst_local address the batch's rows, and the batch is edge_ids_ref's."""
    c = world["sym-every-third"]
    indptr, col = c["indptr"], c["col"]
    seeds = c["seeds"][990:1030]                                       # the hub among them
    want = block_conditions(indptr, col, seeds, 25)
    nodes, dst, src = c["graph"].labor_block(seeds, 25, salt=SALT)
    torch.cuda.synchronize()
    ids = nodes.cpu().numpy()
    U = ids.size
    assert np.array_equal(ids, want["input_nodes"]) and 6 in seeds and 100 < U < 4000
    fanout = [3, 2]
    wl = Workload(dim=4, indptr=indptr, col=col, n_seeds=64, n_valid=8, n_test=8)
    wl.sets[(0, 0)] = (np.ascontiguousarray(ids), np.ascontiguousarray(wl.labels_all[ids]))
    gpu = GpuSide(wl, U, fanout, edge_ids=True)
    try:
        got = gpu.run(0, 0, 0)
        rows = got["sampled_ids"]
        assert np.array_equal(rows[:U], ids), "the batch's first rows are the block's input nodes, in order"
        s, d = src.cpu().numpy(), dst.cpu().numpy()
        assert np.array_equal(rows[s], want["src"]) and np.array_equal(rows[d], seeds[want["dst"]])
        ref_batch = edge_ids_ref.run_batch(indptr, col, ids, wl.labels_all[ids], U, 0, fanout, True)
        compare_batches(got, ref_batch, "block input nodes: ")
        assert gpu.pools[0].error() == 0
    finally:
        torch.cuda.synchronize()
        gpu.close()
