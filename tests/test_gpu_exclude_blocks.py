"""GraphStorage.seed_edge_exclusion and the exclude_eids keyword of full_neighbor_block, labor_block and sample_distinct_block on the GPU
(DGL's as_edge_prediction_sampler(exclude="self" | "reverse_id")): seed edges drawn from the symmetric graph of tests/node2vec_ref.py,
the blocks around their endpoints with and without the keyword against the references of the ops composed with tests/exclude_ref.py in
numpy; no excluded id among a block's eids, every other edge of the unfiltered block there and in order, full_neighbor_block's offsets
the prefix sums of the kept degrees; the ValueErrors.  The conditions are asserted from numpy alone before any launch."""
import numpy as np
import pytest
import torch

from tests import exclude_ref as ref
from tests import in_edges_ref, labor_ref, link_ref, node2vec_ref, topk_ref
from tests.compare import same_arrays

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = 700                                                            # seed edges
FANOUT = {"labor": 6, "distinct": 5}
SALT = 29
KEYS = ("input_nodes", "dst_local", "src_local", "eids")
MODES = ("self", "reverse_id")
OPS = ("full", "labor", "distinct")


def seed_edges():
    """(indptr, col, seed edge ids, the block's seeds): B distinct live edges -- parallel edges, self-loops and edges without a reverse
    among them -- and their distinct endpoints in order of first appearance, as edge_prediction_seeds lists them."""
    indptr, col, _ = node2vec_ref.sym_graph()
    E = col.size
    rev = ref.reverse_edge_ids(indptr, col, np.arange(E))
    back = ref.reverse_edge_ids(indptr, col, rev)
    live = col >= 0
    special = np.concatenate([np.nonzero(live & (rev < 0))[0][:5], np.nonzero((rev >= 0) & (back != np.arange(E)))[0][:20],
                              np.nonzero(rev == np.arange(E))[0][:10]])
    spread = np.arange(3 * B, dtype=np.int64) * 2654435761 % E
    spread = spread[live[spread] & (np.diff(indptr)[link_ref.find_edges(indptr, col, spread)[0]] < 300)]      # (no hub row: the blocks stay small)
    eids = np.unique(np.concatenate([special, spread]))[:B]
    eids = eids[np.random.RandomState(3).permutation(eids.size)]
    row, c = link_ref.find_edges(indptr, col, eids)
    unique, _, count = link_ref.unique_ids(np.concatenate([row, c]))
    return indptr, col, eids.astype(np.int64), unique[:count]


def unfiltered(op, indptr, col, seeds):
    """The op's block without the keyword, from its own reference, with the global src."""
    if op == "full":
        b = in_edges_ref.full_neighbor_block(indptr, col, seeds)
    elif op == "labor":
        b = labor_ref.block(indptr, col, seeds, FANOUT["labor"], SALT)
    else:
        b = topk_ref.block(indptr, col, None, seeds, FANOUT["distinct"], SALT)
        b["src"] = b["input_nodes"][b["src_local"]]
    return b


def filtered(b, seeds, members):
    """The block with exclude_eids composed in numpy: the filter over the unfiltered block's global triples, then the block tail."""
    nodes, dst, src_local, eid = ref.block_of(seeds, b["dst_local"], b["src"], b["eids"], members)
    out = dict(input_nodes=nodes, dst_local=dst, src_local=src_local, eids=eid)
    out["offsets"] = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=seeds.size))]).astype(np.int64)
    return out


def conditions(indptr, col, eids, seeds):
    """Every (op, mode): the filter drops something, "reverse_id" more than "self"; kept edges are the unfiltered block's others."""
    assert eids.size == B and np.unique(eids).size == B and seeds.size > B
    rev = ref.reverse_edge_ids(indptr, col, eids)
    assert (rev < 0).sum() >= 3 and (rev == eids).sum() >= 5 and np.setdiff1d(rev[rev >= 0], eids).size >= 0.8 * B
    made = {}
    for op in OPS:
        b = unfiltered(op, indptr, col, seeds)
        dropped = {}
        for mode in MODES:
            members = ref.seed_exclusion(indptr, col, eids, mode)
            f = filtered(b, seeds, members)
            gone = np.isin(b["eids"], members[members >= 0])
            assert np.array_equal(f["eids"], b["eids"][~gone]) and not np.isin(f["eids"], members).any()
            dropped[mode] = int(gone.sum())
            made[op, mode] = (members, f)
        assert 0 < dropped["self"] < dropped["reverse_id"] < b["eids"].size, (op, dropped)
        made[op, None] = (None, b)
    assert made["full", "self"][1]["eids"].size == made["full", None][1]["eids"].size - B, "the full block holds every seed edge"
    return made


@pytest.fixture(scope="module")
def world(hip):
    from legion_amd import engine
    indptr, col, eids, seeds = seed_edges()
    made = conditions(indptr, col, eids, seeds)
    graph = engine.GraphStorage(1, torch.from_numpy(indptr).to(DEV), torch.from_numpy(col).to(DEV))
    yield dict(indptr=indptr, col=col, eids=eids, seeds=seeds, made=made, graph=graph)
    torch.cuda.synchronize()
    graph.close()


def run(graph, op, seeds, return_eids, **kw):
    s = torch.from_numpy(seeds).to(DEV)
    if op == "full":
        out = graph.full_neighbor_block(s, return_eids=return_eids, **kw)
        return dict(zip(("input_nodes", "dst_local", "src_local", "offsets", "eids"), out))
    if op == "labor":
        out = graph.labor_block(s, FANOUT["labor"], salt=SALT, return_eids=return_eids, **kw)
    else:
        out = graph.sample_distinct_block(s, FANOUT["distinct"], salt=SALT, return_eids=return_eids, **kw)
    return dict(zip(KEYS, out))


def same_block(got, want, what, return_eids=True):
    keys = [k for k in ("input_nodes", "dst_local", "src_local", "offsets", "eids") if k in got and (return_eids or k != "eids")]
    assert ("eids" in got) == return_eids, what
    same_arrays([got[k] for k in keys], [want[k] for k in keys], what, keys)


@pytest.mark.parametrize("mode", MODES)
def test_the_set_holds_the_seed_edges_and_their_reverses(world, mode):
    w = world
    s = w["graph"].seed_edge_exclusion(w["eids"], exclude=mode)
    members = ref.seed_exclusion(w["indptr"], w["col"], w["eids"], mode)
    assert s.k == members.size
    same_arrays(s.eids, members, f"{mode}: the ids of the set")
    q = np.arange(-2, w["col"].size + 2, dtype=np.int64)
    same_arrays(s.contains(q), ref.contains(members, q), f"{mode}: every edge id of the graph")


@pytest.mark.parametrize("op", OPS)
def test_without_the_keyword_the_block_is_as_before(world, op):
    w = world
    for return_eids in (True, False):
        same_block(run(w["graph"], op, w["seeds"], return_eids), w["made"][op, None][1], f"{op} without exclude_eids", return_eids)
        same_block(run(w["graph"], op, w["seeds"], return_eids, exclude_eids=None), w["made"][op, None][1], f"{op} exclude_eids=None", return_eids)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("op", OPS)
def test_the_block_without_the_excluded_edges(world, op, mode):
    w = world
    members, want = w["made"][op, mode]
    s = w["graph"].seed_edge_exclusion(w["eids"], exclude=mode)
    got = run(w["graph"], op, w["seeds"], True, exclude_eids=s)
    same_block(got, want, f"{op} {mode}")
    eids = got["eids"].cpu().numpy()
    before = w["made"][op, None][1]["eids"]
    assert not np.isin(eids, members).any(), "no excluded id appears"
    assert np.array_equal(eids, before[~np.isin(before, members[members >= 0])]), "every other edge of the unfiltered block, in order"
    if op == "full":
        deg = np.bincount(got["dst_local"].cpu().numpy(), minlength=w["seeds"].size)
        assert np.array_equal(got["offsets"].cpu().numpy(), np.concatenate([[0], np.cumsum(deg)])), "offsets: the kept degrees' prefix sums"
    same_block(run(w["graph"], op, w["seeds"], False, exclude_eids=s), want, f"{op} {mode} without eids", False)


def test_a_set_that_excludes_everything_and_another_stream(world):
    from legion_amd import engine
    w = world
    b = w["made"]["full", None][1]
    everything = engine.EdgeIdSet(b["eids"])
    got = run(w["graph"], "full", w["seeds"], True, exclude_eids=everything)
    n = w["seeds"].size
    assert got["dst_local"].numel() == 0 and got["eids"].numel() == 0 and got["src_local"].numel() == 0
    same_arrays([got["input_nodes"], got["offsets"]], [w["seeds"], np.zeros(n + 1, dtype=np.int64)], "nothing left", ("input_nodes", "offsets"))
    side = torch.cuda.Stream()
    s = w["graph"].seed_edge_exclusion(w["eids"], exclude="reverse_id", stream=side)
    got = run(w["graph"], "labor", w["seeds"], True, exclude_eids=s, stream=side)
    side.synchronize()
    same_block(got, w["made"]["labor", "reverse_id"][1], "labor reverse_id on another stream")


def test_value_errors(world):
    from legion_amd import engine
    g = world["graph"]
    seeds = world["seeds"][:10]
    for bad in ("reverse", "Self", None, 1, b"self", "reverse_types"):
        with pytest.raises(ValueError, match="exclude must be"):
            g.seed_edge_exclusion(world["eids"], exclude=bad)
    for bad in (world["eids"], torch.from_numpy(world["eids"]), [1, 2], "self", 5):
        with pytest.raises(ValueError, match="exclude_eids must be an EdgeIdSet"):
            g.full_neighbor_block(seeds, exclude_eids=bad)
        with pytest.raises(ValueError, match="exclude_eids must be an EdgeIdSet"):
            g.labor_block(seeds, 3, exclude_eids=bad)
        with pytest.raises(ValueError, match="exclude_eids must be an EdgeIdSet"):
            g.sample_distinct_block(seeds, 3, exclude_eids=bad)
    s = engine.EdgeIdSet(world["eids"])
    with pytest.raises(ValueError, match="distinct vertices"):
        g.full_neighbor_block(np.array([5, 9, 5], dtype=np.int32), exclude_eids=s)
