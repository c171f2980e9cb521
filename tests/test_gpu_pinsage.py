"""PinSAGE's neighbour sampler on the GPU (GraphStorage.pinsage_neighbors, legion_pinsage_neighbors): neighbours and counts bit for bit
against the numpy restatement in tests/pinsage_ref.py on the hand-built graph and weights of tests/walk_ref.py -- every class of
visits per seed and both sides of each class edge, tile edges in seeds, uniform and weighted picks, the termination draw, the whole
range of the draw index -- its composition with this build's own random_walk, the C ABI's refusals, the fixed table, and a captured
launch."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import pinsage_ref as ref
from tests import walk_ref
from tests import weighted_ref
from tests.compare import same_arrays

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
M31 = 2 ** 31 - 1
NUM_SEEDS = [1, 3, 64, 65, 257]
SHAPES = [(1, 1, 1),          # the smallest shape
          (10, 2, 3),         # DGL's example
          (7, 9, 5),          # 63 visits
          (8, 8, 64),         # 64 visits = k
          (5, 13, 4),         # 65 visits
          (65, 3, 200),       # k above the visits, more than 64 walks per seed
          (64, 16, 10),       # 1024 visits, the cap
          (3, 11, 5)]
BASE = 40


@pytest.fixture(scope="module")
def world(hip):
    """The hand-built graph three times over the same device arrays: `graph` with the hand-made weights, `unit` with all weights 1.0f,
    `bare` without a table."""
    from legion_amd import engine
    indptr, col, w = walk_ref.hand_graph()
    d_indptr, d_col = torch.from_numpy(indptr).to(DEV), torch.from_numpy(col).to(DEV)
    graphs = {k: engine.GraphStorage(1, d_indptr, d_col) for k in ("graph", "unit", "bare")}
    graphs["graph"].set_edge_weights(w)
    graphs["unit"].set_edge_weights(np.ones(col.size, np.float32))
    torch.cuda.synchronize()
    table = weighted_ref.cdf(indptr, w)
    assert np.array_equal(graphs["graph"].edge_cdf().cpu().numpy().view(np.uint32), table.view(np.uint32)), "edge_cdf"
    yield dict(graphs, indptr=indptr, col=col, w=w, table=table, L=hip)
    for k in ("graph", "unit", "bare"):
        graphs[k].close()


same_slots = functools.partial(same_arrays, names=("neighbours (seed, slot)", "counts (seed, slot)"))


def test_every_index_the_walks_form_is_inside_its_array(world):
    """Before anything runs: over the inputs of this file the rule reads only inside indptr, col and edge_cdf, and a seed outside the
    graph reads nothing (rule 1 comes before any load).  The kernel's own addresses are the rule's (walk_step.h)."""
    for table, p in ((None, 0.0), (world["table"], 0.0), (world["table"], 0.3), (None, 0.5)):
        reads = {}
        ref.visits(world["indptr"], world["col"], walk_ref.seeds_for(257), 10, 2, table=table, termination_prob=p, base=BASE, reads=reads)
        ref.visits(world["indptr"], world["col"], walk_ref.seeds_for(65), 5, 13, table=table, termination_prob=p, base=BASE, reads=reads)
        walk_ref.assert_reads_in_bounds(reads, walk_ref.NODE_NUM, world["col"].size)
    reads = {}
    out = ref.neighbors(world["indptr"], world["col"], np.array([-1, walk_ref.NODE_NUM], np.int32), 10, 2, 3, table=world["table"],
                        reads=reads)
    assert np.all(out[0] == -1) and np.all(out[1] == 0) and all(i.size == 0 for chunks in reads.values() for i in chunks)


@pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "weighted"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("n", NUM_SEEDS)
def test_neighbours_are_the_reference_bit_for_bit(world, n, shape, weighted):
    R, T, k = shape
    seeds = walk_ref.seeds_for(n)
    d_seeds = torch.from_numpy(seeds).to(DEV)
    for p in (0.0, 0.3, 0.5):
        want = ref.neighbors(world["indptr"], world["col"], seeds, R, T, k, table=world["table"] if weighted else None,
                             termination_prob=p, base=BASE)
        got = world["graph"].pinsage_neighbors(d_seeds, R, T, k, termination_prob=p, weighted=weighted, base=BASE)
        torch.cuda.synchronize()
        same_slots(got, want, f"{n} seeds, {shape}, {'weighted' if weighted else 'uniform'}, termination {p}")


@pytest.mark.parametrize("shape", [(10, 2, 3), (5, 13, 4), (65, 3, 200), (64, 16, 10)], ids=lambda s: "x".join(map(str, s)))
def test_composition_with_this_builds_random_walk(world, shape):
    """termination_prob = 0: the result is the count / top-k, done in numpy on the host, of this build's own random_walk traces over
    the seeds repeated R times -- the new kernel tied to the existing one without the reference."""
    R, T, k = shape
    seeds = torch.from_numpy(walk_ref.seeds_for(257)).to(DEV)
    for weighted, base in ((False, 0), (True, 977)):
        traces = world["graph"].random_walk(seeds.repeat_interleave(R), T, weighted=weighted, base=base)
        got = world["graph"].pinsage_neighbors(seeds, R, T, k, termination_prob=0.0, weighted=weighted, base=base)
        torch.cuda.synchronize()
        want = ref.topk(traces.cpu().numpy()[:, 1:].reshape(257, R * T), k)
        same_slots(got, want, f"{shape} weighted {weighted}")


def test_termination_one_leaves_the_first_steps(world):
    seeds = walk_ref.seeds_for(257)
    for weighted in (False, True):
        want = ref.neighbors(world["indptr"], world["col"], seeds, 10, 2, 3, table=world["table"] if weighted else None,
                             termination_prob=1.0, base=BASE)
        got = world["graph"].pinsage_neighbors(seeds, 10, 2, 3, termination_prob=1.0, weighted=weighted, base=BASE)
        torch.cuda.synchronize()
        same_slots(got, want, f"termination 1.0 weighted {weighted}")
        assert np.all(want[1].sum(axis=1) <= 10) and (want[1] > 0).any()      # one visit per walk at the most, and some


def test_unit_weights_are_the_unweighted_sampler(world):
    seeds = walk_ref.seeds_for(257)
    for shape in ((10, 2, 3), (7, 9, 5)):
        a = world["unit"].pinsage_neighbors(seeds, *shape, weighted=True, termination_prob=0.3, base=9)
        b = world["unit"].pinsage_neighbors(seeds, *shape, weighted=False, termination_prob=0.3, base=9)
        torch.cuda.synchronize()
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        same_slots(a, ref.neighbors(world["indptr"], world["col"], seeds, *shape, termination_prob=0.3, base=9), "unit weights")


@pytest.mark.parametrize("base", [0, 1234567890, M31 - 65 * 5 * 13], ids=["zero", "mid", "largest"])
def test_base(world, base):
    """The largest legal base: the last walk's last step draws at index 2^31 - 2, its restart draw at 2^32 - 1."""
    seeds = walk_ref.seeds_for(65)
    for weighted, p in ((False, 0.0), (True, 0.0), (True, 0.3), (False, 0.5)):
        want = ref.neighbors(world["indptr"], world["col"], seeds, 5, 13, 4, table=world["table"] if weighted else None,
                             termination_prob=p, base=base)
        got = world["graph"].pinsage_neighbors(seeds, 5, 13, 4, termination_prob=p, weighted=weighted, base=base)
        torch.cuda.synchronize()
        same_slots(got, want, f"base {base} weighted {weighted} termination {p}")


def test_a_call_on_another_stream_is_the_default_streams(world):
    """stream=: the launch goes to a stream that is not current (and the call's tensors are recorded on it); same neighbourhoods."""
    seeds = torch.from_numpy(walk_ref.seeds_for(257)).to(DEV)
    shapes = [(10, 2, 3), (64, 16, 10)]
    want = [world["graph"].pinsage_neighbors(seeds, *shape, weighted=True, termination_prob=0.3, base=5) for shape in shapes]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    assert s != torch.cuda.current_stream()
    got = [world["graph"].pinsage_neighbors(seeds, *shape, weighted=True, termination_prob=0.3, base=5, stream=s) for shape in shapes]
    host = world["graph"].pinsage_neighbors(walk_ref.seeds_for(257), *shapes[0], weighted=True, termination_prob=0.3, base=5, stream=s)
    s.synchronize()
    for a, b in zip(got + [host], want + [want[0]]):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    same_slots(got[0], ref.neighbors(world["indptr"], world["col"], seeds.cpu().numpy(), *shapes[0], table=world["table"], termination_prob=0.3,
                                     base=5), "stream=")


def test_empty_call_returns_empty_arrays(world):
    nb, ct = world["graph"].pinsage_neighbors(np.zeros(0, np.int32), 10, 2, 3)
    assert nb.shape == ct.shape == (0, 3) and nb.dtype == ct.dtype == torch.int32


def test_c_abi_refusals_leave_the_outputs_untouched(world):
    L = world["L"]
    n, R, T, k = 8, 5, 4, 3
    seeds = torch.arange(n, dtype=torch.int32, device=DEV)
    nb = torch.full((n, k), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    ct = torch.full((n, k), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    g, bare = world["graph"].handle, world["bare"].handle
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    ok = dict(stream=s, graph=g, seeds=P(seeds), n=n, R=R, T=T, k=k, weighted=0, p=0.5, base=0, nb=P(nb), ct=P(ct))

    def call(a):
        return L.legion_pinsage_neighbors(a["stream"], a["graph"], a["seeds"], a["n"], a["R"], a["T"], a["k"], a["weighted"], a["p"],
                                          a["base"], a["nb"], a["ct"])
    bad = [dict(graph=None), dict(seeds=None), dict(nb=None), dict(ct=None), dict(n=-1), dict(R=0), dict(R=-1), dict(T=0), dict(T=-2),
           dict(k=0), dict(k=-3), dict(R=41, T=25), dict(R=1025, T=1), dict(R=1, T=1025), dict(R=2 ** 16, T=2 ** 16), dict(k=1025),
           dict(base=-1), dict(base=M31 - n * R * T + 1), dict(base=2 ** 62), dict(n=2 ** 31 - 1, R=1, T=2), dict(weighted=2),
           dict(weighted=-1), dict(graph=bare, weighted=1), dict(p=float("nan")), dict(p=-0.25), dict(p=1.0000001)]
    for change in bad:
        a = dict(ok, **change)
        assert ref.refused(a["n"], a["R"], a["T"], a["k"], a["weighted"], a["p"], a["base"], a["graph"] == g) or \
            None in (a["graph"], a["seeds"], a["nb"], a["ct"]), change
        assert call(a) == -1, change
    assert call(dict(ok, n=0)) == 0                                            # no seeds: accepted, nothing runs
    torch.cuda.synchronize()
    assert bool((nb == 0x5A5A5A5A).all()) and bool((ct == 0x5A5A5A5A).all())
    assert call(dict(ok, base=M31 - n * R * T)) == 0                           # the largest base is legal
    torch.cuda.synchronize()
    assert not bool((nb == 0x5A5A5A5A).any()) and not bool((ct == 0x5A5A5A5A).any())
    want = ref.neighbors(world["indptr"], world["col"], seeds.cpu().numpy(), R, T, k, termination_prob=0.5, base=M31 - n * R * T)
    same_slots((nb, ct), want, "the largest base through the C ABI")
    with pytest.raises(ValueError, match="set_edge_weights"):
        world["bare"].pinsage_neighbors(seeds, R, T, k, weighted=True)


def test_a_weighted_call_fixes_the_table(world):
    from legion_amd import engine
    g = engine.GraphStorage(1, world["graph"].indptr, world["graph"].col)
    try:
        g.set_edge_weights(world["w"])
        g.set_edge_weights(world["w"])                          # replaced freely before the first weighted call
        g.pinsage_neighbors(walk_ref.seeds_for(64), 10, 2, 3)   # ... and an unweighted call does not fix it
        g.set_edge_weights(world["w"])
        g.pinsage_neighbors(walk_ref.seeds_for(64), 10, 2, 3, weighted=True)
        torch.cuda.synchronize()
        w = torch.from_numpy(world["w"]).to(DEV)
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert world["L"].legion_graph_set_edge_weights(g.handle, s, ctypes.c_void_p(w.data_ptr())) == -1
        with pytest.raises(RuntimeError):
            g.set_edge_weights(world["w"])
    finally:
        torch.cuda.synchronize()
        g.close()


def test_a_captured_call_replays_the_eager_result(world):
    L = world["L"]
    n, R, T, k = 257, 10, 2, 3
    seeds = torch.from_numpy(walk_ref.seeds_for(n)).to(DEV)
    eager = world["graph"].pinsage_neighbors(seeds, R, T, k, weighted=True, termination_prob=0.5, base=5)
    nb = torch.zeros((n, k), dtype=torch.int32, device=DEV)
    ct = torch.zeros((n, k), dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = L.legion_pinsage_neighbors(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), world["graph"].handle,
                                        ctypes.c_void_p(seeds.data_ptr()), n, R, T, k, 1, 0.5, 5, ctypes.c_void_p(nb.data_ptr()),
                                        ctypes.c_void_p(ct.data_ptr()))
    assert rc == 0
    for _ in range(2):
        nb.fill_(-7)
        ct.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(nb, eager[0]) and torch.equal(ct, eager[1])
