"""Random walks on the GPU (GraphStorage.random_walk, legion_random_walk): traces and edge ids bit for bit against the numpy restatement
in tests/walk_ref.py on a hand-built graph -- every workgroup / chunk boundary in walks and steps, uniform and weighted picks, the
restart draw, the whole range of the draw index -- and the C ABI's refusals, the fixed table, and a captured launch."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import walk_ref as ref
from tests import weighted_ref
from tests.compare import same_arrays

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NUM_WALKS = [1, 63, 64, 65, 257, 5000]
LENGTHS = [1, 2, 15, 16, 17, 100]
M31 = 2 ** 31 - 1


@pytest.fixture(scope="module")
def world(hip):
    """The hand-built graph three times over the same device arrays: `graph` with the hand-made weights, `unit` with all weights 1.0f,
    `bare` without a table."""
    from legion_amd import engine
    indptr, col, w = ref.hand_graph()
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


same_walk = functools.partial(same_arrays, names=("trace entries (walk, position)", "edge ids (walk, step)"))


def test_every_index_the_walks_form_is_inside_its_array(world):
    """Before anything runs: over the inputs of this file the rule reads only inside indptr, col and edge_cdf, and a seed outside the
    graph reads nothing (rule 1 comes before any load).  The kernel's own addresses are the rule's (kernels_walk.hip walk_step)."""
    for table, restart in ((None, 0.0), (world["table"], 0.0), (world["table"], 0.3)):
        reads = {}
        ref.walk(world["indptr"], world["col"], ref.seeds_for(5000), 17, table=table, restart_prob=restart, reads=reads)
        ref.assert_reads_in_bounds(reads, ref.NODE_NUM, world["col"].size)
    reads = {}
    out = ref.walk(world["indptr"], world["col"], np.array([-1, ref.NODE_NUM], np.int32), 3, table=world["table"], reads=reads)
    assert np.all(out[0][:, 1:] == -1) and all(i.size == 0 for chunks in reads.values() for i in chunks)


@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("num_walks", NUM_WALKS)
def test_walks_are_the_reference_bit_for_bit(world, num_walks, length):
    """Uniform and weighted, with edge ids; without them the traces are the same."""
    seeds = ref.seeds_for(num_walks)
    d_seeds = torch.from_numpy(seeds).to(DEV)
    for weighted in (False, True):
        ctx = f"{num_walks} x {length} {'weighted' if weighted else 'uniform'}"
        want = ref.walk(world["indptr"], world["col"], seeds, length, table=world["table"] if weighted else None)
        got = world["graph"].random_walk(d_seeds, length, weighted=weighted, return_eids=True)
        only = world["graph"].random_walk(d_seeds, length, weighted=weighted)
        torch.cuda.synchronize()
        same_walk(got, want, ctx)
        ref.check(world["indptr"], world["col"], seeds, got[0].cpu().numpy(), got[1].cpu().numpy())
        assert isinstance(only, torch.Tensor) and torch.equal(only, got[0]), ctx + ": traces without edge ids"


# trace rows of 8, 9, 16, 17 and 32 positions: one chunk of the staging tile exactly and one position into the next, for the chunk of 8
# (edge ids) and of 16 (plain), at one walk and around one tile of 256.  (15, 1), (15, 257), (16, 1) and (16, 257) are cases of
# test_walks_are_the_reference_bit_for_bit above, which this test runs at the rest.
CHUNK_EDGES = [(n, length) for length in (7, 8, 15, 16, 31) for n in (1, 255, 256, 257) if not (n in NUM_WALKS and length in LENGTHS)]


@pytest.mark.parametrize("num_walks, length", CHUNK_EDGES)
def test_chunk_edges_of_the_staging_tile(world, num_walks, length):
    """Uniform and weighted, with edge ids and without, as the grid above."""
    assert len(CHUNK_EDGES) == 16
    test_walks_are_the_reference_bit_for_bit(world, num_walks, length)


@pytest.mark.parametrize("restart", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "weighted"])
@pytest.mark.parametrize("eids", [False, True], ids=["plain", "edge-ids"])
def test_restart(world, weighted, restart, eids):
    seeds = ref.seeds_for(257)
    want = ref.walk(world["indptr"], world["col"], seeds, 17, table=world["table"] if weighted else None, restart_prob=restart, base=40)
    got = world["graph"].random_walk(seeds, 17, weighted=weighted, restart_prob=restart, return_eids=eids, base=40)
    torch.cuda.synchronize()
    if eids:
        same_walk(got, want, f"restart {restart}")
    else:
        assert np.array_equal(got.cpu().numpy(), want[0])
    if restart == 1.0:
        assert np.all(want[0][:, 1:] == -1)
    if restart == 0.0:
        assert (want[0][:, 17] >= 0).any()


def test_unit_weights_are_the_unweighted_walk(world):
    seeds = ref.seeds_for(5000)
    a = world["unit"].random_walk(seeds, 16, weighted=True, return_eids=True, base=9)
    b = world["unit"].random_walk(seeds, 16, weighted=False, return_eids=True, base=9)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    same_walk(a, ref.walk(world["indptr"], world["col"], seeds, 16, base=9), "unit weights")


@pytest.mark.parametrize("base", [0, 1234567890, M31 - 65 * 17], ids=["zero", "mid", "largest"])
def test_base(world, base):
    """The largest legal base: the last walk's last step draws at index 2^31 - 2, its restart draw at 2^32 - 1."""
    seeds = ref.seeds_for(65)
    for weighted, restart in ((False, 0.0), (True, 0.0), (True, 0.3), (False, 0.3)):
        want = ref.walk(world["indptr"], world["col"], seeds, 17, table=world["table"] if weighted else None, restart_prob=restart,
                        base=base)
        got = world["graph"].random_walk(seeds, 17, weighted=weighted, restart_prob=restart, return_eids=True, base=base)
        torch.cuda.synchronize()
        same_walk(got, want, f"base {base} weighted {weighted} restart {restart}")


def test_a_walk_on_another_stream_is_the_default_streams(world):
    """stream=: the launch goes to a stream that is not current (and the call's tensors are recorded on it); same walks."""
    seeds = torch.from_numpy(ref.seeds_for(5000)).to(DEV)
    want = world["graph"].random_walk(seeds, 17, weighted=True, restart_prob=0.3, return_eids=True, base=5)
    plain = world["graph"].random_walk(seeds, 17, base=5)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    assert s != torch.cuda.current_stream()
    got = world["graph"].random_walk(seeds, 17, weighted=True, restart_prob=0.3, return_eids=True, base=5, stream=s)
    only = world["graph"].random_walk(seeds, 17, base=5, stream=s)
    host = world["graph"].random_walk(ref.seeds_for(5000), 17, base=5, stream=s)      # seeds from the host: copied, then walked on s
    s.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(only, plain) and torch.equal(host, plain)
    same_walk(got, ref.walk(world["indptr"], world["col"], seeds.cpu().numpy(), 17, table=world["table"], restart_prob=0.3, base=5), "stream=")


def test_empty_call_returns_empty_arrays(world):
    traces, eids = world["graph"].random_walk(np.zeros(0, np.int32), 3, return_eids=True)
    assert traces.shape == (0, 4) and eids.shape == (0, 3) and traces.dtype == torch.int32 and eids.dtype == torch.int64


def test_c_abi_refusals_leave_the_outputs_untouched(world):
    L = world["L"]
    n, length = 8, 4
    seeds = torch.arange(n, dtype=torch.int32, device=DEV)
    traces = torch.full((n, length + 1), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    eids = torch.full((n, length), 0x5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    g, bare = world["graph"].handle, world["bare"].handle
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    ok = dict(stream=s, graph=g, seeds=P(seeds), n=n, length=length, weighted=0, restart=0.0, base=0, traces=P(traces), eids=P(eids))
    bad = [dict(graph=None), dict(seeds=None), dict(traces=None), dict(n=-1), dict(length=0), dict(length=-2), dict(base=-1),
           dict(base=M31 - n * length + 1), dict(n=2 ** 31 - 1, length=2), dict(weighted=2), dict(weighted=-1),
           dict(graph=bare, weighted=1), dict(restart=float("nan")), dict(restart=-0.25), dict(restart=1.0000001)]
    for change in bad:
        a = dict(ok, **change)
        assert ref.refused(a["n"], a["length"], a["weighted"], a["restart"], a["base"], a["graph"] == g) or \
            None in (a["graph"], a["seeds"], a["traces"]), change
        rc = L.legion_random_walk(a["stream"], a["graph"], a["seeds"], a["n"], a["length"], a["weighted"], a["restart"], a["base"],
                                  a["traces"], a["eids"])
        assert rc == -1, change
    assert L.legion_random_walk(s, g, P(seeds), 0, length, 0, 0.0, 0, P(traces), P(eids)) == 0      # no walks: accepted, nothing runs
    torch.cuda.synchronize()
    assert bool((traces == 0x5A5A5A5A).all()) and bool((eids == 0x5A5A5A5A5A5A).all())
    a = dict(ok, base=M31 - n * length)                                                              # the largest base is legal
    assert L.legion_random_walk(a["stream"], a["graph"], a["seeds"], n, length, 0, 0.0, a["base"], a["traces"], a["eids"]) == 0
    torch.cuda.synchronize()
    assert not bool((traces == 0x5A5A5A5A).any())
    with pytest.raises(ValueError, match="set_edge_weights"):
        world["bare"].random_walk(seeds, length, weighted=True)


def test_a_weighted_walk_fixes_the_table(world):
    from legion_amd import engine
    g = engine.GraphStorage(1, world["graph"].indptr, world["graph"].col)
    try:
        g.set_edge_weights(world["w"])
        g.set_edge_weights(world["w"])                          # replaced freely before the first weighted walk
        g.random_walk(ref.seeds_for(64), 2)                     # ... and an unweighted walk does not fix it
        g.set_edge_weights(world["w"])
        g.random_walk(ref.seeds_for(64), 2, weighted=True)
        torch.cuda.synchronize()
        w = torch.from_numpy(world["w"]).to(DEV)
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert world["L"].legion_graph_set_edge_weights(g.handle, s, ctypes.c_void_p(w.data_ptr())) == -1
        with pytest.raises(RuntimeError):
            g.set_edge_weights(world["w"])
    finally:
        torch.cuda.synchronize()
        g.close()


def test_a_captured_walk_replays_the_eager_result(world):
    L = world["L"]
    n, length = 257, 17
    seeds = torch.from_numpy(ref.seeds_for(n)).to(DEV)
    eager = world["graph"].random_walk(seeds, length, weighted=True, restart_prob=0.3, return_eids=True, base=5)
    traces = torch.zeros((n, length + 1), dtype=torch.int32, device=DEV)
    eids = torch.zeros((n, length), dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = L.legion_random_walk(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), world["graph"].handle,
                                  ctypes.c_void_p(seeds.data_ptr()), n, length, 1, 0.3, 5, ctypes.c_void_p(traces.data_ptr()),
                                  ctypes.c_void_p(eids.data_ptr()))
    assert rc == 0
    for _ in range(2):
        traces.fill_(-7)
        eids.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(traces, eager[0]) and torch.equal(eids, eager[1])
