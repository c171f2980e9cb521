"""node2vec walks on the GPU (GraphStorage.node2vec_random_walk, legion_node2vec_walk): traces and edge ids bit for bit against the numpy
restatement in tests/node2vec_ref.py on its symmetric graph -- every workgroup / chunk boundary in walks and steps, five (p, q), four
max_tries, uniform, weighted and unit-weight picks, the whole range of the draw index -- p = q = 1 against the GPU's own random_walk, the
C ABI's refusals, a captured launch, another stream, and legion_graph_check_rows_sorted on graphs sorted and not.

The grid is the product thinned: case number c of the 36 (walks, steps) pairs takes (p, q) number c mod 5, max_tries number c mod 4,
the weights c mod 3 and the base (c div 3) mod 3 -- 5, 4 and 3 are coprime, so every value meets every other somewhere -- and runs with
and without edge ids.  The references are computed once, with the counters that show, before any launch, what the cases exercise."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import node2vec_ref as ref
from tests import walk_ref
from tests import weighted_ref
from tests.compare import same_arrays

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NUM_WALKS = [1, 63, 64, 65, 257, 5000]
LENGTHS = [1, 2, 15, 16, 17, 100]
PQ = [(1.0, 1.0), (0.5, 2.0), (4.0, 0.25), (0.25, 4.0), (16.0, 1.0)]
TRIES = [256, 2, 3, 1]
WEIGHTS = ["uniform", "weighted", "unit"]
M31 = 2 ** 31 - 1


def case(num_walks, length):
    c = NUM_WALKS.index(num_walks) * len(LENGTHS) + LENGTHS.index(length)
    base = [0, 1234567890, M31 - num_walks * length][(c // 3) % 3]
    return dict(n=num_walks, length=length, pq=PQ[c % 5], tries=TRIES[c % 4], weights=WEIGHTS[c % 3], base=base)


CASES = [case(n, length) for n in NUM_WALKS for length in LENGTHS]


@pytest.fixture(scope="module")
def world(hip):
    """The symmetric graph three times over the same device arrays: `graph` with the hand-made weights, `unit` with all weights 1.0f,
    `bare` without a table and never checked for sorted rows; and `want(case)`, the reference of a grid case, computed once."""
    from legion_amd import engine
    indptr, col, w = ref.sym_graph()
    d_indptr, d_col = torch.from_numpy(indptr).to(DEV), torch.from_numpy(col).to(DEV)
    graphs = {k: engine.GraphStorage(1, d_indptr, d_col) for k in ("graph", "unit", "bare")}
    graphs["graph"].set_edge_weights(w)
    graphs["unit"].set_edge_weights(np.ones(col.size, np.float32))
    torch.cuda.synchronize()
    table = weighted_ref.cdf(indptr, w)
    assert np.array_equal(graphs["graph"].edge_cdf().cpu().numpy().view(np.uint32), table.view(np.uint32)), "edge_cdf"
    unit = weighted_ref.cdf(indptr, np.ones(col.size, np.float32))
    made = {}

    def want(c):
        key = (c["n"], c["length"])
        if key not in made:
            stats, reads = ref.new_stats(), {}
            tab = {"uniform": None, "weighted": table, "unit": unit}[c["weights"]]
            out = ref.walk(indptr, col, ref.seeds_for(c["n"]), c["length"], *c["pq"], table=tab, max_tries=c["tries"], base=c["base"],
                           reads=reads, stats=stats)
            walk_ref.assert_reads_in_bounds(reads, ref.NODE_NUM, col.size)
            made[key] = (out, stats)
        return made[key]

    yield dict(graphs, indptr=indptr, col=col, w=w, table=table, L=hip, want=want)
    for k in ("graph", "unit", "bare"):
        graphs[k].close()


same_walk = functools.partial(same_arrays, names=("trace entries (walk, position)", "edge ids (walk, step)"))


def test_the_cases_show_every_class_before_any_launch(world):
    """From the reference's counters alone: over the grid each class of candidate (return, neighbour of t, other) was both accepted and
    rejected at least 100 times by an accept draw, the forced last try fired at least 100 times, the search that an early decision cannot
    avoid ran, also over the 4 097-entry row, and every value of the grid's axes is in some case.  Every index read was inside its array
    (world.want asserts it per case)."""
    acc, rej, forced, searches, rows = [0, 0, 0], [0, 0, 0], 0, 0, set()
    for c in CASES:
        s = world["want"](c)[1]
        for k in range(3):
            acc[k] += s["accepted"][k]
            rej[k] += s["rejected"][k]
        if c["tries"] > 1:
            forced += s["forced"]
        searches += s["searches"]
        rows |= s["searched_rows"]
    print("accepted", acc, "rejected", rej, "forced", forced, "searches", searches, "rows searched", len(rows))
    assert min(acc) >= 100 and min(rej) >= 100, (acc, rej)
    assert forced >= 100 and searches >= 100 and 6 in rows and ref.HUBS[6] == 4097
    for axis, values in (("pq", PQ), ("tries", TRIES), ("weights", WEIGHTS)):
        assert {c[axis] for c in CASES} == set(values), axis
    assert {(c["base"] == 0, c["base"] + c["n"] * c["length"] == M31) for c in CASES} == {(True, False), (False, True), (False, False)}


@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("num_walks", NUM_WALKS)
def test_walks_are_the_reference_bit_for_bit(world, num_walks, length):
    """With edge ids; without them the traces are the same."""
    c = case(num_walks, length)
    want = world["want"](c)[0]
    g = world["unit" if c["weights"] == "unit" else "graph"]
    seeds = torch.from_numpy(ref.seeds_for(num_walks)).to(DEV)
    kw = dict(weighted=c["weights"] != "uniform", max_tries=c["tries"], base=c["base"])
    got = g.node2vec_random_walk(seeds, *c["pq"], length, return_eids=True, **kw)
    only = g.node2vec_random_walk(seeds, *c["pq"], length, **kw)
    torch.cuda.synchronize()
    same_walk(got, want, str(c))
    walk_ref.check(world["indptr"], world["col"], seeds.cpu().numpy(), got[0].cpu().numpy(), got[1].cpu().numpy())
    assert isinstance(only, torch.Tensor) and torch.equal(only, got[0]), str(c) + ": traces without edge ids"


# trace rows of 8, 9, 16, 17 and 32 positions: one chunk of the staging tile exactly and one position into the next, for the chunk of 8
# (edge ids) and of 16 (plain), at one walk and around one tile of 256.  (15, 1), (15, 257), (16, 1) and (16, 257) are cases of
# test_walks_are_the_reference_bit_for_bit above.
CHUNK_EDGES = [(n, length) for length in (7, 8, 15, 16, 31) for n in (1, 255, 256, 257) if not (n in NUM_WALKS and length in LENGTHS)]


@pytest.mark.parametrize("num_walks, length", CHUNK_EDGES)
def test_chunk_edges_of_the_staging_tile(world, num_walks, length):
    """With edge ids and without; case number c takes the biased (p, q) number c mod 4 and is weighted when c is odd."""
    assert len(CHUNK_EDGES) == 16
    c = CHUNK_EDGES.index((num_walks, length))
    pq, weighted = PQ[1 + c % 4], c % 2 == 1
    seeds = ref.seeds_for(num_walks)
    reads = {}
    want = ref.walk(world["indptr"], world["col"], seeds, length, *pq, table=world["table"] if weighted else None, base=77, reads=reads)
    walk_ref.assert_reads_in_bounds(reads, ref.NODE_NUM, world["col"].size)
    d_seeds = torch.from_numpy(seeds).to(DEV)
    got = world["graph"].node2vec_random_walk(d_seeds, *pq, length, weighted=weighted, return_eids=True, base=77)
    only = world["graph"].node2vec_random_walk(d_seeds, *pq, length, weighted=weighted, base=77)
    torch.cuda.synchronize()
    ctx = f"{num_walks} x {length}, (p, q) = {pq}, {'weighted' if weighted else 'uniform'}"
    same_walk(got, want, ctx)
    assert isinstance(only, torch.Tensor) and torch.equal(only, got[0]), ctx + ": traces without edge ids"


@pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "weighted"])
@pytest.mark.parametrize("num_walks, length", [(5000, 17), (257, 100), (65, 1)])
def test_unbiased_walks_are_the_random_walk_kernels(world, num_walks, length, weighted):
    """p = q = 1 runs the node2vec kernel (every candidate's weight is the envelope): its pin against random_walk_kernel.  max_tries = 1
    with a bias is the same walk."""
    seeds = torch.from_numpy(ref.seeds_for(num_walks)).to(DEV)
    g = world["graph"]
    a = g.random_walk(seeds, length, weighted=weighted, return_eids=True, base=9)
    b = g.node2vec_random_walk(seeds, 1.0, 1.0, length, weighted=weighted, return_eids=True, base=9)
    c = g.node2vec_random_walk(seeds, 0.25, 4.0, length, weighted=weighted, return_eids=True, max_tries=1, base=9)
    d = g.node2vec_random_walk(seeds, 1.0, 1.0, length, weighted=weighted, base=9)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0], c[0]) and torch.equal(a[1], c[1]) and torch.equal(a[0], d)
    assert (a[0][:, -1] >= 0).any()


def test_a_walk_on_another_stream_is_the_default_streams(world):
    """stream=: the launch goes to a stream that is not current (and the call's tensors are recorded on it); same walks."""
    seeds = torch.from_numpy(ref.seeds_for(5000)).to(DEV)
    g = world["graph"]
    want = g.node2vec_random_walk(seeds, 0.5, 2.0, 17, weighted=True, return_eids=True, base=5)
    plain = g.node2vec_random_walk(seeds, 4.0, 0.25, 17, base=5)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    assert s != torch.cuda.current_stream()
    got = g.node2vec_random_walk(seeds, 0.5, 2.0, 17, weighted=True, return_eids=True, base=5, stream=s)
    only = g.node2vec_random_walk(seeds, 4.0, 0.25, 17, base=5, stream=s)
    host = g.node2vec_random_walk(ref.seeds_for(5000), 4.0, 0.25, 17, base=5, stream=s)      # seeds from the host: copied, then walked on s
    s.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(only, plain) and torch.equal(host, plain)
    same_walk(got, ref.walk(world["indptr"], world["col"], seeds.cpu().numpy(), 17, 0.5, 2.0, table=world["table"], base=5), "stream=")


def test_empty_call_returns_empty_arrays(world):
    traces, eids = world["graph"].node2vec_random_walk(np.zeros(0, np.int32), 0.5, 2.0, 3, return_eids=True)
    assert traces.shape == (0, 4) and eids.shape == (0, 3) and traces.dtype == torch.int32 and eids.dtype == torch.int64


def test_c_abi_refusals_leave_the_outputs_untouched(world):
    from legion_amd import engine
    L = world["L"]
    n, length = 8, 4
    seeds = torch.arange(n, dtype=torch.int32, device=DEV)
    traces = torch.full((n, length + 1), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    eids = torch.full((n, length), 0x5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    hand = walk_ref.hand_graph()                                                                     # its rows are not sorted
    assert not ref.rows_sorted(hand[0], hand[1])
    unsorted = engine.GraphStorage(1, torch.from_numpy(hand[0]).to(DEV), torch.from_numpy(hand[1]).to(DEV))
    try:
        assert world["graph"].rows_sorted() is True and unsorted.rows_sorted() is False
        sorted_of = {world["graph"].handle: 1, world["unit"].handle: 1, world["bare"].handle: -1, unsorted.handle: 0}
        g, bare = world["graph"].handle, world["bare"].handle
        P = lambda t: ctypes.c_void_p(t.data_ptr())
        ok = dict(stream=s, graph=g, seeds=P(seeds), n=n, length=length, p=0.5, q=2.0, weighted=0, tries=256, base=0, traces=P(traces),
                  eids=P(eids))
        bad = [dict(graph=None), dict(seeds=None), dict(traces=None), dict(n=-1), dict(length=0), dict(length=-2), dict(base=-1),
               dict(base=M31 - n * length + 1), dict(n=2 ** 31 - 1, length=2), dict(weighted=2), dict(weighted=-1),
               dict(graph=bare, weighted=1), dict(tries=0), dict(tries=257), dict(tries=-1),
               dict(p=0.0), dict(p=-1.0), dict(p=float("nan")), dict(p=float("inf")), dict(q=0.0), dict(q=-2.0), dict(q=float("nan")),
               dict(q=float("inf")), dict(p=16.5, q=1.0), dict(p=1.0, q=17.0), dict(p=0.06, q=1.0), dict(p=8.0, q=0.25),
               dict(graph=bare), dict(graph=unsorted.handle), dict(graph=unsorted.handle, p=1.0, q=1.0)]
        for change in bad:
            a = dict(ok, **change)
            assert None in (a["graph"], a["seeds"], a["traces"]) or \
                ref.refused(a["n"], a["length"], a["p"], a["q"], a["weighted"], a["tries"], a["base"], a["graph"] == g, sorted_of[a["graph"]]), change
            rc = L.legion_node2vec_walk(a["stream"], a["graph"], a["seeds"], a["n"], a["length"], a["p"], a["q"], a["weighted"], a["tries"],
                                        a["base"], a["traces"], a["eids"])
            assert rc == -1, change
        assert L.legion_node2vec_walk(s, g, P(seeds), 0, length, 0.5, 2.0, 0, 256, 0, P(traces), P(eids)) == 0      # no walks: nothing runs
        torch.cuda.synchronize()
        assert bool((traces == 0x5A5A5A5A).all()) and bool((eids == 0x5A5A5A5A5A5A).all())
        for change in (dict(base=M31 - n * length), dict(p=16.0, q=1.0), dict(p=0.0625, q=1.0), dict(tries=1)):      # the legal edges
            a = dict(ok, **change)
            traces.fill_(0x5A5A5A5A)
            assert L.legion_node2vec_walk(a["stream"], a["graph"], a["seeds"], n, length, a["p"], a["q"], 0, a["tries"], a["base"],
                                          a["traces"], a["eids"]) == 0, change
            torch.cuda.synchronize()
            assert not bool((traces == 0x5A5A5A5A).any()), change
        with pytest.raises(ValueError, match="set_edge_weights"):
            world["bare"].node2vec_random_walk(seeds, 1.0, 1.0, length, weighted=True)
        with pytest.raises(ValueError, match="sorted"):
            unsorted.node2vec_random_walk(seeds, 1.0, 1.0, length)
        assert L.legion_graph_check_rows_sorted(bare, s) == 1                                         # checked now: the same call is taken
        a = ok
        assert L.legion_node2vec_walk(s, bare, a["seeds"], n, length, 0.5, 2.0, 0, 256, 0, a["traces"], a["eids"]) == 0
        torch.cuda.synchronize()
    finally:
        torch.cuda.synchronize()
        unsorted.close()


def test_a_weighted_walk_fixes_the_table(world):
    from legion_amd import engine
    g = engine.GraphStorage(1, world["graph"].indptr, world["graph"].col)
    try:
        g.set_edge_weights(world["w"])
        g.node2vec_random_walk(ref.seeds_for(64), 0.5, 2.0, 2)      # an unweighted walk does not fix it
        g.set_edge_weights(world["w"])
        g.node2vec_random_walk(ref.seeds_for(64), 0.5, 2.0, 2, weighted=True)
        torch.cuda.synchronize()
        with pytest.raises(RuntimeError):
            g.set_edge_weights(world["w"])
    finally:
        torch.cuda.synchronize()
        g.close()


def test_a_captured_walk_replays_the_eager_result(world):
    L = world["L"]
    n, length = 257, 17
    seeds = torch.from_numpy(ref.seeds_for(n)).to(DEV)
    eager = world["graph"].node2vec_random_walk(seeds, 4.0, 0.25, length, weighted=True, return_eids=True, base=5)
    traces = torch.zeros((n, length + 1), dtype=torch.int32, device=DEV)
    eids = torch.zeros((n, length), dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    same_walk(eager, ref.walk(world["indptr"], world["col"], seeds.cpu().numpy(), length, 4.0, 0.25, table=world["table"], base=5), "eager")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = L.legion_node2vec_walk(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), world["graph"].handle,
                                    ctypes.c_void_p(seeds.data_ptr()), n, length, 4.0, 0.25, 1, 256, 5, ctypes.c_void_p(traces.data_ptr()),
                                    ctypes.c_void_p(eids.data_ptr()))
    assert rc == 0
    for _ in range(2):
        traces.fill_(-7)
        eids.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(traces, eager[0]) and torch.equal(eids, eager[1])


# ---- legion_graph_check_rows_sorted -----------------------------------------------------------------------------------------------
def _small():
    """Rows {5, 9}, two empty rows, {1, 3}, an empty row, {0, 0, 7}: sorted, with a decrease exactly across a row boundary (9 -> 1) that has
    empty rows on either side of it."""
    return np.array([0, 2, 2, 2, 4, 4, 7], dtype=np.int64), np.array([5, 9, 1, 3, 0, 0, 7], dtype=np.int32)


def _sorted_cases():
    indptr, col, _ = ref.sym_graph()
    out = {"sorted": (indptr, col, True)}
    last = int(np.nonzero(np.diff(indptr) >= 2)[0][-1])
    assert indptr[last + 1] == col.size                             # the last row: its last two entries the other way round
    c = col.copy()
    assert c[-2] < c[-1]
    c[-2], c[-1] = c[-1], c[-2]
    out["last-row"] = (indptr, c, False)
    c = col.copy()
    at = int(indptr[6]) + 2048                                      # inside the 4 097-entry row
    assert c[at] < c[at + 1]
    c[at], c[at + 1] = c[at + 1], c[at]
    out["long-row"] = (indptr, c, False)
    ip, c = _small()
    out["across-a-boundary"] = (ip, c, True)
    c = c.copy()
    c[0], c[1] = 9, 5                                               # position 1 of a two-entry row
    out["two-entry-row"] = (ip, c, False)
    out["no-edges"] = (np.zeros(5, dtype=np.int64), np.zeros(0, dtype=np.int32), True)
    out["one-edge"] = (np.array([0, 0, 1], dtype=np.int64), np.array([1], dtype=np.int32), True)
    return out


@pytest.mark.parametrize("name", ["sorted", "last-row", "long-row", "across-a-boundary", "two-entry-row", "no-edges", "one-edge"])
def test_check_rows_sorted(hip, name):
    from legion_amd import engine
    indptr, col, want = _sorted_cases()[name]
    assert ref.rows_sorted(indptr, col) == want
    g = engine.GraphStorage(1, torch.from_numpy(indptr).to(DEV), torch.from_numpy(col).to(DEV))
    try:
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert hip.legion_graph_check_rows_sorted(g.handle, s) == int(want)
        assert hip.legion_graph_check_rows_sorted(g.handle, s) == int(want)      # the remembered value
        assert g.rows_sorted() is want and g.rows_sorted() is want
    finally:
        torch.cuda.synchronize()
        g.close()
