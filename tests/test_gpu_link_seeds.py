"""The seeds of a link-prediction batch on the GPU, end to end: GraphStorage.edge_prediction_seeds against the three references of
tests/link_ref.py chained, the local indices giving back the endpoints, each op captured into a graph and on a stream that is not
current, the C ABI's refusals leaving sentinel-filled buffers untouched, and the distinct seeds handed to FeatureStorage.set_ids: the
batch's sampled_ids start with them in order, so the local indices address the batch's rows."""
import ctypes

import numpy as np
import pytest
import torch

from tests import edge_ids_ref
from tests import link_ref as ref
from tests import node2vec_ref, walk_ref
from tests.gpu_harness import GpuSide
from tests.helpers import Workload, compare_batches

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
M31 = 2 ** 31 - 1
SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def world(hip):
    """`graph` checked sorted by its first use, `bare` over the same arrays never checked, `unsorted` over walk_ref's hand graph."""
    from legion_amd import engine
    indptr, col, _ = node2vec_ref.sym_graph()
    d_indptr, d_col = torch.from_numpy(indptr).to(DEV), torch.from_numpy(col).to(DEV)
    graph, bare = engine.GraphStorage(1, d_indptr, d_col), engine.GraphStorage(1, d_indptr, d_col)
    hand = walk_ref.hand_graph()
    assert not node2vec_ref.rows_sorted(hand[0], hand[1])
    unsorted = engine.GraphStorage(1, torch.from_numpy(hand[0]).to(DEV), torch.from_numpy(hand[1]).to(DEV))
    assert graph.rows_sorted() is True and unsorted.rows_sorted() is False
    yield dict(graph=graph, bare=bare, unsorted=unsorted, indptr=indptr, col=col, L=hip)
    torch.cuda.synchronize()
    for g in (graph, bare, unsorted):
        g.close()


def _eq(got, want, ctx):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, f"{ctx}: {got.dtype} {got.shape}"
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{ctx}: {len(bad)} entries differ, first at {bad[0]}: got {got[tuple(bad[0])]} want {want[tuple(bad[0])]}"


# ---- the composite ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B, k, kw", [(257, 5, dict()), (5000, 1, dict(base=1234567890)), (65, 64, dict(exclude_self=False, max_tries=2)),
                                      (1, 3, dict(exclude_edges=False, base=M31 - 3))])
def test_edge_prediction_seeds_is_the_three_references_chained(world, B, k, kw):
    indptr, col = world["indptr"], world["col"]
    eids = ref.eids_for(indptr, col, B)
    exclude = int(kw.get("exclude_self", True)) | int(kw.get("exclude_edges", True)) << 1
    want = ref.edge_prediction_seeds(indptr, col, eids, k, exclude, kw.get("max_tries", 256), kw.get("base", 0))
    assert B < 63 or ((want["row"] < 0).sum() >= 33 and want["num_seeds"] < (want["ids"] >= 0).sum())      # -1s and repeats
    seeds, num, pos_row, pos_col, neg_col = world["graph"].edge_prediction_seeds(torch.from_numpy(eids).to(DEV), k, **kw)
    torch.cuda.synchronize()
    ctx = f"B {B} k {k} {kw}"
    assert num.shape == (1,) and num.is_cuda and int(num.item()) == want["num_seeds"], ctx
    _eq(seeds, want["seeds"], ctx + " seeds")
    _eq(pos_row, want["pos_row"], ctx + " pos_row")
    _eq(pos_col, want["pos_col"], ctx + " pos_col")
    _eq(neg_col, want["neg_col"], ctx + " neg_col")
    assert seeds.shape == (B * (2 + k),) and pos_row.shape == (B,) and pos_col.shape == (B,) and neg_col.shape == (B, k)
    # the local indices give back the endpoints: seeds[pos_row] is the edge's row, and so on (-1 stays -1)
    row, c = world["graph"].find_edges(eids)
    neg = world["graph"].negative_sample(row, k, **kw)
    padded = torch.cat([seeds, torch.full((1,), -1, dtype=torch.int32, device=DEV)]).long()      # (index -1: the -1 at the end)
    assert torch.equal(padded[pos_row.long()], row.long()) and torch.equal(padded[pos_col.long()], c.long())
    assert torch.equal(padded[neg_col.long()], neg.long())
    _eq(row, want["row"], ctx + " row")
    _eq(c, want["col"], ctx + " col")
    _eq(neg, want["neg"], ctx + " neg")
    U = want["num_seeds"]
    assert bool((seeds[:U] >= 0).all()) and bool((seeds[U:] == -1).all()) and torch.unique(seeds[:U]).numel() == U


def test_no_seed_edges(world):
    seeds, num, pos_row, pos_col, neg_col = world["graph"].edge_prediction_seeds(np.zeros(0, np.int64), 4)
    assert seeds.shape == (0,) and pos_row.shape == (0,) and pos_col.shape == (0,) and neg_col.shape == (0, 4) and int(num.item()) == 0


def test_unsorted_rows_are_refused_only_with_the_edge_exclusion(world):
    rows = np.arange(8, dtype=np.int32)
    with pytest.raises(ValueError, match="sorted"):
        world["unsorted"].negative_sample(rows, 3)
    with pytest.raises(ValueError, match="sorted"):
        world["unsorted"].edge_prediction_seeds(np.arange(8, dtype=np.int64), 3)
    hand = walk_ref.hand_graph()
    got = world["unsorted"].negative_sample(rows, 3, exclude_edges=False, base=5)
    torch.cuda.synchronize()
    _eq(got, ref.negative_sample(hand[0], hand[1], rows, 3, 1, 256, 5), "unsorted graph, exclude_self only")


# ---- another stream, a captured launch --------------------------------------------------------------------------------------------
def test_every_op_on_another_stream(world):
    from legion_amd import engine
    g, indptr, col = world["graph"], world["indptr"], world["col"]
    eids = ref.eids_for(indptr, col, 5000)
    want = ref.edge_prediction_seeds(indptr, col, eids, 5, base=7)
    d_eids = torch.from_numpy(eids).to(DEV)
    d_rows = torch.from_numpy(want["row"]).to(DEV)
    d_ids = torch.from_numpy(want["ids"]).to(DEV)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    assert s != torch.cuda.current_stream()
    row, c = g.find_edges(d_eids, stream=s)
    neg = g.negative_sample(d_rows, 5, base=7, stream=s)
    unique, local, count = engine.unique_ids(d_ids, stream=s)
    host = g.negative_sample(want["row"], 5, base=7, stream=s)        # rows from the host: copied, then sampled on s
    all5 = g.edge_prediction_seeds(d_eids, 5, base=7, stream=s)
    s.synchronize()
    _eq(row, want["row"], "row")
    _eq(c, want["col"], "col")
    _eq(neg, want["neg"], "neg")
    _eq(host, want["neg"], "neg from host rows")
    _eq(unique, want["seeds"], "unique")
    _eq(local, np.concatenate([want["pos_row"], want["pos_col"], want["neg_col"].reshape(-1)]), "local")
    assert int(count.item()) == want["num_seeds"] == int(all5[1].item())
    _eq(all5[0], want["seeds"], "seeds")
    _eq(all5[4], want["neg_col"], "neg_col")


def test_captured_launches_replay_the_eager_results(world):
    L, g = world["L"], world["graph"]
    indptr, col = world["indptr"], world["col"]
    B, k = 257, 5
    eids = ref.eids_for(indptr, col, B)
    want = ref.edge_prediction_seeds(indptr, col, eids, k, base=5)
    m = B * (2 + k)
    d_eids = torch.from_numpy(eids).to(DEV)
    ids = torch.zeros(m, dtype=torch.int32, device=DEV)              # [rows | cols | negatives]: each op writes its part
    unique, local = torch.zeros(m, dtype=torch.int32, device=DEV), torch.zeros(m, dtype=torch.int32, device=DEV)
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    nbytes = int(L.legion_unique_ids_scratch_bytes(m))
    assert nbytes == ref.scratch_bytes(m)
    scratch = torch.zeros(nbytes // 4, dtype=torch.int32, device=DEV)
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + 4 * off)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = [L.legion_find_edges(s, g.handle, P(d_eids), B, P(ids), P(ids, B)),
              L.legion_negative_sample(s, g.handle, P(ids), B, k, 3, 256, 5, P(ids, 2 * B)),
              L.legion_unique_ids(s, P(ids), m, P(unique), P(local), P(count), P(scratch), nbytes)]
    assert rc == [0, 0, 0]
    for _ in range(2):
        for t in (ids, unique, local, count, scratch):
            t.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        _eq(ids, want["ids"], "ids")
        _eq(unique, want["seeds"], "unique")
        _eq(local, np.concatenate([want["pos_row"], want["pos_col"], want["neg_col"].reshape(-1)]), "local")
        assert int(count.item()) == want["num_seeds"]


# ---- the C ABI's refusals ---------------------------------------------------------------------------------------------------------
def test_c_abi_refusals_leave_the_outputs_untouched(world):
    L = world["L"]
    g, bare, unsorted = world["graph"].handle, world["bare"].handle, world["unsorted"].handle
    sorted_of = {g: 1, bare: -1, unsorted: 0}
    n, k = 8, 4
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + 4 * off)
    eids = torch.arange(n, dtype=torch.int64, device=DEV)
    rows = torch.arange(n, dtype=torch.int32, device=DEV)
    out = {name: torch.full((4 * n * k,), SENTINEL, dtype=torch.int32, device=DEV) for name in ("row", "col", "neg", "unique", "local", "count")}
    ids = torch.arange(2 * n * k, dtype=torch.int32, device=DEV)     # (twice the ids of a call: room for the overlap cases)
    m = n * k
    nbytes = int(L.legion_unique_ids_scratch_bytes(m))
    scratch = torch.full((nbytes // 4,), SENTINEL, dtype=torch.int32, device=DEV)

    for change in (dict(graph=None), dict(eids=None), dict(row=None), dict(col=None), dict(n=-1), dict(n=-2 ** 31)):
        a = dict(dict(graph=g, eids=P(eids), n=n, row=P(out["row"]), col=P(out["col"])), **change)
        assert L.legion_find_edges(s, a["graph"], a["eids"], a["n"], a["row"], a["col"]) == -1, change
    assert L.legion_find_edges(s, g, P(eids), 0, P(out["row"]), P(out["col"])) == 0

    ok = dict(graph=g, rows=P(rows), n=n, k=k, exclude=3, tries=256, base=0, neg=P(out["neg"]))
    bad = [dict(graph=None), dict(rows=None), dict(neg=None), dict(n=-1), dict(k=0), dict(k=-1), dict(base=-1), dict(base=M31 - n * k + 1),
           dict(n=2 ** 31 - 1, k=2), dict(base=2 ** 62), dict(exclude=-1), dict(exclude=4), dict(tries=0), dict(tries=257), dict(tries=-1),
           dict(graph=bare), dict(graph=bare, exclude=2), dict(graph=unsorted), dict(graph=unsorted, exclude=2)]
    for change in bad:
        a = dict(ok, **change)
        assert None in (a["graph"], a["rows"], a["neg"]) or \
            ref.negative_refused(a["n"], a["k"], a["exclude"], a["tries"], a["base"], sorted_of[a["graph"]]), change
        assert L.legion_negative_sample(s, a["graph"], a["rows"], a["n"], a["k"], a["exclude"], a["tries"], a["base"], a["neg"]) == -1, change
    assert L.legion_negative_sample(s, g, P(rows), 0, k, 3, 256, 0, P(out["neg"])) == 0                  # no rows: nothing runs

    oku = dict(ids=P(ids), m=m, unique=P(out["unique"]), local=P(out["local"]), count=P(out["count"]), scratch=P(scratch), bytes=nbytes)
    badu = [dict(ids=None), dict(unique=None), dict(local=None), dict(count=None), dict(scratch=None), dict(m=-1), dict(m=2 ** 20 + 1, bytes=2 ** 40),
            dict(bytes=nbytes - 1), dict(bytes=0), dict(bytes=-1), dict(unique=P(ids)), dict(local=P(ids)), dict(count=P(ids)),
            dict(unique=P(ids, m - 1)), dict(local=P(ids, m - 1)), dict(count=P(ids, m - 1))]
    for change in badu:
        a = dict(oku, **change)
        assert L.legion_unique_ids(s, a["ids"], a["m"], a["unique"], a["local"], a["count"], a["scratch"], a["bytes"]) == -1, change
    torch.cuda.synchronize()
    for name, t in out.items():
        assert bool((t == SENTINEL).all()), name
    assert bool((scratch == SENTINEL).all()) and torch.equal(ids, torch.arange(2 * n * k, dtype=torch.int32, device=DEV))

    # the legal edges are taken: the last draw index, one try, the exclusions that do not search on the unchecked and the unsorted graph,
    # outputs that start right behind the ids, no ids at all
    for change in (dict(base=M31 - n * k), dict(tries=1), dict(graph=bare, exclude=0), dict(graph=bare, exclude=1), dict(graph=unsorted, exclude=1)):
        a = dict(ok, **change)
        out["neg"].fill_(SENTINEL)
        assert L.legion_negative_sample(s, a["graph"], a["rows"], n, k, a["exclude"], a["tries"], a["base"], a["neg"]) == 0, change
        torch.cuda.synchronize()
        assert not bool((out["neg"][:n * k] == SENTINEL).any()) and bool((out["neg"][n * k:] == SENTINEL).all()), change
    assert L.legion_unique_ids(s, P(ids), m, P(ids, m), P(out["local"]), P(out["count"]), P(scratch), nbytes) == 0
    torch.cuda.synchronize()
    assert torch.equal(ids[m:], torch.arange(m, dtype=torch.int32, device=DEV)) and int(out["count"][0].item()) == m
    assert L.legion_unique_ids(s, P(ids), 0, P(out["unique"]), P(out["local"]), P(out["count"]), P(scratch), nbytes) == 0
    torch.cuda.synchronize()
    assert int(out["count"][0].item()) == 0 and bool((out["unique"] == SENTINEL).all())
    assert L.legion_graph_check_rows_sorted(bare, s) == 1                                                # checked now: the same call is taken
    assert L.legion_negative_sample(s, bare, P(rows), n, k, 3, 256, 0, P(out["neg"])) == 0
    torch.cuda.synchronize()


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def test_the_seeds_start_a_sampled_batch(world):
    """The U distinct seeds of one call go through the host to FeatureStorage.set_ids; one batch of U with fan-out [3, 2] and edge ids:
    sampled_ids[:U] are the seeds in order -- the local indices address the batch's rows -- and the batch is edge_ids_ref's."""
    indptr, col = world["indptr"], world["col"]
    fanout = [3, 2]
    eids = ref.eids_for(indptr, col, 257)
    seeds, num, pos_row, pos_col, neg_col = world["graph"].edge_prediction_seeds(eids, 5, base=11)
    U = int(num.item())                                                # (through the host)
    want_seeds = ref.edge_prediction_seeds(indptr, col, eids, 5, base=11)
    assert U == want_seeds["num_seeds"] and U > 1000
    ids = seeds[:U].cpu().numpy()
    wl = Workload(dim=4, indptr=indptr, col=col, n_seeds=64, n_valid=8, n_test=8)
    wl.sets[(0, 0)] = (np.ascontiguousarray(ids), np.ascontiguousarray(wl.labels_all[ids]))
    gpu = GpuSide(wl, U, fanout, edge_ids=True)
    try:
        got = gpu.run(0, 0, 0)
        assert np.array_equal(got["sampled_ids"][:U], ids), "the batch's first rows are the seeds, in order"
        rows = got["sampled_ids"]
        pr, pc, nc = (x.cpu().numpy() for x in (pos_row, pos_col, neg_col))
        live = pr >= 0
        assert np.array_equal(rows[pr[live]], want_seeds["row"][live]) and np.array_equal(rows[pc[live]], want_seeds["col"][live])
        assert np.array_equal(rows[nc[nc >= 0]], want_seeds["neg"][nc >= 0])
        want = edge_ids_ref.run_batch(indptr, col, ids, wl.labels_all[ids], U, 0, fanout, True)
        compare_batches(got, want, "link-prediction seeds: ")
        assert np.array_equal(got["agg_edge_ids"], want["agg_edge_ids"])
        edge_ids_ref.check_edge_ids(indptr, col, got)
        assert gpu.pools[0].error() == 0
    finally:
        torch.cuda.synchronize()
        gpu.close()
