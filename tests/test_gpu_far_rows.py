"""Edge offsets beyond 2^31 and 2^32 in every mode: edge ids, sampling without replacement, the prefix table and weighted picks,
rows_sorted, random_walk, node2vec_random_walk, pinsage_neighbors and the neighbour sampler (full CSR, cached topology, graph replay)
bit for bit against the CPU references on the layout of tests/far_rows.py, whose live rows straddle the boundary behind 2^31 or 2^32
entries of ballast that nothing reads.  The references run on the reference view (tests/test_far_rows_cpu.py proves it is the whole
graph's); the column, weight and table arrays of the whole graph exist on the device only.

The same bodies run at three boundaries.  A failure at 5000 is a fault of the harness or of the kernel at any size; a failure at 2^31
but not at 5000 is an offset that went through a signed 32-bit value; a failure at 2^32 only, through an unsigned one.  Every assertion
message ends with that reading (`world["why"]`).  Every test first asserts, from the reference alone, that its inputs do put edge ids on
both sides of the boundary (far_rows.want_*)."""
import ctypes
import time

import numpy as np
import pytest
import torch

from legion_amd import synth
from tests import far_rows
from tests import node2vec_ref
from tests.compare import same_arrays
from tests.helpers import KEYS_EXACT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DIM = 16

@pytest.fixture(scope="module", params=list(far_rows.BOUNDARIES))
def world(hip, request):
    """The whole graph on the device at one boundary, with its weights and table (far_rows.device_world)."""
    with far_rows.device_world(hip, request.param, weights=True) as w:
        yield w


# ---- the table ----------------------------------------------------------------------------------------------------------------------
def test_table(world):
    g, why = world["g"], world["why"]
    cdf = world["graph"].edge_cdf()
    assert cdf.shape == (g.E,)
    got = cdf[g.offset:].cpu().numpy()
    bad = np.nonzero(got.view(np.uint32) != g.table_ref.view(np.uint32))[0]
    assert bad.size == 0, f"{bad.size} entries of the live table differ, first at live position {bad[:5]}" + why
    ramp = torch.arange(1, g.L + 1, dtype=torch.float32, device=DEV)                 # exact: L < 2^24
    for row in (0, (g.B - 1) // 2, g.B - 2):                                        # the first, a middle and the last full ballast row
        assert g.deg[row] == g.L
        s = int(g.indptr[row])
        assert torch.equal(cdf[s:s + g.L], ramp), f"the table of ballast row {row}" + why
    s, d = int(g.indptr[g.B - 1]), int(g.deg[g.B - 1])                              # ... and the shortened one
    assert torch.equal(cdf[s:s + d], ramp[:d]), "the table of the last ballast row" + why


def test_weighted_picks(world):
    """legion_draw_weighted_batch with row_start values beyond the boundary, the straddling row included."""
    g, hip = world["g"], world["L"]
    idx, row_start, deg, want = g.want_picks()
    t_idx, t_rs, t_d = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (idx, row_start, deg))
    out = torch.full((idx.size,), -7, dtype=torch.int32, device=DEV)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    hip.legion_draw_weighted_batch(s, ctypes.c_void_p(t_idx.data_ptr()), ctypes.c_void_p(t_rs.data_ptr()), ctypes.c_void_p(t_d.data_ptr()),
                                   ctypes.c_void_p(world["graph"].edge_cdf().data_ptr()), ctypes.c_void_p(out.data_ptr()), idx.size)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got, want), f"{int((got != want).sum())} picks differ" + world["why"]


# ---- rows_sorted --------------------------------------------------------------------------------------------------------------------
def test_rows_sorted(world):
    """True on the graph; False with one adjacent pair swapped inside a live row that starts beyond the boundary; True when the only
    decreasing pair of the whole array lies across a row boundary beyond it."""
    from legion_amd import engine
    g, why = world["g"], world["why"]
    t0 = time.perf_counter()
    assert world["graph"].rows_sorted() is True, "the graph's rows are sorted" + why
    print(f"\ninversion count at {world['name']}: {time.perf_counter() - t0:.3f} s")
    live = g.col_ref
    starts = g.indptr_ref[g.B:-1]
    across = starts[(np.diff(g.indptr_ref[g.B:]) > 0) & (starts > g.k) & (starts < live.size)]      # row boundaries beyond the boundary
    assert (live[across - 1] > live[across]).sum() >= 10              # the graph itself decreases across many of them
    row = next(v for v in range(g.hub + 1, g.node_num) if g.deg[v] >= 4)
    at = next(e for e in range(int(g.indptr_ref[row]), int(g.indptr_ref[row + 1]) - 1) if 0 <= live[e] < live[e + 1])
    assert g.indptr[row] > g.boundary
    swapped = live.copy()
    swapped[at], swapped[at + 1] = live[at + 1], live[at]
    edge = int(across[across.size // 2])
    flat = np.full(live.size, g.B, dtype=np.int32)                    # every live entry the same vertex, but the last of one row
    flat[edge - 1] = g.B + 1
    down = np.nonzero(np.concatenate([[0], flat])[:-1] > flat)[0]
    assert down.tolist() == [edge] and edge + g.offset > g.boundary   # the whole array's only decreasing pair, across a row boundary
    c2 = world["col"].clone()
    for name, changed, want in (("one pair swapped inside a row", swapped, False), ("the only decreasing pair across a row boundary", flat, True)):
        assert node2vec_ref.rows_sorted(g.indptr_ref, changed) is want, name
        c2[g.offset:] = torch.from_numpy(changed).to(DEV)
        other = engine.GraphStorage(1, world["indptr"], c2)
        try:
            assert other.rows_sorted() is want, f"rows_sorted with {name}" + why
        finally:
            torch.cuda.synchronize()
            other.close()
    del c2


# ---- the walks ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", far_rows.WALK_CASES, ids=lambda c: "-".join(map(str, c)))
def test_random_walk(world, case):
    g = world["g"]
    count, length, weighted, restart = case
    reads = {}
    want = g.want_walk(*case, reads=reads)
    g.assert_no_ballast_read(reads, view=True)
    seeds = torch.from_numpy(g.seeds(count)).to(DEV)
    got = world["graph"].random_walk(seeds, length, weighted=weighted, restart_prob=restart, return_eids=True)
    only = world["graph"].random_walk(seeds, length, weighted=weighted, restart_prob=restart)
    torch.cuda.synchronize()
    same_arrays(got, want, f"random_walk {case}" + world["why"])
    assert torch.equal(only, got[0]), f"random_walk {case}: traces without edge ids" + world["why"]


@pytest.mark.parametrize("case", far_rows.NODE2VEC_CASES, ids=lambda c: "-".join(map(str, c)))
def test_node2vec(world, case):
    g = world["g"]
    count, length, p, q, weighted, tries = case
    reads = {}
    want = g.want_node2vec(*case, reads=reads)
    g.assert_no_ballast_read(reads, view=True)
    seeds = torch.from_numpy(g.seeds(count)).to(DEV)
    got = world["graph"].node2vec_random_walk(seeds, p, q, length, weighted=weighted, return_eids=True, max_tries=tries)
    torch.cuda.synchronize()
    same_arrays(got, want, f"node2vec {case}" + world["why"])


@pytest.mark.parametrize("case", far_rows.PINSAGE_CASES, ids=lambda c: "-".join(map(str, c)))
def test_pinsage(world, case):
    g = world["g"]
    count, R, T, k, weighted, termination = case
    reads = {}
    want = g.want_pinsage(*case, reads=reads)
    g.assert_no_ballast_read(reads, view=True)
    got = world["graph"].pinsage_neighbors(torch.from_numpy(g.seeds(count)).to(DEV), R, T, k, termination_prob=termination, weighted=weighted)
    torch.cuda.synchronize()
    same_arrays(got, want, f"pinsage {case}" + world["why"])


# ---- the neighbour sampler ----------------------------------------------------------------------------------------------------------
class _Sampler:
    """A graph of its own over the world's arrays (a topology cache rewrites a graph's row headers), a small feature table over
    B + n vertices, a cache and one pool in `mode` with edge ids."""

    def __init__(self, world, mode, fanout, cache_memory):
        from legion_amd import engine
        g = world["g"]
        self.g, self.mode, self.fanout, self.batch = g, mode, list(fanout), far_rows.SAMPLER_BATCH
        self.kw = dict(replace=mode != "distinct", edge_ids=True, weighted=mode == "weighted")
        self.graph = engine.GraphStorage(1, world["indptr"], world["col"])
        if mode == "weighted":
            self.graph.set_edge_weights(world["w"])
        self.table = synth.features_numpy(0, g.node_num, DIM, 7)
        self.features = torch.from_numpy(self.table).to(DEV)
        self.feature = engine.FeatureStorage(1, self.features)
        self.feature.set_ids(0, 0, *g.train_ids())
        self.n_batches = -(-g.n // self.batch)
        self.cache = engine.UnifiedCache(cache_memory, DIM, self.n_batches, 1, g.node_num)
        self.cache.init_controller(0)
        self.pool = engine.MemoryPool(0, g.node_num, self.batch, self.fanout, DIM, **self.kw)
        self.pool.alloc_features(self.pool.num_ids)
        torch.cuda.synchronize()

    def run(self, it, is_presc=False):
        from legion_amd import engine
        engine.enqueue_batch(None, self.graph, self.feature, self.cache, self.pool, self.batch, it, 0, 0, is_presc, self.fanout)
        torch.cuda.synchronize()
        return engine.read_batch(self.pool)

    def check(self, got, want, ctx):
        for key in KEYS_EXACT + ["agg_edge_ids"]:
            a, b = got[key], want[key]
            assert a.dtype == b.dtype and a.shape == b.shape, f"{ctx}{key}: {a.dtype} {a.shape} != {b.dtype} {b.shape}"
            bad = np.nonzero(a != b)[0]
            assert bad.size == 0, f"{ctx}{key}: {bad.size} mismatches, first at {bad[0]}: got {a[bad[0]]} want {b[bad[0]]}"
        rows = got["float_features"][:want["sampled_ids"].size]
        assert np.array_equal(rows.view(np.uint32), self.table[want["sampled_ids"]].view(np.uint32)), f"{ctx}gathered rows"

    def close(self):
        torch.cuda.synchronize()
        self.pool.close()
        self.cache.close()
        self.feature.close()
        self.graph.close()


@pytest.mark.parametrize("fanout", far_rows.SAMPLER_SHAPES, ids=lambda f: "x".join(map(str, f)))
@pytest.mark.parametrize("mode", far_rows.SAMPLER_MODES)
def test_neighbour_sampler(world, monkeypatch, mode, fanout):
    """Batches from the full CSR; the same batches after a PreSC epoch, the cost model and a fill with a topology cache and no column
    slots, with topology hits on rows whose full-CSR start lies beyond the boundary; then one lane group under graph replay."""
    from legion_amd import engine
    monkeypatch.setenv("LEGION_COL_SLOTS", "0")
    g, why = world["g"], world["why"]
    sm = _Sampler(world, mode, fanout, cache_memory=64 << 10)
    try:
        its = (0, 1, sm.n_batches - 1)
        want = {it: g.want_batch(mode, it, sm.batch, fanout) for it in its}
        for it in its:
            sm.check(sm.run(it), want[it], f"{mode} {fanout} batch {it} from the full CSR: ")
        assert sm.pool.error() == 0
        for it in range(sm.n_batches):
            sm.run(it, is_presc=True)
        tx = sm.cache.topo_transactions(0)
        sm.cache.candidate_selection(0, sm.graph)
        sm.cache.cost_model(sm.feature, sm.graph, (tx, 0), sm.n_batches)
        sm.cache.fill_up(sm.feature, sm.graph)
        assert sm.cache.edge_capacity(0) > 0 and sm.graph.column_slots(0) is False
        hits = 0
        for it in its:
            sm.check(sm.run(it), want[it], f"{mode} {fanout} batch {it} with a cached topology: ")
            ec, H = want[it]["edge_counter"], len(fanout)
            frontier = want[it]["agg_src_ids"][int(ec[9 + H - 2]):int(ec[9 + H - 1])].astype(np.int64)      # the last hop's
            tp = sm.pool.buffer("tmp_part_ind")[:frontier.size].cpu().numpy()
            hits += int(((tp >= 0) & (g.indptr[frontier] > g.boundary)).sum())
        print(f"\n{mode} {fanout} at {world['name']}: topology capacity {sm.cache.edge_capacity(0)}, {hits} last-hop hits beyond the boundary")
        assert hits > 0, "no topology hit on a row that starts beyond the boundary"
        assert sm.pool.error() == 0
        pipe = engine.Pipeline(sm.graph, sm.feature, sm.cache, 0, sm.batch, fanout, 2, sm.pool.num_ids, True, 2, **sm.kw)
        try:
            for rep in range(3):                                    # slot 0 twice: its graph is replayed
                sl = pipe.submit(0, 0)
                pipe.wait(sl)
                for lane in (0, 1):
                    sm.check(engine.read_batch(pipe.pools[sl][lane]), want[lane], f"{mode} {fanout} replay {rep} lane {lane}: ")
            assert all(pool.error() == 0 for lanes in pipe.pools for pool in lanes)
        finally:
            pipe.close()
    except AssertionError as e:
        raise AssertionError(str(e) + why) from e
    finally:
        sm.close()
