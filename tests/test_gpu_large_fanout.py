"""Large fan-outs in both sampling modes, bit for bit against the references.

Without replacement (fan-outs 41..256, LEGION_DISTINCT_MAX_FANOUT): the picks of legion_draw_distinct_batch, whole batches of
every bucket class, lane groups and the server binary against tests/distinct_ref.py, and the cap at 256 at every entry point.
With replacement (fan-outs around and beyond LG_SUPER = 1024 slots, one workgroup's super tile): whole batches, PreSC's hotness
and topology transactions and the caches built from them against the oracle -- where one entry covers a whole super tile.
The graphs are built here, not by RMAT, so that the degrees around f are under control.  Wide feature rows: see the end."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from legion_amd import engine, synth
from oracle import ffi
from tests import distinct_ref as ref
from tests.gpu_harness import CpuSide, GpuSide
from tests.helpers import Workload, compare_batches
from tests.test_gpu_pipeline import expected_topo_transactions

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUPER = 1024                       # LG_SUPER: slots of one super tile
CAP = 256                          # LEGION_DISTINCT_MAX_FANOUT
SMALL, MEDIUM = 1 << 19, 1 << 22   # LG_LDS_SLOTS_SMALL / _MEDIUM: the bucket classes by slots (no PreSC hint)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- graphs and workloads ----------------------------------------------------------------------------------------------------
def csr_with_degrees(deg, seed):
    """CSR over N = deg.size vertices (a power of two) whose row v has deg[v] DISTINCT neighbours: (o_v + i * s_v) mod N, s_v odd."""
    N = deg.size
    assert N & (N - 1) == 0 and deg.max() <= N
    rng = np.random.RandomState(seed)
    indptr = np.zeros(N + 1, np.int64)
    np.cumsum(deg, out=indptr[1:])
    row = np.repeat(np.arange(N, dtype=np.int64), deg)
    pos = np.arange(indptr[-1], dtype=np.int64) - indptr[row]
    o = rng.randint(0, N, size=N).astype(np.int64)
    s = rng.randint(0, N // 2, size=N).astype(np.int64) * 2 + 1
    col = ((o[row] + pos * s[row]) % N).astype(np.int32)
    return indptr, col


class Wl:
    """What GpuSide / CpuSide read of a tests.helpers.Workload, over a given graph and given seed lists (one partition)."""

    def __init__(self, indptr, col, train, valid, test, dim):
        self.indptr, self.col = indptr, col
        self.N, self.E, self.D, self.P = int(indptr.size - 1), int(col.size), dim, 1
        self.features = synth.features_numpy(0, self.N, dim, 7) if dim > 0 else None
        labels = (np.arange(self.N, dtype=np.int64) * 2654435761 % 47).astype(np.int32)
        self.sets = {(0, m): (np.ascontiguousarray(s, dtype=np.int32), np.ascontiguousarray(labels[s]))
                     for m, s in enumerate((train, valid, test))}


def distinct_graph(f, N=8192, seed=1):
    """Rows of degree 0, 1, f-1, f, f+1, 3f and a few thousand, in random vertex order."""
    rng = np.random.RandomState(seed + f)
    classes = np.array([0, 1, f - 1, f, f + 1, 3 * f, 0], np.int64)
    deg = classes[np.arange(N) % classes.size]
    few_k = np.arange(N) % classes.size == classes.size - 1
    deg[few_k] = np.minimum(rng.randint(2000, 4000, size=int(few_k.sum())), N)
    deg = deg[rng.permutation(N)]
    return csr_with_degrees(deg, seed)


def replace_graph(N=4096, seed=2):
    """Hubs (2000..20000 neighbours), rows of degree 1..5, rows of degree 0 and some in between."""
    rng = np.random.RandomState(seed)
    deg = rng.randint(1, 6, size=N).astype(np.int64)
    v = rng.permutation(N)
    deg[v[:40]] = rng.randint(2000, 20000, size=40)
    deg[v[40:200]] = rng.randint(50, 600, size=160)
    deg[v[200:1000]] = 0
    return csr_with_degrees(np.minimum(deg, N), seed)


def seed_sets(N, n_train, n_valid=300, n_test=200, seed=11):
    perm = np.random.RandomState(seed).permutation(N).astype(np.int32)
    return perm[:n_train], perm[n_train:n_train + n_valid], perm[n_train + n_valid:n_train + n_valid + n_test]


def bucket_class(batch, fanout):
    slots = batch * int(np.prod(fanout))
    return "small" if slots <= SMALL else "medium" if slots <= MEDIUM else "large"


def assert_class(pool, cls):
    want = {"small": (8, 16), "medium": (64,), "large": (256,)}[cls]
    assert pool.lds_buckets() in want, f"{pool.lds_buckets()} buckets, want the {cls} class"


def hop_frontiers(batch):
    """(fan-out index h, frontier ids) of every hop of a batch in the reader's layout."""
    nc, ec = batch["node_counter"], batch["edge_counter"]
    out = []
    for h in range(int(batch["hop_num"])):
        out.append(batch["sampled_ids"][:int(nc[9])] if h == 0 else batch["agg_src_ids"][int(ec[9 + h - 1]):int(ec[9 + h])])
    return out


def straddlers(frontier, deg, f):
    """Entries with D > f whose f slots cross a super-tile boundary, and entries with D > f that end a super tile."""
    q = np.nonzero(deg[np.maximum(frontier, 0)] * (frontier >= 0) > f)[0].astype(np.int64)
    first, last = q * f, q * f + f - 1
    return int((first // SUPER != last // SUPER).sum()), int(((last + 1) % SUPER == 0).sum())


def check_distinct_edges(wl, got, fanout):
    """Independent of distinct_ref: hop by hop, frontier entry q has exactly min(f, D) edges, all to q's vertex, to distinct
    neighbours that are in q's row."""
    deg = np.diff(wl.indptr)
    ec = got["edge_counter"]
    for h, fr in enumerate(hop_frontiers(got)):
        f = fanout[h]
        d = np.where(fr >= 0, deg[np.maximum(fr, 0)], 0)
        n = np.minimum(d, f)
        lo, hi = int(ec[9 + h]), int(ec[9 + h + 1])
        assert hi - lo == int(n.sum()), f"hop {h}: {hi - lo} edges, want {int(n.sum())}"
        q = np.repeat(np.arange(fr.size), n)
        src, dst = got["agg_src_ids"][lo:hi].astype(np.int64), got["agg_dst_ids"][lo:hi]
        assert np.array_equal(dst, fr[q]), f"hop {h}: edges out of slot order"
        key = np.sort(q * wl.N + src)
        assert np.all(np.diff(key) > 0), f"hop {h}: a frontier entry has a repeated neighbour"
        v = fr[q].astype(np.int64)
        for i in np.random.RandomState(h).choice(src.size, min(src.size, 500), replace=False):
            assert src[i] in wl.col[wl.indptr[v[i]]:wl.indptr[v[i] + 1]], f"hop {h}: a neighbour that is not in its row"


# ---- a. the picks without replacement --------------------------------------------------------------------------------------
def check_pick_properties(P, D, f):
    """Every row: min(f, D) non-negative picks first, distinct, in [0, D); 0..D-1 in order for D <= f; -1 after them."""
    for i in range(P.shape[0]):
        n = min(f, int(D[i]))
        row = P[i]
        assert np.all(row[n:] == -1), f"row {i} (D {D[i]}): a pick past min(f, D)"
        p = row[:n].astype(np.int64)
        assert np.all((p >= 0) & (p < int(D[i]))), f"row {i} (D {D[i]}): a pick outside [0, D)"
        assert np.unique(p).size == n, f"row {i} (D {D[i]}): repeated picks"
        if D[i] <= f:
            assert np.array_equal(p, np.arange(n)), f"row {i} (D {D[i]}): not every neighbour in CSR order"


@pytest.mark.parametrize("f", [41, 64, 100, 127, 128, 129, 200, 255, 256])
def test_distinct_picks_at_large_fanouts(hip, f):
    from legion_amd import lib
    L = lib.load()
    D = np.array([0, 1, f - 1, f, f + 1, 2 * f, 1000, 10**6, 2**31 - 1] * 24, dtype=np.int64)
    base = (np.arange(D.size, dtype=np.int64) * f + 4_000_000).astype(np.int32)
    dev = torch.device("cuda:0")
    tb, td = torch.from_numpy(base).to(dev), torch.from_numpy(D.astype(np.int32)).to(dev)
    out = torch.full((D.size * f,), -7, dtype=torch.int32, device=dev)
    assert L.legion_draw_distinct_batch(_stream(), _p(tb), _p(td), f, _p(out), D.size) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(D.size, f)
    check_pick_properties(got, D, f)
    assert np.array_equal(got, ref.picks(base, D, f))


@pytest.mark.parametrize("f", [0, CAP + 1])
def test_distinct_picks_refuse_fanouts_outside_the_cap(hip, f):
    from legion_amd import lib
    L = lib.load()
    n = 50
    dev = torch.device("cuda:0")
    tb = torch.arange(n, dtype=torch.int32, device=dev) * 300
    td = torch.full((n,), 5000, dtype=torch.int32, device=dev)
    out = torch.full((n * (CAP + 1),), -7, dtype=torch.int32, device=dev)
    assert L.legion_draw_distinct_batch(_stream(), _p(tb), _p(td), f, _p(out), n) == -1
    torch.cuda.synchronize()
    assert bool((out == -7).all())                      # nothing launched


# ---- b. whole batches without replacement -----------------------------------------------------------------------------------
def _distinct_want(wl, it, mode, batch, fanout):
    ids, labels = wl.sets[(0, mode)]
    return ref.run_batch(wl.indptr, wl.col, ids, labels, batch, it, fanout)


def _compare_rows(got, want, wl, ctx):
    compare_batches(got, want, ctx)
    rows = got["float_features"][:want["sampled_ids"].size]
    assert np.array_equal(rows.view(np.uint32), wl.features[want["sampled_ids"]].view(np.uint32)), f"{ctx}gathered rows"


DISTINCT_CASES = [([256], 300), ([256], 3000), ([255], 300), ([255], 2500), ([200, 2], 500), ([200, 2], 2000),
                  ([129, 3], 1200), ([64, 64], 1040)]


@pytest.mark.parametrize("fanout,batch", DISTINCT_CASES, ids=[f"{'x'.join(map(str, f))}-B{b}-{bucket_class(b, f)}" for f, b in DISTINCT_CASES])
def test_distinct_batches_at_large_fanouts(hip, fanout, batch):
    """Every mode and the clamped last batch against distinct_ref, plus the edge counts and distinctness on their own.  Coverage:
    in each hop of f > 40, entries with D > f cross super-tile boundaries (f not dividing 1024: the first entry's thread redraws
    its slots of the previous super tile) or end one (f dividing 1024: s_pick used to the tile's last word)."""
    f_big = max(fanout)
    indptr, col = distinct_graph(f_big)
    n_train = batch * 2 + batch // 3 + 1                  # two full batches and a clamped one
    wl = Wl(indptr, col, *seed_sets(indptr.size - 1, n_train), dim=8)
    gpu = GpuSide(wl, batch, fanout)
    pool = gpu.pools[0]
    pool.set_replace(False)
    assert_class(pool, bucket_class(batch, fanout))
    deg = np.diff(indptr)
    cross = ends = 0
    runs = [(0, 0), (2, 0), (0, 1), (0, 2)]               # train 0, the clamped last one, valid, test
    if bucket_class(batch, fanout) != "large":
        runs.insert(1, (1, 0))
    for it, mode in runs:
        got = gpu.run(0, it, mode)
        want = _distinct_want(wl, it, mode, batch, fanout)
        _compare_rows(got, want, wl, f"{fanout} B {batch} mode {mode} batch {it}: ")
        check_distinct_edges(wl, got, fanout)
        if mode == 0 and it == 2:
            assert 0 < want["labels"].size < batch          # (the clamped batch)
        for h, fr in enumerate(hop_frontiers(want)):
            if fanout[h] > 40:
                c, e = straddlers(fr, deg, fanout[h])
                cross += c
                ends += e
    assert pool.error() == 0
    if any(f > 40 and SUPER % f for f in fanout):
        assert cross > 0, "no entry with D > f crossed a super-tile boundary"
    else:
        assert ends > 0, "no entry with D > f ended a super tile"
    gpu.close()


# ---- c. whole batches with replacement -------------------------------------------------------------------------------------
REPLACE_CASES = [([300], 1), ([300], 7), ([1023], 7), ([1024], 1), ([1024], 7), ([1025], 7), ([3000], 1), ([3000], 7),
                 ([2, 1500], 7), ([1100, 2], 7),
                 ([1025], 1000), ([3000], 300), ([2, 1500], 300),
                 ([3000], 1500), ([1100, 2], 2000)]


def replace_workload(batch, dim=8):
    indptr, col = replace_graph()
    return Wl(indptr, col, *seed_sets(indptr.size - 1, max(300, batch * 2 + batch // 3 + 1)), dim=dim)


def continued_tiles(frontier, f):
    """Super tiles that begin inside a real entry's slots (the entry began in an earlier tile: PreSC does not count it again)."""
    q = np.nonzero(frontier >= 0)[0].astype(np.int64)
    return int(((q * f + f - 1) // SUPER - (q * f) // SUPER).sum())


def covered_tiles(frontier, f):
    """Super tiles that lie inside one real entry's slots and hold no entry's first slot (PreSC counts no row in them)."""
    q = np.nonzero(frontier >= 0)[0].astype(np.int64)
    first = q * f // SUPER + 1                         # tiles starting in (q*f, q*f + f - SUPER]
    last = (q * f + f - SUPER) // SUPER
    return int(np.maximum(last - first + 1, 0).sum())


@pytest.mark.parametrize("fanout,batch", REPLACE_CASES, ids=[f"{'x'.join(map(str, f))}-B{b}-{bucket_class(b, f)}" for f, b in REPLACE_CASES])
def test_replace_batches_at_super_tile_fanouts(hip, fanout, batch):
    wl = replace_workload(batch)
    rows = wl.N + batch
    gpu, cpu = GpuSide(wl, batch, fanout, feature_rows=rows), CpuSide(wl, batch, fanout, feature_rows=rows)
    assert_class(gpu.pools[0], bucket_class(batch, fanout))
    n_train = wl.sets[(0, 0)][0].size
    last = (n_train + batch - 1) // batch - 1
    for it, mode in [(0, 0), (1, 0), (last, 0), (0, 1), (0, 2)]:
        compare_batches(gpu.run(0, it, mode), cpu.run(0, it, mode), f"{fanout} B {batch} mode {mode} batch {it}: ")
    assert gpu.pools[0].error() == 0
    gpu.close(); cpu.close()


@pytest.mark.parametrize("fanout,batch", [([1025], 7), ([3000], 7), ([2, 1500], 7), ([1100, 2], 1)])
def test_replace_presc_then_topology_cache(hip, col_slots, fanout, batch):
    """PreSC over an epoch at fan-outs where one entry spans whole super tiles: the hotness arrays and the topology
    transactions (counted in the tile of a row's first slot only) equal the oracle's; then a cache with a topology share serves
    the oracle's batches and the last hop's topology hit mask (tmp_part_ind, rewritten by every tile of a spanning entry)."""
    wl = replace_workload(batch)
    rows = wl.N + batch
    gpu, cpu = GpuSide(wl, batch, fanout, cache_memory=600_000, feature_rows=rows), CpuSide(wl, batch, fanout, feature_rows=rows)
    n_train = wl.sets[(0, 0)][0].size
    steps = (n_train + batch - 1) // batch
    want_tx, continued, covered = 0, 0, 0
    for it in range(steps):
        g, c = gpu.run(0, it, 0, is_presc=True), cpu.run(0, it, 0, is_presc=True)
        compare_batches(g, c, f"presc {it}: ")
        want_tx += expected_topo_transactions(wl, c, fanout)
        for h, fr in enumerate(hop_frontiers(c)):
            if fanout[h] > SUPER:
                continued += continued_tiles(fr, fanout[h])
                covered += covered_tiles(fr, fanout[h])
    assert continued > 0, "no super tile began inside an entry"
    if max(fanout) >= 2 * SUPER:
        assert covered > 0, "no super tile lay inside one entry"
    assert gpu.cache.topo_transactions(0) == want_tx
    assert np.array_equal(gpu.cache.array("node_access_time", 0).cpu().numpy().view(np.uint64), cpu.node_access[0])
    assert np.array_equal(gpu.cache.array("edge_access_time", 0).cpu().numpy().view(np.uint64), cpu.edge_access[0])
    capacity = (wl.N // 4, 60)
    gpu.cache.candidate_selection(0, gpu.graph)
    gpu.cache.set_capacity(*capacity)
    gpu.cache.fill_up(gpu.feature, gpu.graph)
    assert gpu.graph.column_slots(0) == col_slots
    cpu.build_cache(0, capacity=capacity)
    H = len(fanout)
    topo = 0
    for it in range(min(steps, 3)):
        g, c = gpu.run(0, it, 0), cpu.run(0, it, 0)
        compare_batches(g, c, f"cached topology {it}: ")
        assert np.array_equal(g["cache_search_buffer"], c["cache_search_buffer"])
        n_f = int(g["edge_counter"][9 + H - 1] - g["edge_counter"][9 + H - 2]) if H > 1 else int(g["node_counter"][9])
        tp_g = gpu.pools[0].buffer("tmp_part_ind")[:n_f].cpu().numpy()
        tp_c = np.ctypeslib.as_array(cpu.pools[0].p.contents.tmp_part_ind, shape=(max(n_f, 1),))[:n_f]
        assert np.array_equal(tp_g, tp_c), f"tmp_part_ind batch {it}"
        topo += int((tp_g >= 0).sum())
    assert topo > 0                                      # some rows came from the cached topology
    assert gpu.pools[0].error() == 0
    gpu.close(); cpu.close()


# ---- d. lane groups ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph,weave", [(True, False), (True, True)], ids=["graph", "weave"])
def test_pipeline_distinct_at_the_cap(hip, use_graph, weave):
    fanout, batch, group = [CAP], 64, 3
    indptr, col = distinct_graph(CAP, N=4096)
    wl = Wl(indptr, col, *seed_sets(indptr.size - 1, batch * group * 2 + 20), dim=16)
    gpu = GpuSide(wl, batch, fanout)
    pipe = engine.Pipeline(gpu.graph, gpu.feature, gpu.cache, 0, batch, fanout, group, gpu.pools[0].num_ids, use_graph, 2,
                           weave=weave, replace=False)
    n_batches = (wl.sets[(0, 0)][0].size + batch - 1) // batch
    for gi in range((n_batches + group - 1) // group):
        sl = pipe.submit(gi * group, 0)
        pipe.wait(sl)
        for lane in range(group):
            got = engine.read_batch(pipe.pools[sl][lane])
            _compare_rows(got, _distinct_want(wl, gi * group + lane, 0, batch, fanout), wl, f"group {gi} lane {lane}: ")
            assert pipe.pools[sl][lane].error() == 0
    pipe.close()
    gpu.close()


@pytest.mark.parametrize("use_graph,weave", [(True, False), (True, True)], ids=["graph", "weave"])
def test_pipeline_replace_past_a_super_tile(hip, use_graph, weave):
    fanout, batch, group = [1025], 7, 3
    wl = replace_workload(batch, dim=16)
    gpu, cpu = GpuSide(wl, batch, fanout), CpuSide(wl, batch, fanout)
    pipe = engine.Pipeline(gpu.graph, gpu.feature, gpu.cache, 0, batch, fanout, group, gpu.pools[0].num_ids, use_graph, 2,
                           weave=weave)
    for gi in range(3):
        sl = pipe.submit(gi * group, 0)
        pipe.wait(sl)
        for lane in range(group):
            compare_batches(engine.read_batch(pipe.pools[sl][lane]), cpu.run(0, gi * group + lane, 0), f"group {gi} lane {lane}: ")
            assert pipe.pools[sl][lane].error() == 0
    pipe.close()
    gpu.close(); cpu.close()


# ---- e. the cap at every entry point ---------------------------------------------------------------------------------------
def test_pool_and_pipeline_accept_256_and_refuse_257(hip):
    wl = Workload(scale=10, edge_factor=8, dim=4, n_seeds=200)
    gpu = GpuSide(wl, 8, [4])
    ok = engine.MemoryPool(0, wl.N, 4, [CAP], wl.D, replace=False)
    assert ok.replace is False
    ok.close()
    ok = engine.MemoryPool(0, wl.N, 4, [3, CAP], wl.D)
    ok.set_replace(False)
    ok.close()
    with pytest.raises(RuntimeError):
        engine.MemoryPool(0, wl.N, 4, [CAP + 1], wl.D, replace=False)
    big = engine.MemoryPool(0, wl.N, 4, [3, CAP + 1], wl.D)
    with pytest.raises(RuntimeError):
        big.set_replace(False)
    assert big.replace is True
    big.close()
    pipe = engine.Pipeline(gpu.graph, gpu.feature, gpu.cache, 0, 4, [CAP], 2, 4 + 4 * CAP, True, 2, replace=False)
    pipe.close()
    with pytest.raises(RuntimeError):
        engine.Pipeline(gpu.graph, gpu.feature, gpu.cache, 0, 4, [CAP + 1], 2, 4 + 4 * (CAP + 1), True, 2, replace=False)
    gpu.close()


def test_enqueued_hop_above_the_cap_is_refused(hip):
    """A replace=False pool sized for [256] that is enqueued with a 257 hop: error bit 8, the hop is not sampled (no edge), the
    seeds are untouched."""
    indptr, col = distinct_graph(CAP, N=4096)
    wl = Wl(indptr, col, *seed_sets(indptr.size - 1, 200), dim=8)
    batch = 16
    gpu = GpuSide(wl, batch, [CAP])
    pool = gpu.pools[0]
    pool.set_replace(False)
    engine.enqueue_batch(None, gpu.graph, gpu.feature, gpu.cache, pool, batch, 0, 0, 0, False, [CAP + 1])
    torch.cuda.synchronize()
    assert pool.error() & 8
    ec = pool.buffer("edge_counter").cpu().numpy()
    assert not ec.any(), f"edge counters {ec.tolist()}"
    assert np.array_equal(pool.buffer("sampled_ids")[:batch].cpu().numpy(), wl.sets[(0, 0)][0][:batch])
    gpu.close()


def _server_dataset(tmp_path, f, D=24):
    from tests.test_gpu_boundary import write_dataset
    indptr, col = distinct_graph(f, N=2048)
    N = indptr.size - 1
    feats = synth.features_numpy(0, N, D, 7)
    labels = (np.arange(N) % 47).astype(np.int32)
    train, valid, test = seed_sets(N, 300, 60, 40, seed=3)
    ds = str(tmp_path / "ds") + "/"
    write_dataset(ds, indptr, col, feats, labels, train, valid, test)
    return ds, indptr, col, feats, labels, (train, valid, test)


def _meta(work, ds, B, N, E, D, sets, epoch):
    work.mkdir()
    fields = [ds, B, N, E, D, sets[0].size, sets[1].size, sets[2].size, 60_000, epoch]
    (work / "meta_config").write_text(" ".join(str(f) for f in fields))


def test_server_binary_without_replacement_at_the_cap(hip, tmp_path, monkeypatch):
    """sampling_server --sample-replace 0 at fan-out 256 against tests/fake_trainer.py: every batch equals distinct_ref's."""
    from tests.server_proc import start_server
    D, B, epoch, fanout = 24, 48, 1, [CAP]
    ds, indptr, col, feats, labels, sets = _server_dataset(tmp_path, CAP, D)
    work = tmp_path / "run"
    _meta(work, ds, B, indptr.size - 1, col.size, D, sets, epoch)
    ns = f"_lf{os.getpid()}"
    monkeypatch.setenv("LEGION_IPC_NAMESPACE", ns)
    env = dict(os.environ)
    argv = [os.path.join(ROOT, "legion_amd", "bin", "sampling_server"), "1", "0", str(CAP), "--sample-replace", "0"]
    server, log = start_server(argv, work, env, work / "server.log")
    try:
        st = ffi.Steps()
        L = ffi.load()
        one = lambda v: (ctypes.c_int32 * 1)(v)
        L.lgo_coordinate(ctypes.byref(st), 1, one(sets[0].size), one(sets[1].size), one(sets[2].size), B, epoch)
        out_npz = tmp_path / "trainer.npz"
        tr = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fake_trainer.py"), "0", str(D), str(epoch), str(out_npz)],
                            env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, stdin=subprocess.DEVNULL, text=True,
                            timeout=300)
        assert tr.returncode == 0, tr.stdout[-3000:] + "\n---- server ----\n" + open(work / "server.log").read()[-2000:]
        got = np.load(out_npz)
        assert got["steps"].tolist() == [st.train_step, st.valid_step, st.test_step]
        for gb in range(L.lgo_max_step(ctypes.byref(st))):
            mode = L.lgo_current_mode(ctypes.byref(st), gb)
            it = L.lgo_local_batch_id(ctypes.byref(st), gb)
            bs = L.lgo_current_batchsize(ctypes.byref(st), 0, mode)
            want = ref.run_batch(indptr, col, sets[mode], labels[sets[mode]], bs, it, fanout)
            n_e = int(want["edge_counter"][10])
            assert np.array_equal(got[f"b{gb}_ids"], want["sampled_ids"]), f"batch {gb} mode {mode}"
            assert np.array_equal(got[f"b{gb}_labels"], want["labels"]), f"batch {gb}"
            assert np.array_equal(got[f"b{gb}_feats"], feats[want["sampled_ids"]].view(np.uint32)), f"batch {gb} rows"
            assert np.array_equal(got[f"b{gb}_src0"], want["agg_src_off"][:n_e]), f"batch {gb}"
            assert np.array_equal(got[f"b{gb}_dst0"], want["agg_dst_off"][:n_e]), f"batch {gb}"
        server.wait(timeout=60)
        assert server.returncode == 0
        text = open(work / "server.log").read()
        assert "Sampling: without replacement" in text and "Server Stopped" in text
    finally:
        if server.poll() is None:
            server.kill()
        log.close()
        for name in os.listdir("/dev/shm"):
            if name.endswith(ns):
                os.unlink(os.path.join("/dev/shm", name))


def test_server_binary_refuses_257_without_replacement(hip, tmp_path, monkeypatch):
    D, B = 24, 48
    ds, indptr, col, feats, labels, sets = _server_dataset(tmp_path, CAP, D)
    work = tmp_path / "run"
    _meta(work, ds, B, indptr.size - 1, col.size, D, sets, 1)
    ns = f"_lr{os.getpid()}"
    env = dict(os.environ, LEGION_IPC_NAMESPACE=ns)
    argv = [os.path.join(ROOT, "legion_amd", "bin", "sampling_server"), "1", "0", str(CAP + 1), "--sample-replace", "0"]
    try:
        p = subprocess.run(argv, cwd=work, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, stdin=subprocess.DEVNULL,
                           text=True, timeout=300)
        assert p.returncode != 0, p.stdout[-2000:]
        assert "sampling without replacement takes fan-outs up to 256" in p.stdout, p.stdout[-2000:]
        assert "System is ready for serving" not in p.stdout
    finally:
        for name in os.listdir("/dev/shm"):
            if name.endswith(ns):
                os.unlink(os.path.join("/dev/shm", name))


# ---- wide feature rows, whole batches -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1030, 2048])
def test_wide_rows_whole_batches_with_a_partial_cache(hip, D):
    """Rows of more than 256 16-byte chunks (the gather's walk with dr = 0, dc = 256): D = 1030 on the dword-aligned path with a
    scalar tail, D = 2048 on the 16-byte path; misses, hits from a partial cache, every mode, against the oracle."""
    wl = Workload(scale=10, edge_factor=8, dim=D, n_seeds=400)
    fanout, batch = [5, 4], 48
    gpu, cpu = GpuSide(wl, batch, fanout), CpuSide(wl, batch, fanout)
    steps = (wl.sets[(0, 0)][0].size - 1) // batch
    for it in range(steps):
        compare_batches(gpu.run(0, it, 0, is_presc=True), cpu.run(0, it, 0, is_presc=True), f"presc {it}: ")
    cap = (wl.N // 4, 100)
    gpu.cache.candidate_selection(0, gpu.graph)
    gpu.cache.set_capacity(*cap)
    gpu.cache.fill_up(gpu.feature, gpu.graph)
    cpu.build_cache(0, capacity=cap)
    hits = misses = 0
    for mode in (0, 1, 2):
        for it in range(2):
            g, c = gpu.run(0, it, mode), cpu.run(0, it, mode)
            compare_batches(g, c, f"D {D} mode {mode} batch {it}: ")
            assert np.array_equal(g["cache_search_buffer"], c["cache_search_buffer"])
            assert g["float_features"].shape[1] == D
            hits += int((g["cache_search_buffer"] >= 0).sum())
            misses += int((g["cache_search_buffer"] < 0).sum())
    assert hits > 0 and misses > 0
    gpu.close(); cpu.close()
