"""bfloat16 feature OUTPUT (MemoryPool / Pipeline feature_out_dtype="bfloat16", legion_pool_set_feature_out_dtype) on the GPU.

Each gathered row must be torch's .to(torch.bfloat16) of the row the oracle gathers, bit for bit, in a contiguous bf16[rows x D]
buffer: for a float32 storage that is round to nearest even (NaNs kept NaNs), for a bf16 storage the stored bits verbatim (the
oracle runs on the pre-rounded table).  Ids, counters, COO offsets and cache_search_buffer stay the oracle's.  Covered: every D
class, every source class of the gather, the lane-group Pipeline with hipGraph replay and weave, and the sampling_server binary
against a trainer process on the view path and the pipe-slot path."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from legion_amd import engine, synth
from oracle import ffi
from tests.gpu_harness import CpuSide, GpuSide
from tests.helpers import Workload, compare_batches
from tests.mode_ref import bf16_bits, rounded
from tests.server_proc import start_server
from tests.test_gpu_boundary import check_trainer_batches, write_dataset

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x7A5C      # a bf16 no gather writes in these tests (their tables hold no such value)


def out_sides(wl, batch, fanout, storage, cache_memory=0, feature_rows=None):
    """GpuSide whose pools hand over bf16 rows (features of the given storage dtype); CpuSide (oracle) on the table that storage
    serves."""
    gpu = GpuSide(wl, batch, fanout, cache_memory=cache_memory)
    if storage == "bfloat16":
        gpu.feature.close()
        gpu.feature = engine.FeatureStorage(wl.P, gpu.features, wl.N, wl.D, feature_dtype="bfloat16")
        for (p, mode), (ids, labels) in wl.sets.items():
            gpu.feature.set_ids(p, mode, ids, labels)
    for p in range(wl.P):
        gpu.pools[p].close()
        pool = engine.MemoryPool(p, wl.N, batch, fanout, wl.D, feature_out_dtype="bfloat16")
        pool.alloc_features(feature_rows if feature_rows is not None else pool.num_ids)
        pool.buffer("float_features").view(torch.int16).fill_(SENTINEL)
        gpu.pools[p] = pool
    torch.cuda.synchronize()
    wl_c = copy.copy(wl)
    if storage == "bfloat16":
        wl_c.features = rounded(wl.features)
    return gpu, CpuSide(wl_c, batch, fanout, feature_rows=feature_rows)


def check(gpu, cpu, dev, it, mode, ctx, pool=None):
    """One batch on both sides: everything but the rows through compare_batches, the rows as bf16 bits; the buffer past the
    batch's rows still holds the sentinel (written again for the next batch)."""
    if pool is None:
        g = gpu.run(dev, it, mode)
    else:
        g = engine.read_batch(pool)
    c = cpu.run(dev, it, mode)
    rows = g.pop("float_features")
    want = c.pop("float_features")
    compare_batches(g, c, ctx)
    assert rows.dtype == np.uint16 and rows.shape == want.shape, (ctx, rows.shape, want.shape)
    wb = bf16_bits(want)
    if not np.array_equal(rows, wb):
        bad = np.nonzero((rows != wb).any(axis=1))[0]
        raise AssertionError(f"{ctx}{bad.size} rows differ, first {bad[:5]}: got {rows[bad[0]][:8]} want {wb[bad[0]][:8]}")
    p = pool if pool is not None else gpu.pools[dev]
    buf = p.buffer("float_features")
    assert buf.dtype == torch.bfloat16 and buf.is_contiguous() and buf.shape[1] == want.shape[1]
    tail = buf[rows.shape[0]:].view(torch.int16).cpu().numpy()
    assert np.all(tail == SENTINEL), f"{ctx}rows past the batch were written"
    buf.view(torch.int16).fill_(SENTINEL)         # for the next batch's check
    torch.cuda.synchronize()
    return g, c


def presample(gpu, cpu, wl, batch):
    steps = min((wl.sets[(p, 0)][0].size - 1) // batch for p in range(wl.P))
    for p in range(wl.P):
        for it in range(steps):
            g, c = gpu.run(p, it, 0, is_presc=True), cpu.run(p, it, 0, is_presc=True)
            compare_batches(g, c, f"presc gpu {p} it {it}: ")
    return steps


# ---- 1. parity through the C ABI, every D class, both storages ----------------------------------------------------------------
CASES = [(storage, D, cache, fanout) for storage in ("float32", "bfloat16")
         for i, D in enumerate([1, 4, 7, 100, 128, 256, 602, 1024])
         for j, cache in enumerate(["none", "partial", "whole"])
         for fanout in [[[6], [5, 4], [4, 3, 2]][(i + j) % 3]]]
CASES += [(storage, D, cache, fanout) for storage in ("float32", "bfloat16")      # more than 256 chunks a row: pitch / 8,
          for i, D in enumerate([2049, 2056, 4096], start=8)                      # (D + 7) / 8 > 256 (after the cases above,
          for j, cache in enumerate(["none", "partial", "whole"])                 # whose ids stay as they were)
          for fanout in [[[6], [5, 4], [4, 3, 2]][(i + j) % 3]]]


@pytest.mark.parametrize("storage,D,cache,fanout", CASES)
def test_bf16_rows_match_torch_of_the_oracle(hip, storage, D, cache, fanout):
    wl = Workload(scale=10, edge_factor=8, dim=D, n_seeds=500)
    batch = 48
    gpu, cpu = out_sides(wl, batch, fanout, storage)
    assert gpu.pools[0].feature_out_dtype == "bfloat16"
    if cache != "none":
        presample(gpu, cpu, wl, batch)
        cap = (wl.N // 4, 200) if cache == "partial" else (wl.N, wl.N)
        gpu.cache.candidate_selection(0, gpu.graph)
        gpu.cache.set_capacity(*cap)
        gpu.cache.fill_up(gpu.feature, gpu.graph)
        cpu.build_cache(0, capacity=cap)
    hits = 0
    for mode in (0, 1):
        for it in range(2):
            g, _ = check(gpu, cpu, 0, it, mode, f"{storage} D {D} cache {cache} mode {mode} batch {it}: ")
            hits += int((g["cache_search_buffer"] >= 0).sum())
    assert (hits > 0) == (cache != "none")
    gpu.close(); cpu.close()


def test_special_values_round_like_torch(hip):
    """float32 storage rows holding ties, subnormals, values past the bf16 maximum, infinities and NaNs."""
    special = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00008000, 0x00018000,
                        0x00007FFF, 0x3F808000, 0x3F818000, 0x3F80C000, 0x3F817FFF, 0xBF808000, 0x7F7FFFFF, 0xFF7FFFFF,
                        0x7F7F7FFF, 0x7F7F8000, 0x7F800000, 0xFF800000, 0x7F800001, 0xFF800001, 0x7FC00000, 0xFFFFFFFF,
                        0x7F807FFF, 0x7FBFFFFF], dtype=np.uint32)
    for D in (7, 26, 128):
        wl = Workload(scale=10, edge_factor=8, dim=D, n_seeds=500)
        flat = wl.features.reshape(-1).view(np.uint32)
        flat[:] = np.resize(special, flat.size)
        batch, fanout = 48, [5, 4]
        gpu, cpu = out_sides(wl, batch, fanout, "float32")
        for it in range(2):
            g = gpu.run(0, it, 0)
            c = cpu.run(0, it, 0)
            got = g["float_features"]
            want = c["float_features"].view(np.uint32)
            nan = (want & 0x7FFFFFFF) > 0x7F800000
            wb = bf16_bits(c["float_features"])
            assert np.array_equal(got[~nan], wb[~nan]), f"D {D} batch {it}"
            assert np.all((got[nan] & 0x7FFF) > 0x7F80) and np.all((got[nan] & 0x40) != 0), "NaNs must stay quiet NaNs"
            assert np.array_equal(got[nan] >> 15, (want[nan] >> 31).astype(np.uint16))
        gpu.close(); cpu.close()


def test_pool_setter_is_refused_after_allocation(hip):
    pool = engine.MemoryPool(0, 1000, 16, [4], 8)
    assert pool.feature_out_dtype == "float32"
    pool.set_feature_out_dtype("bfloat16")
    pool.set_feature_out_dtype("float32")
    pool.alloc_features(pool.num_ids)
    assert pool.buffer("float_features").dtype == torch.float32
    with pytest.raises(RuntimeError):
        pool.set_feature_out_dtype("bfloat16")
    assert pool._lib.legion_pool_set_feature_out_dtype(pool.handle, 1) == -1
    assert pool.feature_out_dtype == "float32"
    pool.close()


# ---- 2. tiers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["float32", "bfloat16"])
@pytest.mark.parametrize("D,replica_rows", [(32, 0), (32, 60), (100, 0), (7, 40)])
def test_striped_clique_and_replica(hip, col_slots, storage, D, replica_rows):
    P, mode_bits, capacity = 2, 1, (150, 90)
    wl = Workload(scale=11, edge_factor=8, dim=D, partition_count=P, n_seeds=1200)
    fanout, batch = [5, 4], 64
    gpu, cpu = out_sides(wl, batch, fanout, storage)
    presample(gpu, cpu, wl, batch)
    gpu.cache.candidate_selection(mode_bits, gpu.graph)
    gpu.cache.set_capacity(*capacity)
    if replica_rows:
        gpu.cache.set_replica_memory(replica_rows * (2 * engine.bf16_pitch(D) if storage == "bfloat16" else 4 * D))
    gpu.cache.fill_up(gpu.feature, gpu.graph)
    cpu.build_cache(mode_bits, capacity=capacity)
    for p in range(P):
        assert gpu.cache.replica_rows(p) == replica_rows
        gpu.cache.gather_stats(p)
        for it in range(2):
            check(gpu, cpu, p, it, 0, f"clique {storage} gpu {p} batch {it}: ")
        stripe, replica, peer = gpu.cache.gather_stats3(p)
        assert peer > 0 and (replica > 0) == (replica_rows > 0)
    gpu.close(); cpu.close()


@pytest.mark.parametrize("storage", ["float32", "bfloat16"])
def test_bulk_peer_gather_is_refused(hip, storage):
    wl = Workload(scale=10, edge_factor=8, dim=32, partition_count=2, n_seeds=600)
    fanout, batch = [5, 4], 48
    gpu, cpu = out_sides(wl, batch, fanout, storage)
    presample(gpu, cpu, wl, batch)
    gpu.cache.candidate_selection(1, gpu.graph)
    gpu.cache.set_capacity(100, 50)
    gpu.cache.fill_up(gpu.feature, gpu.graph)
    pipe = engine.Pipeline(gpu.graph, gpu.feature, gpu.cache, 0, batch, fanout, 2, ffi.num_ids_for(batch, fanout), use_graph=False,
                           slots=2, arena="shared", feature_out_dtype="bfloat16")
    with pytest.raises(RuntimeError):
        pipe.bulk_enable()
    pipe.close()
    gpu.close(); cpu.close()


@pytest.mark.parametrize("storage", ["float32", "bfloat16"])
@pytest.mark.parametrize("D,cpu_cap,gpu_cap", [(128, 300, 200), (100, 250, 0), (7, 40, 40)])
def test_hybrid_tier_against_the_oracle(hip, storage, D, cpu_cap, gpu_cap):
    wl = Workload(scale=11, edge_factor=8, dim=D, n_seeds=1200)
    fanout, batch = [5, 4], 64
    gpu, cpu = out_sides(wl, batch, fanout, storage)
    presample(gpu, cpu, wl, batch)
    gpu.cache.hybrid_init(gpu.feature, gpu.graph, cpu_cap, gpu_cap)
    oc = ffi.OracleCache(wl.N, wl.D, 1, 0)
    oc.hybrid_init(cpu.node_access[0], cpu.wl.features, cpu_cap, gpu_cap)
    cpu.Kg, cpu.caches = 1, [oc]
    for mode in (0, 1, 2):
        check(gpu, cpu, 0, 0, mode, f"hybrid {storage} mode {mode}: ")
    gpu.close(); cpu.close()


@pytest.mark.parametrize("storage", ["float32", "bfloat16"])
def test_pinned_table_placement(hip, monkeypatch, storage):
    monkeypatch.setenv("LEGION_TABLE_PLACEMENT", "pinned")
    wl = Workload(scale=10, edge_factor=8, dim=100, n_seeds=500)
    fanout, batch = [5, 4], 48
    gpu, cpu = out_sides(wl, batch, fanout, storage)
    for it in range(2):
        check(gpu, cpu, 0, it, 0, f"pinned {storage} batch {it}: ")
    gpu.close(); cpu.close()


@pytest.mark.parametrize("storage", ["float32", "bfloat16"])
@pytest.mark.parametrize("group,slots,weave,D", [(3, 2, False, 100), (4, 2, True, 128), (2, 2, True, 7)])
def test_lane_group_pipeline_with_graph_replay(hip, storage, group, slots, weave, D):
    wl = Workload(scale=11, edge_factor=8, dim=D, n_seeds=700)
    fanout, batch = [6, 3], 64
    gpu, cpu = out_sides(wl, batch, fanout, storage)
    presample(gpu, cpu, wl, batch)
    gpu.cache.candidate_selection(0, gpu.graph)
    gpu.cache.set_capacity(150, 80)
    gpu.cache.fill_up(gpu.feature, gpu.graph)
    cpu.build_cache(0, capacity=(150, 80))
    num_ids = gpu.pools[0].num_ids
    pipe = engine.Pipeline(gpu.graph, gpu.feature, gpu.cache, 0, batch, fanout, group, num_ids, True, slots, weave=weave,
                           feature_out_dtype="bfloat16")
    for row in pipe.pools:
        for pool in row:
            assert pool.feature_out_dtype == "bfloat16"
            pool.buffer("float_features").view(torch.int16).fill_(SENTINEL)
    torch.cuda.synchronize()
    n_batches = (wl.sets[(0, 0)][0].size + batch - 1) // batch
    for gi in range(min((n_batches + group - 1) // group, 3)):
        sl = pipe.submit(gi * group, 0)
        pipe.wait(sl)
        for lane in range(min(group, n_batches - gi * group)):
            pool = pipe.pools[sl][lane]
            check(gpu, cpu, 0, gi * group + lane, 0, f"{storage} group {gi} lane {lane}: ", pool=pool)
    pipe.close()
    gpu.close(); cpu.close()


# ---- 3. end to end: the server binary and a trainer process --------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("path", ["view", "slot"])
@pytest.mark.parametrize("disk", [False, True], ids=["in-memory", "disk"])
def test_server_hands_bf16_rows_to_the_trainer(hip, tmp_path, monkeypatch, storage, path, disk):
    scale, D, B, fanout, epoch, cache_memory, cpu_cap, gpu_cap = 11, 20, 48, [5, 3], 2, 60_000, 260, 170
    indptr, col = synth.rmat_csr_numpy(scale, 8, 20231)
    N = indptr.size - 1
    feats = synth.features_numpy(0, N, D, 7)
    feats_r = rounded(feats)      # what a bf16 storage serves, and torch's bf16 of every float32 row (widened back, exactly)
    labels = (np.arange(N) % 47).astype(np.int32)
    perm = np.random.RandomState(3).permutation(N).astype(np.int32)
    train, valid, test = perm[:500], perm[500:590], perm[590:640]
    ds = str(tmp_path / "ds") + "/"
    write_dataset(ds, indptr, col, feats, labels, train, valid, test)
    work = tmp_path / "run"
    work.mkdir()
    fields = [ds, B, N, col.size, D, train.size, valid.size, test.size, cache_memory, epoch] + ([0, 0, 0, cpu_cap, gpu_cap] if disk else [])
    (work / "meta_config").write_text(" ".join(str(f) for f in fields))
    ns = f"_bo{os.getpid()}"
    monkeypatch.setenv("LEGION_IPC_NAMESPACE", ns)
    env = dict(os.environ)
    tenv = dict(env)
    if path == "slot":
        tenv["LEGION_NO_DIRECT_VIEWS"] = "1"
    argv = [os.path.join(ROOT, "legion_amd", "bin", "sampling_server"), "1", "0"] + [str(f) for f in fanout] + \
        (["--disk"] if disk else []) + ["--feature-dtype", storage, "--feature-out-dtype", "bf16"]
    server, log = start_server(argv, work, env, work / "server.log")
    try:
        import ctypes
        g = ffi.OracleGraph(1, indptr, col)
        st = ffi.Steps()
        L = ffi.load()
        one = lambda v: (ctypes.c_int32 * 1)(v)
        L.lgo_coordinate(ctypes.byref(st), 1, one(train.size), one(valid.size), one(test.size), B, epoch)
        node_acc, edge_acc = np.zeros(N, dtype=np.uint64), np.zeros(N, dtype=np.uint64)
        max_bs = max(B, st.valid_bs[0], st.test_bs[0])
        pool = ffi.OraclePool(N, max_bs, fanout, ffi.num_ids_for(max_bs, fanout), D)
        max_ids = 0
        for it in range(st.train_step):
            pool.run_batch(g, None, None, train, labels[train], B, it, 0, True, node_acc, edge_acc)
            max_ids = max(max_ids, int(pool.read_batch()["node_counter"][7]))
        cache = ffi.OracleCache(N, D, 1, 0)
        if disk:
            cache.hybrid_init(node_acc, feats_r, cpu_cap, gpu_cap)
        else:
            cm = ffi.OracleCache(N, engine.bf16_pitch(D) // 2 if storage == "bf16" else D, 1, 0)
            cm.candidate_selection([node_acc], [edge_acc])
            cm.cost_model(cache_memory, indptr, (0, 0), [max_ids], st.train_step)
            cache.candidate_selection([node_acc], [edge_acc])
            cache.set_capacity(cm.node_capacity, cm.edge_capacity)
            cache.fill_up(feats_r, indptr, col)
            g.attach_cache(cache)
        out_npz = tmp_path / "trainer.npz"
        tr = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bf16_trainer.py"), "0", str(D), str(epoch), str(out_npz)],
                            env=tenv, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, stdin=subprocess.DEVNULL, text=True,
                            timeout=300)
        assert tr.returncode == 0, tr.stdout[-3000:] + "\n---- server ----\n" + open(work / "server.log").read()[-2000:]
        got = np.load(out_npz)
        check_trainer_batches(got, st, pool, g, cache, feats_r, {0: train, 1: valid, 2: test}, labels, fanout, D, epoch)
        server.wait(timeout=60)
        assert server.returncode == 0
        text = open(work / "server.log").read()
        assert "Feature output dtype: bf16" in text and "Server Stopped" in text
    finally:
        if server.poll() is None:
            server.kill()
        log.close()
        for name in os.listdir("/dev/shm"):
            if name.endswith(ns):
                os.unlink(os.path.join("/dev/shm", name))
