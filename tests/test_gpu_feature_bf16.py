"""bfloat16 feature storage (FeatureStorage feature_dtype="bfloat16", legion_hip.h LEGION_FEATURE_BF16) on the GPU.

The conversion f32 -> bf16 is torch's round to nearest even, bit for bit.  Everything else is parity: the oracle copies rows
verbatim, so the oracle run on the table pre-rounded to bf16 (and widened back, exactly) is what a bf16 storage must serve --
ids, counters, COO offsets, cache_search_buffer and every float32 row byte-equal -- through every source class of the gather
(full table, stripes, peer stripes, replica, hybrid CPU / GPU caches), the lane-group Pipeline with hipGraph, and the
sampling_server binary against a trainer process."""
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
from tests.mode_ref import rounded
from tests.server_proc import start_server
from tests.test_gpu_boundary import check_trainer_batches, write_dataset

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def torch_bf16_bits(x):
    return torch.from_numpy(x.view(np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def convert_on_gpu(x, D):
    """uint32 bit patterns (rows of D) through legion_convert_f32_to_bf16; returns the uint16 bits, pad columns included."""
    src = torch.from_numpy(x.view(np.float32).reshape(-1, D)).cuda()
    out = engine.convert_f32_to_bf16(src)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint16)


def bf16_sides(wl, batch, fanout, **kw):
    """GpuSide with a bf16 FeatureStorage over the float32 table; CpuSide (oracle) over the pre-rounded table."""
    gpu = GpuSide(wl, batch, fanout, **kw.get("gpu", {}))
    gpu.feature.close()
    gpu.feature = engine.FeatureStorage(wl.P, gpu.features, wl.N, wl.D, feature_dtype="bfloat16")
    for (p, mode), (ids, labels) in wl.sets.items():
        gpu.feature.set_ids(p, mode, ids, labels)
    assert gpu.feature.row_bytes == 2 * engine.bf16_pitch(wl.D)
    wl_r = copy.copy(wl)
    wl_r.features = rounded(wl.features)
    cpu = CpuSide(wl_r, batch, fanout)
    return gpu, cpu


def presample(gpu, cpu, wl, batch):
    steps = min((wl.sets[(p, 0)][0].size - 1) // batch for p in range(wl.P))
    assert steps >= 1
    for p in range(wl.P):
        for it in range(steps):
            compare_batches(gpu.run(p, it, 0, is_presc=True), cpu.run(p, it, 0, is_presc=True), f"presc gpu {p} it {it}: ")
    return steps


# ---- 1. the conversion ---------------------------------------------------------------------------------------------------
def test_conversion_matches_torch_bit_for_bit(hip):
    rng = np.random.RandomState(5)
    bits = rng.randint(0, 2 ** 32, size=3 * 2 ** 20 + 40, dtype=np.uint64).astype(np.uint32)
    bits = bits[(bits & 0x7FFFFFFF) <= 0x7F800000]                 # NaNs: their own test
    special = np.array([0x00000000, 0x80000000,                     # +-0
                        0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00008000, 0x00018000, 0x00007FFF,   # subnormals
                        0x3F808000, 0x3F818000, 0x3F80C000, 0x3F817FFF, 0xBF808000,                          # ties / near ties
                        0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F7FFF, 0x7F7F8000,                                      # FLT_MAX, past the max
                        0x7F800000, 0xFF800000], dtype=np.uint32)                                            # +-inf
    for D, x in ((128, bits[:(bits.size // 128) * 128]), (7, np.tile(special, 7)), (1, special)):
        got = convert_on_gpu(x, D)
        P = engine.bf16_pitch(D)
        assert got.shape == (x.size // D, P)
        want = torch_bf16_bits(x).reshape(-1, D)
        assert np.array_equal(got[:, :D], want), np.nonzero(got[:, :D] != want)
        assert np.all(got[:, D:] == 0)                               # pad elements
    # what the special values must give (torch's rounding, stated)
    got = convert_on_gpu(special, 1)[:, 0]
    assert got[special.tolist().index(0x3F808000)] == 0x3F80 and got[special.tolist().index(0x3F818000)] == 0x3F82
    assert got[special.tolist().index(0x7F7FFFFF)] == 0x7F80 and got[special.tolist().index(0xFF7FFFFF)] == 0xFF80
    assert got[special.tolist().index(0x00000001)] == 0x0000 and got[special.tolist().index(0x007FFFFF)] == 0x0080


def test_conversion_keeps_nans(hip):
    nans = np.array([0x7F800001, 0xFF800001, 0x7FC00000, 0xFFC00000, 0x7FFFFFFF, 0xFFFFFFFF, 0x7F807FFF, 0x7FBFFFFF,
                     0x7F80FFFF, 0xFF808000], dtype=np.uint32)
    got = convert_on_gpu(np.tile(nans, 3), 3).reshape(-1, 8)[:, :3].ravel()
    assert np.all((got & 0x7FFF) > 0x7F80), [hex(v) for v in got]


# ---- 2. parity through the C ABI -------------------------------------------------------------------------------------------
CASES = [(D, cache, fanout) for i, D in enumerate([1, 4, 7, 100, 128, 256, 602, 1024,
                                                   2049, 2056, 4096])      # more than 256 chunks a row: pitch / 8, (D + 7) / 8 > 256
         for j, cache in enumerate(["none", "partial", "whole"])
         for fanout in [[[6], [5, 4], [4, 3, 2]][(i + j) % 3]]]


@pytest.mark.parametrize("D,cache,fanout", CASES)
def test_batches_match_the_oracle_on_the_rounded_table(hip, D, cache, fanout):
    wl = Workload(scale=10, edge_factor=8, dim=D, n_seeds=500)
    batch = 48
    gpu, cpu = bf16_sides(wl, batch, fanout)
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
            g, c = gpu.run(0, it, mode), cpu.run(0, it, mode)
            compare_batches(g, c, f"D {D} cache {cache} mode {mode} batch {it}: ")
            assert np.array_equal(g["cache_search_buffer"], c["cache_search_buffer"])
            assert g["float_features"].shape[1] == D
            hits += int((g["cache_search_buffer"] >= 0).sum())
    assert (hits > 0) == (cache != "none")
    gpu.close(); cpu.close()


# ---- 3. the cost model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,cache_memory,counters", [(64, 200_000, (0, 0)), (100, 400_000, (50_000, 70_000)), (7, 100_000, (0, 0)),
                                                     (128, 3_000_000, (9, 9))])
def test_cost_model_counts_bf16_row_bytes(hip, D, cache_memory, counters):
    """D enters the model only as row bytes: a bf16 cache sizes like the oracle's with D' = P / 2."""
    wl = Workload(scale=12, edge_factor=8, dim=D, n_seeds=2000)
    fanout, batch = [10, 5], 128
    gpu, cpu = bf16_sides(wl, batch, fanout, gpu={"cache_memory": cache_memory})
    steps = presample(gpu, cpu, wl, batch)
    gpu.cache.candidate_selection(0, gpu.graph)
    gpu.cache.cost_model(gpu.feature, gpu.graph, counters, steps)
    oc = ffi.OracleCache(wl.N, engine.bf16_pitch(D) // 2, 1, 0)
    oc.candidate_selection([cpu.node_access[0]], [cpu.edge_access[0]])
    oc.cost_model(cache_memory, wl.indptr, counters, cpu.max_ids[:1], steps)
    cap = (gpu.cache.node_capacity(0), gpu.cache.edge_capacity(0))
    assert cap == (oc.node_capacity, oc.edge_capacity)
    oc.close()
    gpu.cache.fill_up(gpu.feature, gpu.graph)
    cpu.build_cache(0, capacity=cap)
    g, c = gpu.run(0, 0, 0), cpu.run(0, 0, 0)
    compare_batches(g, c, "serve after cost model: ")
    assert np.array_equal(g["cache_search_buffer"], c["cache_search_buffer"])
    gpu.close(); cpu.close()


# ---- 4. tiers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,replica_rows", [(32, 0), (32, 60), (100, 0), (7, 40)])
def test_striped_clique_and_replica(hip, col_slots, D, replica_rows):
    """Two logical GPUs on the one device as a clique (peer_gather = direct): own stripe, the peer's stripe, the replica."""
    P, mode_bits, capacity = 2, 1, (150, 90)
    wl = Workload(scale=11, edge_factor=8, dim=D, partition_count=P, n_seeds=1200)
    fanout, batch = [5, 4], 64
    gpu, cpu = bf16_sides(wl, batch, fanout)
    presample(gpu, cpu, wl, batch)
    gpu.cache.candidate_selection(mode_bits, gpu.graph)
    gpu.cache.set_capacity(*capacity)
    if replica_rows:
        gpu.cache.set_replica_memory(replica_rows * 2 * engine.bf16_pitch(D))      # bf16 row bytes: exactly replica_rows rows
    gpu.cache.fill_up(gpu.feature, gpu.graph)
    cpu.build_cache(mode_bits, capacity=capacity)
    for p in range(P):
        assert gpu.cache.replica_rows(p) == replica_rows
        gpu.cache.gather_stats(p)                       # arms the counters
        for it in range(2):
            g, c = gpu.run(p, it, 0), cpu.run(p, it, 0)
            compare_batches(g, c, f"clique gpu {p} batch {it}: ")
            assert np.array_equal(g["cache_search_buffer"], c["cache_search_buffer"])
        stripe, replica, peer = gpu.cache.gather_stats3(p)
        assert peer > 0 and (replica > 0) == (replica_rows > 0)
        assert gpu.cache.peer_transactions(p) == peer * 2 * engine.bf16_pitch(D) // 64
    gpu.close(); cpu.close()


def test_bulk_peer_gather_is_refused(hip):
    wl = Workload(scale=10, edge_factor=8, dim=32, partition_count=2, n_seeds=600)
    fanout, batch = [5, 4], 48
    gpu, cpu = bf16_sides(wl, batch, fanout)
    presample(gpu, cpu, wl, batch)
    gpu.cache.candidate_selection(1, gpu.graph)
    gpu.cache.set_capacity(100, 50)
    gpu.cache.fill_up(gpu.feature, gpu.graph)
    pipe = engine.Pipeline(gpu.graph, gpu.feature, gpu.cache, 0, batch, fanout, 2, ffi.num_ids_for(batch, fanout), use_graph=False,
                           slots=2, arena="shared")
    with pytest.raises(RuntimeError):
        pipe.bulk_enable()
    pipe.close()
    gpu.close(); cpu.close()


@pytest.mark.parametrize("D,cpu_cap,gpu_cap", [(128, 300, 200), (100, 250, 0), (7, 40, 40), (24, 0, 250)])
def test_hybrid_tier_against_the_oracle(hip, D, cpu_cap, gpu_cap):
    wl = Workload(scale=11, edge_factor=8, dim=D, n_seeds=1200)
    fanout, batch = [5, 4], 64
    gpu, cpu = bf16_sides(wl, batch, fanout)
    presample(gpu, cpu, wl, batch)
    gpu.cache.hybrid_init(gpu.feature, gpu.graph, cpu_cap, gpu_cap)
    oc = ffi.OracleCache(wl.N, wl.D, 1, 0)
    oc.hybrid_init(cpu.node_access[0], cpu.wl.features, cpu_cap, gpu_cap)
    cpu.Kg, cpu.caches = 1, [oc]
    slots = []
    for mode in (0, 1, 2):
        g, c = gpu.run(0, 0, mode), cpu.run(0, 0, mode)
        compare_batches(g, c, f"hybrid mode {mode}: ")
        assert np.array_equal(g["cache_search_buffer"], c["cache_search_buffer"])
        slots.append(g["cache_search_buffer"])
    s = np.concatenate(slots)
    assert ((s >= 0) & (s < cpu_cap)).any() == (cpu_cap > 0) and (s >= cpu_cap).any() == (gpu_cap > 0) and (s < 0).any()
    gpu.close(); cpu.close()


def test_pinned_table_placement(hip, monkeypatch):
    monkeypatch.setenv("LEGION_TABLE_PLACEMENT", "pinned")
    wl = Workload(scale=10, edge_factor=8, dim=100, n_seeds=500)
    fanout, batch = [5, 4], 48
    gpu, cpu = bf16_sides(wl, batch, fanout)
    for it in range(2):
        compare_batches(gpu.run(0, it, 0), cpu.run(0, it, 0), f"pinned batch {it}: ")
    gpu.close(); cpu.close()


@pytest.mark.parametrize("group,slots,weave", [(3, 2, False), (4, 2, True)])
def test_lane_group_pipeline_with_graph_replay(hip, group, slots, weave):
    wl = Workload(scale=11, edge_factor=8, dim=100, n_seeds=700)
    fanout, batch = [6, 3], 64
    gpu, cpu = bf16_sides(wl, batch, fanout)
    presample(gpu, cpu, wl, batch)
    gpu.cache.candidate_selection(0, gpu.graph)
    gpu.cache.set_capacity(150, 80)
    gpu.cache.fill_up(gpu.feature, gpu.graph)
    cpu.build_cache(0, capacity=(150, 80))
    pipe = engine.Pipeline(gpu.graph, gpu.feature, gpu.cache, 0, batch, fanout, group, gpu.pools[0].num_ids, True, slots, weave=weave)
    n_batches = (wl.sets[(0, 0)][0].size + batch - 1) // batch
    for gi in range((n_batches + group - 1) // group):
        sl = pipe.submit(gi * group, 0)
        pipe.wait(sl)
        for lane in range(group):
            compare_batches(engine.read_batch(pipe.pools[sl][lane]), cpu.run(0, gi * group + lane, 0), f"group {gi} lane {lane}: ")
    pipe.close()
    gpu.close(); cpu.close()


# ---- 5. end to end: the server binary and a trainer process --------------------------------------------------------------------
@pytest.mark.parametrize("disk", [False, True], ids=["in-memory", "disk"])
def test_server_binary_with_bf16_features(hip, tmp_path, monkeypatch, disk):
    scale, D, B, fanout, epoch, cache_memory, cpu_cap, gpu_cap = 11, 20, 48, [5, 3], 2, 60_000, 260, 170
    indptr, col = synth.rmat_csr_numpy(scale, 8, 20231)
    N = indptr.size - 1
    feats = synth.features_numpy(0, N, D, 7)
    feats_r = rounded(feats)
    assert not np.array_equal(feats_r, feats)
    labels = (np.arange(N) % 47).astype(np.int32)
    perm = np.random.RandomState(3).permutation(N).astype(np.int32)
    train, valid, test = perm[:500], perm[500:590], perm[590:640]
    ds = str(tmp_path / "ds") + "/"
    write_dataset(ds, indptr, col, feats, labels, train, valid, test)
    work = tmp_path / "run"
    work.mkdir()
    fields = [ds, B, N, col.size, D, train.size, valid.size, test.size, cache_memory, epoch] + ([0, 0, 0, cpu_cap, gpu_cap] if disk else [])
    (work / "meta_config").write_text(" ".join(str(f) for f in fields))
    ns = f"_bf{os.getpid()}"
    monkeypatch.setenv("LEGION_IPC_NAMESPACE", ns)
    env = dict(os.environ)
    argv = [os.path.join(ROOT, "legion_amd", "bin", "sampling_server"), "1", "0"] + [str(f) for f in fanout] + \
        (["--disk"] if disk else []) + ["--feature-dtype", "bf16"]
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
            cm = ffi.OracleCache(N, engine.bf16_pitch(D) // 2, 1, 0)        # bf16 rows in the cost model
            cm.candidate_selection([node_acc], [edge_acc])
            cm.cost_model(cache_memory, indptr, (0, 0), [max_ids], st.train_step)
            cache.candidate_selection([node_acc], [edge_acc])
            cache.set_capacity(cm.node_capacity, cm.edge_capacity)
            cache.fill_up(feats_r, indptr, col)
            g.attach_cache(cache)
        out_npz = tmp_path / "trainer.npz"
        tr = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fake_trainer.py"), "0", str(D), str(epoch), str(out_npz)],
                            env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, stdin=subprocess.DEVNULL, text=True,
                            timeout=300)
        assert tr.returncode == 0, tr.stdout[-3000:] + "\n---- server ----\n" + open(work / "server.log").read()[-2000:]
        got = np.load(out_npz)
        check_trainer_batches(got, st, pool, g, cache, feats_r, {0: train, 1: valid, 2: test}, labels, fanout, D, epoch)
        server.wait(timeout=60)
        assert server.returncode == 0
        text = open(work / "server.log").read()
        assert "Feature dtype: bf16" in text and "Server Stopped" in text
    finally:
        if server.poll() is None:
            server.kill()
        log.close()
        for name in os.listdir("/dev/shm"):
            if name.endswith(ns):
                os.unlink(os.path.join("/dev/shm", name))
