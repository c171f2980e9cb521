"""Sampling without replacement on the GPU (MemoryPool / Pipeline replace=False): the picks of legion_draw_distinct_batch and
whole batches of every sampler class, bit for bit against the numpy restatement in tests/distinct_ref.py."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import ffi
from tests import distinct_ref as ref
from tests.gpu_harness import GpuSide
from tests.helpers import KEYS_EXACT, Workload, compare_batches

pytestmark = pytest.mark.gpu


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _distinct(gpu):
    for pool in gpu.pools:
        pool.set_replace(False)
        assert pool.replace is False
    return gpu


def _want(wl, dev, it, mode, batch, fanout, serve=True, edge_access=None, node_access=None):
    ids, labels = wl.sets[(dev, mode)]
    return ref.run_batch(wl.indptr, wl.col, ids, labels, batch, it, fanout, serve, edge_access, node_access)


def _compare(got, want, wl, ctx):
    compare_batches(got, want, ctx)
    if "float_features" in got and wl.D > 0:
        rows = got["float_features"][:want["sampled_ids"].size]
        assert np.array_equal(rows.view(np.uint32), wl.features[want["sampled_ids"]].view(np.uint32)), f"{ctx}gathered rows"


@pytest.mark.parametrize("f", [1, 2, 3, 10, 25, 40])
def test_picks_match_the_reference(hip, f):
    from legion_amd import lib
    L = lib.load()
    D = np.array([1, f, f + 1, 2 * f, 1000, 10**6, 2**30] * 97, dtype=np.int32)
    base = (np.arange(D.size, dtype=np.int64) * f + 4_000_000).astype(np.int32)
    dev = torch.device("cuda:0")
    tb, td = torch.from_numpy(base).to(dev), torch.from_numpy(D).to(dev)
    out = torch.full((D.size * f,), -7, dtype=torch.int32, device=dev)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.legion_draw_distinct_batch(s, _p(tb), _p(td), f, _p(out), D.size) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().reshape(D.size, f), ref.picks(base, D, f))


@pytest.mark.parametrize("fanout", [[25, 10], [3], [4, 3], [2, 2, 2], [3, 2, 2, 2], [2, 2, 2, 2, 2], [2, 2, 2, 2, 2, 2], [40, 3]])
def test_batches_every_mode_and_the_clamped_last_batch(hip, fanout):
    wl = Workload(scale=11, edge_factor=8, dim=16, n_seeds=700)
    batch = 64
    gpu = _distinct(GpuSide(wl, batch, fanout))
    n_train = (wl.sets[(0, 0)][0].size + batch - 1) // batch          # the last batch is clamped
    for it in list(range(3)) + [n_train - 1]:
        _compare(gpu.run(0, it, 0), _want(wl, 0, it, 0, batch, fanout), wl, f"{fanout} train {it}: ")
    for mode in (1, 2):
        _compare(gpu.run(0, 0, mode), _want(wl, 0, 0, mode, batch, fanout), wl, f"{fanout} mode {mode}: ")
    assert gpu.pools[0].error() == 0
    gpu.close()


@pytest.mark.parametrize("buckets,claim_cap", [("8", "1"), ("16", "40"), ("16", None)])
def test_small_classes_with_claim_list_overflow(hip, monkeypatch, buckets, claim_cap):
    monkeypatch.setenv("LEGION_LDS_SMALL_BUCKETS", buckets)
    if claim_cap is not None:
        monkeypatch.setenv("LEGION_LDS_CLAIM_CAP", claim_cap)
    wl = Workload(scale=12, edge_factor=8, dim=4, n_seeds=600)
    fanout, batch = [4, 3, 3], 48
    gpu = _distinct(GpuSide(wl, batch, fanout))
    for it in range(4):
        _compare(gpu.run(0, it, 0), _want(wl, 0, it, 0, batch, fanout), wl, f"{buckets} buckets cap {claim_cap} batch {it}: ")
    assert gpu.pools[0].error() == 0
    gpu.close()


@pytest.mark.parametrize("batch,fanout", [(6000, [10, 10]), (6000, [10, 10, 8])], ids=["64buckets", "256buckets"])
def test_large_classes(hip, batch, fanout):
    wl = Workload(scale=15, edge_factor=16, dim=4, n_seeds=13000)
    gpu = _distinct(GpuSide(wl, batch, fanout))
    _compare(gpu.run(0, 1, 0), _want(wl, 0, 1, 0, batch, fanout), wl, f"{batch} {fanout}: ")
    assert gpu.pools[0].error() == 0
    gpu.close()


def test_presc_hotness_then_topology_cache(hip, col_slots):
    """PreSC in distinct mode counts the hotness of the distinct edges; the caches built from it then serve the same batches from
    the cached topology (with and without column slots), and the topology hit mask of the last hop is the oracle cache's."""
    wl = Workload(scale=11, edge_factor=8, dim=32, n_seeds=700)
    fanout, batch = [6, 3], 64
    gpu = _distinct(GpuSide(wl, batch, fanout))
    steps = (wl.sets[(0, 0)][0].size - 1) // batch
    ea, na = np.zeros(wl.N, np.uint64), np.zeros(wl.N, np.uint64)
    for it in range(steps):
        g = gpu.run(0, it, 0, is_presc=True)
        compare_batches(g, _want(wl, 0, it, 0, batch, fanout, serve=False, edge_access=ea, node_access=na), f"presc {it}: ")
    assert np.array_equal(gpu.cache.array("edge_access_time", 0).cpu().numpy().view(np.uint64), ea)
    assert np.array_equal(gpu.cache.array("node_access_time", 0).cpu().numpy().view(np.uint64), na)
    gpu.cache.candidate_selection(0, gpu.graph)
    gpu.cache.set_capacity(150, 80)                     # rows served from the cached topology and the full CSR
    gpu.cache.fill_up(gpu.feature, gpu.graph)
    oc = ffi.OracleCache(wl.N, wl.D, 1, 0)             # the same cache built by the oracle from the reference's hotness
    oc.candidate_selection([na], [ea])
    oc.set_capacity(150, 80)
    oc.fill_up(wl.features, wl.indptr, wl.col)
    L = ffi.load()
    topo = 0
    for it in range(3):
        g = gpu.run(0, it, 0)
        want = _want(wl, 0, it, 0, batch, fanout)
        _compare(g, want, wl, f"cached topology {it}: ")
        ec = want["edge_counter"]
        frontier = np.ascontiguousarray(want["agg_src_ids"][ec[9]:ec[10]])          # the last hop's frontier
        tp_c = np.zeros(max(frontier.size, 1), np.int8)
        off = np.zeros(max(frontier.size, 1), np.int32)
        L.lgo_find_topo(oc.c, frontier.ctypes.data_as(ffi.P_I32), tp_c.ctypes.data_as(ffi.P_I8), off.ctypes.data_as(ffi.P_I32),
                        frontier.size)
        tp_g = gpu.pools[0].buffer("tmp_part_ind")[:frontier.size].cpu().numpy()
        assert np.array_equal(tp_g, tp_c[:frontier.size]), f"tmp_part_ind batch {it}"
        topo += int((tp_g >= 0).sum())
    assert topo > 0                                     # some rows did come from the cached topology
    assert gpu.graph.column_slots(0) == col_slots
    oc.close()
    gpu.close()


@pytest.mark.parametrize("group,slots,use_graph,weave", [(4, 2, True, False), (3, 2, True, True), (2, 2, False, False)])
def test_pipeline_graph_replay_and_weave(hip, group, slots, use_graph, weave):
    from legion_amd import engine
    wl = Workload(scale=11, edge_factor=8, dim=32, n_seeds=700)
    fanout, batch = [6, 3], 64
    gpu = _distinct(GpuSide(wl, batch, fanout))
    gpu.cache.candidate_selection(0, gpu.graph)
    gpu.cache.set_capacity(150, 80)
    gpu.cache.fill_up(gpu.feature, gpu.graph)
    pipe = engine.Pipeline(gpu.graph, gpu.feature, gpu.cache, 0, batch, fanout, group, gpu.pools[0].num_ids, use_graph, slots,
                           weave=weave, replace=False)
    n_batches = (wl.sets[(0, 0)][0].size + batch - 1) // batch
    n_groups = min((n_batches + group - 1) // group, 4)
    for gi in range(n_groups):
        sl = pipe.submit(gi * group, 0)
        pipe.wait(sl)
        for lane in range(group):
            b = gi * group + lane
            got = engine.read_batch(pipe.pools[sl][lane])
            _compare(got, _want(wl, 0, b, 0, batch, fanout), wl, f"group {gi} lane {lane}: ")
            if lane == 0 and gi == 0:
                eager = gpu.run(0, b, 0)
                for k in KEYS_EXACT:
                    assert np.array_equal(got[k], eager[k]), k
    with pytest.raises(RuntimeError):
        pipe.set_replace(True)                          # the captured graphs never mix modes
    pipe.close()
    gpu.close()


def test_setters_default_and_refusals(hip):
    from legion_amd import engine
    wl = Workload(scale=10, edge_factor=8, dim=4, n_seeds=200)
    gpu = GpuSide(wl, 32, [4, 2])
    pool = gpu.pools[0]
    assert pool.replace is True and int(pool._lib.legion_pool_sample_replace(pool.handle)) == 1
    pool.set_replace(False)
    pool.set_replace(True)                              # free to change before the first hop
    gpu.run(0, 0, 0)
    with pytest.raises(RuntimeError):
        pool.set_replace(False)
    assert pool.replace is True
    big = engine.MemoryPool(0, wl.N, 4, [300], wl.D)
    with pytest.raises(RuntimeError):
        big.set_replace(False)                          # fan-outs above 256 only with replacement
    big.close()
    gpu.close()


def test_group_lanes_share_one_mode(hip):
    """Every lane of an eager lane group is fixed once the group has sampled, and a group whose lanes disagree is refused
    (nothing enqueued, error bit 8) instead of sampling every lane with lane 0's mode."""
    from legion_amd import engine, lib
    L = lib.load()
    wl = Workload(scale=10, edge_factor=8, dim=4, n_seeds=200)
    fanout, batch = [4, 2], 32
    gpu = GpuSide(wl, batch, fanout)
    pools = [engine.MemoryPool(0, wl.N, batch, fanout, wl.D) for _ in range(2)]
    for pl in pools:
        pl.alloc_features(pl.num_ids)
    arr = (ctypes.c_void_p * 2)(*[pl.handle for pl in pools])
    grp = L.legion_group_create(arr, 2)
    fo = (ctypes.c_int32 * 2)(*fanout)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    pools[1].set_replace(False)                          # lanes disagree: refused
    L.legion_enqueue_group(s, gpu.graph.handle, gpu.feature.handle, gpu.cache.handle, grp, batch, 0, 0, 0, fo, 2)
    torch.cuda.synchronize()
    assert all(pl.error() & 8 for pl in pools)
    L.legion_group_destroy(grp)
    for pl in pools:
        pl.close()
    pools = [engine.MemoryPool(0, wl.N, batch, fanout, wl.D, replace=False) for _ in range(2)]
    for pl in pools:
        pl.alloc_features(pl.num_ids)
    arr = (ctypes.c_void_p * 2)(*[pl.handle for pl in pools])
    grp = L.legion_group_create(arr, 2)
    L.legion_enqueue_group(s, gpu.graph.handle, gpu.feature.handle, gpu.cache.handle, grp, batch, 0, 0, 0, fo, 2)
    torch.cuda.synchronize()
    for lane, pl in enumerate(pools):
        assert pl.error() == 0
        _compare(engine.read_batch(pl), _want(wl, 0, lane, 0, batch, fanout), wl, f"group lane {lane}: ")
        with pytest.raises(RuntimeError):
            pl.set_replace(True)                         # lane 1 as well as lane 0
    L.legion_group_destroy(grp)
    for pl in pools:
        pl.close()
    gpu.close()


# ---- end to end: the server binary with --sample-replace 0 and a trainer process --------------------------------------------------
@pytest.mark.parametrize("path", ["view", "slot"])
@pytest.mark.parametrize("disk", [False, True], ids=["in-memory", "disk"])
def test_server_binary_without_replacement(hip, tmp_path, monkeypatch, path, disk):
    """sampling_server --sample-replace 0 against tests/fake_trainer.py: every batch of two epochs and the validation and test
    batches, handed over as views of the lane arena or through pipe slots, in memory and in disk mode (hybrid tier), equal
    tests/distinct_ref.py's -- ids, labels, both cumulative offset blocks, block sizes and the rows, byte for byte."""
    import os
    import subprocess
    import sys
    from legion_amd import synth
    from tests.server_proc import start_server
    from tests.test_gpu_boundary import write_dataset
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    scale, D, B, fanout, epoch, cache_memory, cpu_cap, gpu_cap = 11, 24, 48, [5, 3], 2, 60_000, 260, 170
    indptr, col = synth.rmat_csr_numpy(scale, 8, 20231)
    N = indptr.size - 1
    feats = synth.features_numpy(0, N, D, 7)
    labels = (np.arange(N) % 47).astype(np.int32)
    perm = np.random.RandomState(3).permutation(N).astype(np.int32)
    train, valid, test = perm[:500], perm[500:590], perm[590:640]
    ds = str(tmp_path / "ds") + "/"
    write_dataset(ds, indptr, col, feats, labels, train, valid, test)
    work = tmp_path / "run"
    work.mkdir()
    fields = [ds, B, N, col.size, D, train.size, valid.size, test.size, cache_memory, epoch] + ([0, 0, 0, cpu_cap, gpu_cap] if disk else [])
    (work / "meta_config").write_text(" ".join(str(f) for f in fields))
    ns = f"_sd{os.getpid()}"
    monkeypatch.setenv("LEGION_IPC_NAMESPACE", ns)
    env = dict(os.environ)
    tenv = dict(env)
    if path == "slot":
        tenv["LEGION_NO_DIRECT_VIEWS"] = "1"
    argv = [os.path.join(root, "legion_amd", "bin", "sampling_server"), "1", "0"] + [str(f) for f in fanout] + \
        (["--disk"] if disk else []) + ["--sample-replace", "0"]
    server, log = start_server(argv, work, env, work / "server.log")
    try:
        st = ffi.Steps()
        L = ffi.load()
        one = lambda v: (ctypes.c_int32 * 1)(v)
        L.lgo_coordinate(ctypes.byref(st), 1, one(train.size), one(valid.size), one(test.size), B, epoch)
        out_npz = tmp_path / "trainer.npz"
        tr = subprocess.run([sys.executable, os.path.join(root, "tests", "fake_trainer.py"), "0", str(D), str(epoch), str(out_npz)],
                            env=tenv, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, stdin=subprocess.DEVNULL, text=True,
                            timeout=300)
        assert tr.returncode == 0, tr.stdout[-3000:] + "\n---- server ----\n" + open(work / "server.log").read()[-2000:]
        got = np.load(out_npz)
        assert got["steps"].tolist() == [st.train_step, st.valid_step, st.test_step]
        sets = {0: train, 1: valid, 2: test}
        total = L.lgo_max_step(ctypes.byref(st))
        H = len(fanout)
        for gb in range(total):
            mode = L.lgo_current_mode(ctypes.byref(st), gb)
            it = L.lgo_local_batch_id(ctypes.byref(st), gb)
            bs = L.lgo_current_batchsize(ctypes.byref(st), 0, mode)
            want = ref.run_batch(indptr, col, sets[mode], labels[sets[mode]], bs, it, fanout)
            nc, ec = want["node_counter"], want["edge_counter"]
            assert np.array_equal(got[f"b{gb}_ids"], want["sampled_ids"]), f"batch {gb} mode {mode}"
            assert np.array_equal(got[f"b{gb}_labels"], want["labels"]), f"batch {gb}"
            assert np.array_equal(got[f"b{gb}_feats"], feats[want["sampled_ids"]].view(np.uint32)), f"batch {gb} rows"
            for k, h in enumerate(range(H, 0, -1)):
                n_e = int(ec[9 + h])
                assert np.array_equal(got[f"b{gb}_src{k}"], want["agg_src_off"][:n_e]), f"batch {gb}"
                assert np.array_equal(got[f"b{gb}_dst{k}"], want["agg_dst_off"][:n_e]), f"batch {gb}"
            exp_sizes = []
            for h in range(H, 0, -1):
                exp_sizes += [int(nc[9 + h]), int(nc[9 + h - 1])]
            assert got[f"b{gb}_sizes"].tolist() == exp_sizes, f"batch {gb}"
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
