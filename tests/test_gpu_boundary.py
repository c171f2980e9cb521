"""The drop-in boundary end to end: the `sampling_server` binary (meta_config + argv, dataset files in
the reference's formats, shm slab + semaphores + IPC handles) serving a fake trainer PROCESS that walks the
protocol of training_backend/legion_graphsage.py:72-128 through the `ipc_service` extension.  Every
batch the trainer sees is compared with the oracle (ids, features, labels, COO blocks, block sizes).
(The trainer end of most tests runs in a process of its own, one server life per process, as in a deployment;
test_one_trainer_process_outlives_eight_server_lives is the long-lived one.  In round 4 seventeen server lives attached to and
detached from the pytest process itself made a device-to-host copy of a freshly opened IPC buffer abort inside the HIP runtime
about once in four suite runs -- with finalize() leaving every arena it had ever mapped in place; DESIGN.md 4.6 has what round 5
found.)"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from legion_amd import synth
from oracle import ffi
from tests.server_proc import start_server

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write_dataset(path, wl_indptr, wl_col, feats, labels, train, valid, test):
    os.makedirs(path, exist_ok=True)
    wl_indptr.astype(np.int64).tofile(os.path.join(path, "edge_src"))
    wl_col.astype(np.int32).tofile(os.path.join(path, "edge_dst"))
    feats.astype(np.float32).tofile(os.path.join(path, "features"))
    labels.astype(np.int32).tofile(os.path.join(path, "labels"))
    train.astype(np.int32).tofile(os.path.join(path, "trainingset"))
    valid.astype(np.int32).tofile(os.path.join(path, "validationset"))
    test.astype(np.int32).tofile(os.path.join(path, "testingset"))


def check_trainer_batches(got, st, pool, g, cache, feats, sets, labels, fanout, D, epoch):
    """Every batch the trainer process dumped against the oracle's replay of the server's schedule."""
    import ctypes
    L = ffi.load()
    total = L.lgo_max_step(ctypes.byref(st))
    assert total == (st.train_step + st.valid_step) * epoch + st.test_step
    H = len(fanout)
    for gb in range(total):
        mode = L.lgo_current_mode(ctypes.byref(st), gb)
        it = L.lgo_local_batch_id(ctypes.byref(st), gb)
        bs = L.lgo_current_batchsize(ctypes.byref(st), 0, mode)
        pool.run_batch(g, cache, feats, sets[mode], labels[sets[mode]], bs, it, mode, False)
        want = pool.read_batch()
        nc, ec = want["node_counter"], want["edge_counter"]
        assert got[f"b{gb}_ntensors"] == 3 + 2 * H
        assert np.array_equal(got[f"b{gb}_ids"], want["sampled_ids"]), f"batch {gb}"
        assert np.array_equal(got[f"b{gb}_labels"], want["labels"])
        got_f = got[f"b{gb}_feats"]
        assert got_f.shape == (int(nc[9 + H]), D)
        if not np.array_equal(got_f, want["float_features"].view(np.uint32)):
            bad = np.nonzero((got_f != want["float_features"].view(np.uint32)).any(axis=1))[0]
            src_rows = [int(np.nonzero((feats.view(np.uint32) == got_f[r]).all(axis=1))[0][:1].sum()) for r in bad[:8]]
            raise AssertionError(f"batch {gb} mode {mode}: rows {bad[:20]} of {got_f.shape[0]} differ; ids there "
                                 f"{want['sampled_ids'][bad[:8]]}, rows actually hold features of {src_rows}; "
                                 f"node_map of those ids {cache.arr('node_map', np.int32)[want['sampled_ids'][bad[:8]]]}; "
                                 f"cap {cache.node_capacity} nc {nc[:12]}")
        for k, h in enumerate(range(H, 0, -1)):      # cumulative prefixes, outermost block first
            n_e = int(ec[9 + h])
            assert np.array_equal(got[f"b{gb}_src{k}"], want["agg_src_off"][:n_e])
            assert np.array_equal(got[f"b{gb}_dst{k}"], want["agg_dst_off"][:n_e])
        exp_sizes = []
        for h in range(H, 0, -1):
            exp_sizes += [int(nc[9 + h]), int(nc[9 + h - 1])]
        assert got[f"b{gb}_sizes"].tolist() == exp_sizes


@pytest.mark.parametrize("server_env", [
    {},                                                        # defaults: whole launch groups into the lane arena, batches handed over as VIEWS of their lane
    {"LEGION_RUNNER_LANES": "3"},                              # many small groups: three in flight, partial groups, mode changes mid-run, lane reuse
    {"LEGION_RUNNER_LANES": "1"},                              # one batch per group: a lane is reused as soon as its batch is released
    {"LEGION_RUNNER_LANES": "2", "LEGION_RUNNER_SLOTS": "2"},  # two groups in flight
    {"LEGION_RUNNER_LANES": "2", "LEGION_RUNNER_SLOTS": "4"},
    {"LEGION_NO_DIRECT_VIEWS": "1"},                           # a trainer end that does not take views: sampler phase in groups, one gather launch per batch into the pipe slot
    {"LEGION_NO_DIRECT_VIEWS": "1", "LEGION_RUNNER_LANES": "3"},
    {"LEGION_RUNNER_HANDOVER": "gather"},                      # gather hand-over for every trainer end (no arena published, lanes without feature buffers)
    {"LEGION_RUNNER_HANDOVER": "gather", "LEGION_RUNNER_LANES": "4", "LEGION_LDS_SMALL_BUCKETS": "16"},     # 16 de-duplication buckets per lane inside the server
    {"LEGION_RUNNER_HANDOVER": "gather", "LEGION_RUNNER_LANES": "1"},   # one batch per group
    {"LEGION_RUNNER_GRAPH": "0"},                              # the reference's operator-by-operator Runner
    {"LEGION_NO_SHM_MIRROR": "1"},                             # no mirror object at all: counters copied from the device, as the reference's trainer end does
    {"LEGION_RUNNER_HANDOVER": "gather", "LEGION_RUNNER_LANES": "5", "LEGION_RUNNER_HO_STREAM": "0"},   # hand-overs on the pipeline's own stream
    {"LEGION_RUNNER_HANDOVER": "gather", "LEGION_RUNNER_LANES": "6", "LEGION_RUNNER_HO_STREAM": "1"},   # one hand-over stream for both pipe slots
    {"LEGION_HOTNESS_REDUCE": "rccl"},                         # the clique sum of the access counters as the library's RCCL all-reduce (a 1-rank communicator here)
    {"LEGION_ARENA_SCATTER_MB": "0"},                          # the lane arena as ONE plain allocation, handed over as a hipIpcMemHandle (default: shuffled chunks, as file descriptors)
    {"LEGION_ARENA_SCATTER_MB": "0", "LEGION_RUNNER_LANES": "3"},
    {"_FANOUT": "4,3,2", "LEGION_RUNNER_LANES": "3"},          # three hops through the server (known lists across two hops, three gathers per group)
    {"_FANOUT": "2,2,2,2,2,2", "LEGION_RUNNER_LANES": "3"},    # six hops, the most the counter block holds: 15 tensors per batch at the trainer
], ids=["default-views", "views-lanes3", "views-lanes1", "views-lanes2-two-groups", "views-lanes2-four-groups", "trainer-without-views",
        "trainer-without-views-lanes3", "gather", "gather-lanes4-16-buckets", "gather-lanes1", "operators",
        "no-mirror", "gather-lanes5-one-stream", "gather-lanes6-shared-ho-stream", "rccl-hotness-reduce", "views-plain-arena", "views-plain-arena-lanes3", "views-three-hops", "views-six-hops"])
def test_server_binary_serves_fake_trainer(hip, tmp_path, server_env, monkeypatch):
    for k, v in server_env.items():
        if not k.startswith("_"):
            monkeypatch.setenv(k, v)

    scale, D, B, fanout, epoch, cache_memory = 11, 24, 48, [int(f) for f in server_env.get("_FANOUT", "5,3").split(",")], 2, 60_000
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
    (work / "meta_config").write_text("{} {} {} {} {} {} {} {} {} {}".format(
        ds, B, N, col.size, D, train.size, valid.size, test.size, cache_memory, epoch))
    ns = f"_t{os.getpid()}"
    monkeypatch.setenv("LEGION_IPC_NAMESPACE", ns)
    env = dict(os.environ)
    server, log = start_server([os.path.join(ROOT, "legion_amd", "bin", "sampling_server"), "1", "0"] + [str(f) for f in fanout],
                               work, env, work / "server.log")
    try:
        # ---- oracle replay of the whole server life: PreSC -> cache -> schedule ------------------
        g = ffi.OracleGraph(1, indptr, col)
        st = ffi.Steps()
        L = ffi.load()
        import ctypes
        one = lambda v: (ctypes.c_int32 * 1)(v)
        L.lgo_coordinate(ctypes.byref(st), 1, one(train.size), one(valid.size), one(test.size), B, epoch)
        node_acc, edge_acc = np.zeros(N, dtype=np.uint64), np.zeros(N, dtype=np.uint64)
        max_bs = max(B, st.valid_bs[0], st.test_bs[0])      # validation batches (90) exceed the raw batch (48)
        pool = ffi.OraclePool(N, max_bs, fanout, ffi.num_ids_for(max_bs, fanout), D)
        max_ids = 0
        for it in range(st.train_step):
            pool.run_batch(g, None, None, train, labels[train], B, it, 0, True, node_acc, edge_acc)
            max_ids = max(max_ids, int(pool.read_batch()["node_counter"][7]))
        cache = ffi.OracleCache(N, D, 1, 0)
        cache.candidate_selection([node_acc], [edge_acc])
        cache.cost_model(cache_memory, indptr, (0, 0), [max_ids], st.train_step)
        cache.fill_up(feats, indptr, col)
        g.attach_cache(cache)
        sets = {0: train, 1: valid, 2: test}

        # ---- the trainer's side of the protocol: a process of its own, as in a deployment (tests/fake_trainer.py walks
        #      initialize -> [get_next -> get_block_size -> synchronize] x schedule -> finalize and dumps what it was handed) ----------
        out_npz = tmp_path / "trainer.npz"
        tr = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fake_trainer.py"), "0", str(D), str(epoch), str(out_npz)],
                            env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, stdin=subprocess.DEVNULL, text=True, timeout=300)
        assert tr.returncode == 0, tr.stdout[-3000:] + "\n---- server ----\n" + open(work / "server.log").read()[-2000:]
        got = np.load(out_npz)
        assert got["steps"].tolist() == [st.train_step, st.valid_step, st.test_step]
        check_trainer_batches(got, st, pool, g, cache, feats, sets, labels, fanout, D, epoch)
        server.wait(timeout=60)
        assert server.returncode == 0
        text = open(work / "server.log").read()
        assert "Server Stopped" in text and "Train Steps: %d" % st.train_step in text
        # which hand-over served the run
        groups = server_env.get("LEGION_RUNNER_GRAPH") != "0"
        ho = server_env.get("LEGION_RUNNER_HANDOVER", "auto")
        views = groups and ho == "auto" and not ({"LEGION_NO_DIRECT_VIEWS", "LEGION_NO_SHM_MIRROR"} & set(server_env))
        want_kind = None if not groups else ("views of the lane arena" if views else "one gather launch per batch into the pipe slots")
        for kind in ("views of the lane arena", "one gather launch per batch into the pipe slots"):
            assert (("hand-over by " + kind) in text) == (kind == want_kind), text[-1500:]
        assert ("RCCL all-reduce (ncclUint64, ncclSum) over 1 GPU" in text) == (server_env.get("LEGION_HOTNESS_REDUCE") == "rccl"), text[-1500:]
    finally:
        if server.poll() is None:
            server.kill()
        log.close()
        for name in os.listdir("/dev/shm"):
            if name.endswith(ns):
                os.unlink(os.path.join("/dev/shm", name))


@pytest.mark.parametrize("server_env", [{}, {"LEGION_RUNNER_HANDOVER": "gather", "LEGION_RUNNER_LANES": "3"}, {"LEGION_RUNNER_GRAPH": "0"},
                                        {"LEGION_COL_SLOTS": "0", "LEGION_RUNNER_LANES": "2"}],
                         ids=["views", "gather-lanes3", "operators", "views-no-column-slots"])
def test_server_binary_in_disk_mode_serves_the_hybrid_tier(hip, tmp_path, server_env, monkeypatch):
    """`sampling_server ... --disk` = Run(fanout, gpu_number, in_memory_mode = 0, cache_mode) (sampling_server/sampling_server.cpp:7):
    a fifteen-field meta_config (SS/storage/storage_management.cu:60-94) whose last two fields size the hybrid CPU-cache /
    GPU-cache tier, built by UnifiedCache::HybridInit instead of CandidateSelection + CostModel + FillUp (the call the reference
    keeps commented out at SS/engine/server.cu:112).  Every batch a trainer process receives against the oracle's replay:
    rows from the GPU cache, from the mapped pinned CPU cache and (misses) from the feature table."""
    for k, v in server_env.items():
        monkeypatch.setenv(k, v)
    scale, D, B, fanout, epoch, cpu_cap, gpu_cap = 11, 24, 48, [5, 3], 2, 260, 170
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
    (work / "meta_config").write_text("{} {} {} {} {} {} {} {} {} {} {} {} {} {} {}".format(
        ds, B, N, col.size, D, train.size, valid.size, test.size, 60_000, epoch, 0, 0, 0, cpu_cap, gpu_cap))
    ns = f"_d{os.getpid()}"
    monkeypatch.setenv("LEGION_IPC_NAMESPACE", ns)
    env = dict(os.environ)
    server, log = start_server([os.path.join(ROOT, "legion_amd", "bin", "sampling_server"), "1", "0", "5", "3", "--disk"],
                               work, env, work / "server.log")
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
        for it in range(st.train_step):
            pool.run_batch(g, None, None, train, labels[train], B, it, 0, True, node_acc, edge_acc)
        cache = ffi.OracleCache(N, D, 1, 0)
        cache.hybrid_init(node_acc, feats, cpu_cap, gpu_cap)
        out_npz = tmp_path / "trainer.npz"
        tr = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fake_trainer.py"), "0", str(D), str(epoch), str(out_npz)],
                            env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, stdin=subprocess.DEVNULL, text=True, timeout=300)
        assert tr.returncode == 0, tr.stdout[-3000:] + "\n---- server ----\n" + open(work / "server.log").read()[-2000:]
        got = np.load(out_npz)
        check_trainer_batches(got, st, pool, g, cache, feats, {0: train, 1: valid, 2: test}, labels, fanout, D, epoch)
        # all three row sources were in play
        node_map = cache.arr("node_map", np.int32)
        slots = np.concatenate([node_map[got[f"b{gb}_ids"]] for gb in range(4)])
        assert ((slots >= 0) & (slots < cpu_cap)).any() and (slots >= cpu_cap).any() and (slots < 0).any()
        server.wait(timeout=60)
        assert server.returncode == 0
        text = open(work / "server.log").read()
        for needle in ("In Disk Mode", "CPU Cache Capacity: %d" % cpu_cap, "GPU Cache Capacity: %d" % gpu_cap, "Finish initializing cache",
                       "System is ready for serving", "Server Stopped"):
            assert needle in text, needle
        assert "Alpha:" not in text                     # the cost model did not run
    finally:
        if server.poll() is None:
            server.kill()
        log.close()
        for name in os.listdir("/dev/shm"):
            if name.endswith(ns):
                os.unlink(os.path.join("/dev/shm", name))


def test_server_in_disk_mode_rejects_a_ten_field_meta_config(hip, tmp_path):
    indptr, col = synth.rmat_csr_numpy(9, 4, 20231)
    N = indptr.size - 1
    ds = str(tmp_path / "ds") + "/"
    perm = np.arange(N, dtype=np.int32)
    write_dataset(ds, indptr, col, synth.features_numpy(0, N, 4, 7), np.zeros(N, dtype=np.int32), perm[:100], perm[100:120], perm[120:130])
    work = tmp_path / "run"
    work.mkdir()
    (work / "meta_config").write_text("{} {} {} {} {} {} {} {} {} {}".format(ds, 16, N, col.size, 4, 100, 20, 10, 50_000, 1))
    ns = f"_e{os.getpid()}"
    res = subprocess.run([os.path.join(ROOT, "legion_amd", "bin", "sampling_server"), "1", "0", "5", "3", "--disk"], cwd=work,
                         env=dict(os.environ, LEGION_IPC_NAMESPACE=ns), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         stdin=subprocess.DEVNULL, text=True, timeout=300)
    for name in os.listdir("/dev/shm"):
        if name.endswith(ns):
            os.unlink(os.path.join("/dev/shm", name))
    assert res.returncode != 0 and "disk mode needs fifteen fields" in res.stdout, res.stdout[-2000:]


@pytest.mark.parametrize("damage,needle", [("short_edge_dst", "file too short"), ("edge_count", "data set mismatch"),
                                           ("seed_range", "data set mismatch"), ("missing_edge_src", "cannout open file")])
def test_server_rejects_a_mismatched_dataset(hip, tmp_path, damage, needle):
    """A data set that does not match meta_config (truncated file, wrong edge count, seed ids beyond N, missing CSR) makes
    the server say so and exit non-zero -- it neither zero-fills nor reads out of bounds (the reference mmaps and reads on)."""
    scale, D, B = 10, 8, 32
    indptr, col = synth.rmat_csr_numpy(scale, 8, 20231)
    N = indptr.size - 1
    feats = synth.features_numpy(0, N, D, 7)
    labels = (np.arange(N) % 47).astype(np.int32)
    perm = np.random.RandomState(3).permutation(N).astype(np.int32)
    train, valid, test = perm[:200], perm[200:240], perm[240:260]
    if damage == "seed_range":
        train = train.copy(); train[17] = N + 5
    ds = str(tmp_path / "ds") + "/"
    write_dataset(ds, indptr, col, feats, labels, train, valid, test)
    E = col.size
    if damage == "short_edge_dst":
        col[: E - 100].astype(np.int32).tofile(os.path.join(ds, "edge_dst"))
    if damage == "edge_count":
        E = E - 64                                      # meta_config disagrees with edge_src[N]
    if damage == "missing_edge_src":
        os.unlink(os.path.join(ds, "edge_src"))
    work = tmp_path / "run"
    work.mkdir()
    (work / "meta_config").write_text("{} {} {} {} {} {} {} {} {} {}".format(
        ds, B, N, E, D, train.size, valid.size, test.size, 50_000, 1))
    ns = f"_r{os.getpid()}"
    res = subprocess.run([os.path.join(ROOT, "legion_amd", "bin", "sampling_server"), "1", "0", "5", "3"], cwd=work,
                         env=dict(os.environ, LEGION_IPC_NAMESPACE=ns), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         stdin=subprocess.DEVNULL, text=True, timeout=300)
    for name in os.listdir("/dev/shm"):
        if name.endswith(ns):
            os.unlink(os.path.join("/dev/shm", name))
    assert res.returncode != 0 and needle in res.stdout, res.stdout[-2000:]
    assert "System is ready for serving" not in res.stdout


def test_vmm_fd_convention_probe_under_both_runtimes(hip):
    """How hipMemImportFromShareableHandle takes a POSIX file descriptor differs between the two HIP runtimes of this image --
    ROCm 7.2's (what a build of the trainer end against /opt/rocm would run on) takes the value, the one bundled with torch
    2.10+rocm7.0 (what `ipc_service` runs on inside a trainer) a pointer, and the wrong one is a segmentation fault.  Round 4
    guessed from hipRuntimeGetVersion(); the probe (legion_amd/trainer/vmm_probe.h) finds out without being able to crash, and
    is run here under both (ADVICE r04 / VERDICT r04 item 2)."""
    probe = os.path.join(ROOT, "legion_amd", "bin", "vmm_convention_probe")
    res = subprocess.run([probe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, stdin=subprocess.DEVNULL)
    assert res.returncode == 0 and "convention 1 " in res.stdout, res.stdout          # ROCm 7.2: by value
    code = ("import sys, torch; sys.path.insert(0, %r); import ipc_service; torch.cuda.set_device(0); torch.zeros(1, device='cuda:0'); "
            "print('convention', ipc_service.vmm_fd_convention(), 'hip', torch.version.hip)" % os.path.join(ROOT, "legion_amd", "trainer"))
    res = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300, stdin=subprocess.DEVNULL)
    assert res.returncode == 0 and "convention 0 " in res.stdout, res.stdout          # torch's bundled runtime: by pointer


def test_one_trainer_process_outlives_eight_server_lives(hip, tmp_path):
    """a single long-lived trainer process -- initialize -> the whole schedule (100+ batches, every one compared
    with the oracle here, by digest) -> finalize, eight server lives in a row, batches as views of the chunked lane arena (tens of
    MB) -- with the GPU's free memory back at its level after every life: finalize() unmaps and releases what initialize() mapped
    (TB/ipc_cuda_kernel.cu:140-156 closes what it opened), so a trainer that outlives a server no longer pins its arena."""
    import hashlib
    scale, D, B, fanout, epoch, cache_memory, lives = 13, 256, 48, [5, 3], 1, 600_000, 8
    indptr, col = synth.rmat_csr_numpy(scale, 8, 20231)
    N = indptr.size - 1
    feats = synth.features_numpy(0, N, D, 7)
    labels = (np.arange(N) % 47).astype(np.int32)
    perm = np.random.RandomState(3).permutation(N).astype(np.int32)
    train, valid, test = perm[:5000], perm[5000:5090], perm[5090:5140]
    ds = str(tmp_path / "ds") + "/"
    write_dataset(ds, indptr, col, feats, labels, train, valid, test)
    work = tmp_path / "run"
    work.mkdir()
    (work / "meta_config").write_text("{} {} {} {} {} {} {} {} {} {}".format(
        ds, B, N, col.size, D, train.size, valid.size, test.size, cache_memory, epoch))
    ns = f"_l{os.getpid()}"
    env = dict(os.environ, LEGION_IPC_NAMESPACE=ns)
    for k in ("LEGION_NO_DIRECT_VIEWS", "LEGION_NO_SHM_MIRROR", "LEGION_RUNNER_HANDOVER", "LEGION_ARENA_SCATTER_MB"):
        env.pop(k, None)
    try:
        res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "long_lived_trainer.py"), str(lives), str(D), str(epoch), str(work)] +
                             [str(f) for f in fanout], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                             stdin=subprocess.DEVNULL, timeout=560)
        logs = "".join(open(work / f).read()[-1200:] for f in sorted(os.listdir(work)) if f.startswith("server"))
        assert res.returncode == 0 and "all lives clean" in res.stdout, res.stdout[-4000:] + "\n---- servers ----\n" + logs[-3000:]
        # (where descriptors of device memory cross no process boundary the server's arena is a plain allocation, opened by its IPC handle)
        from legion_amd import engine
        attached = "chunks): batches arrive as views" if engine.fd_handover_works() else "MiB): batches arrive as views"
        assert "hand-over by views of the lane arena" in logs and attached in res.stdout, res.stdout[-2000:]
        # ---- the oracle's batches of one server life (every life serves the same schedule) ----
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
        cache.candidate_selection([node_acc], [edge_acc])
        cache.cost_model(cache_memory, indptr, (0, 0), [max_ids], st.train_step)
        cache.fill_up(feats, indptr, col)
        g.attach_cache(cache)
        sets = {0: train, 1: valid, 2: test}
        total = L.lgo_max_step(ctypes.byref(st))
        assert total >= 100
        H = len(fanout)
        dig = lambda a: int.from_bytes(hashlib.blake2b(np.ascontiguousarray(a).tobytes(), digest_size=8).digest(), "little")
        wants = []
        for gb in range(total):
            mode = L.lgo_current_mode(ctypes.byref(st), gb)
            it = L.lgo_local_batch_id(ctypes.byref(st), gb)
            bs = L.lgo_current_batchsize(ctypes.byref(st), 0, mode)
            pool.run_batch(g, cache, feats, sets[mode], labels[sets[mode]], bs, it, mode, False)
            w = pool.read_batch()
            nc, ec = w["node_counter"], w["edge_counter"]
            row = [dig(w["sampled_ids"]), dig(w["float_features"].view(np.uint32)), dig(w["labels"])]
            for h in range(H, 0, -1):
                row += [dig(w["agg_src_off"][:int(ec[9 + h])]), dig(w["agg_dst_off"][:int(ec[9 + h])])]
            sizes = []
            for h in range(H, 0, -1):
                sizes += [int(nc[9 + h]), int(nc[9 + h - 1])]
            wants.append((row, sizes))
        for life in range(lives):
            got = np.load(work / f"life{life}.npz")
            assert got["steps"].tolist() == [st.train_step, st.valid_step, st.test_step]
            for gb, (row, sizes) in enumerate(wants):
                assert got["digests"][gb].tolist() == [np.uint64(v) for v in row], f"life {life} batch {gb}: what the trainer was handed differs from the oracle's batch"
                assert got["sizes"][gb].tolist() == sizes, f"life {life} batch {gb}"
    finally:
        for name in os.listdir("/dev/shm"):
            if name.endswith(ns):
                os.unlink(os.path.join("/dev/shm", name))


def _hub_validation_dataset(tmp_path, B):
    """Training seeds: the graph's lowest-degree vertices (a batch of 16 has a few dozen ids); the validation seeds: its 400 hubs
    (thousands of ids per batch): validation batches outgrow lane feature buffers sized 1.2 x the largest TRAINING batch."""
    scale, D = 14, 8
    indptr, col = synth.rmat_csr_numpy(scale, 8, 20231)
    N = indptr.size - 1
    feats = synth.features_numpy(0, N, D, 7)
    labels = (np.arange(N) % 47).astype(np.int32)
    by_deg = np.argsort(np.diff(indptr), kind="stable").astype(np.int32)
    train, valid, test = by_deg[:100], by_deg[-400:], by_deg[2000:2020]
    ds = str(tmp_path / "ds") + "/"
    write_dataset(ds, indptr, col, feats, labels, train, valid, test)
    work = tmp_path / "run"
    work.mkdir()
    (work / "meta_config").write_text("{} {} {} {} {} {} {} {} {} {}".format(
        ds, B, N, col.size, D, train.size, valid.size, test.size, 50_000, 1))
    return work, (indptr, col, feats, labels, train, valid, test, N, D)


@pytest.mark.parametrize("server_env", [{"LEGION_RUNNER_LANES": "4"}, {"LEGION_RUNNER_LANES": "1"},
                                        {"LEGION_RUNNER_LANES": "4", "LEGION_NO_DIRECT_VIEWS": "1"},
                                        {"LEGION_RUNNER_LANES": "4", "LEGION_RUNNER_HANDOVER": "gather"},
                                        {"LEGION_RUNNER_GRAPH": "0"}],
                         ids=["views-lanes4", "views-lanes1", "trainer-without-views", "gather", "operators"])
def test_oversized_validation_batch_is_served_whole_from_the_overflow_buffer(hip, tmp_path, server_env):
    """with the views hand-over a batch with more rows than its lane's feature buffer used to stop the server --
    and validation / test seeds with heavier neighbourhoods than the training batches PreSC saw do that on real data sets.  Now the
    batch's rows are gathered once more, all of them, into the pipe slot's overflow buffer inside the arena and the view of its rows
    points there: every batch of the schedule reaches the trainer and equals the oracle's, rows included.  The other hand-overs --
    a trainer end that does not take views, the forced gather hand-over, the operator-by-operator Runner -- gather into the two pipe
    slots' own buffers, which hold the worst case of a batch (num_ids rows) since round 6: whole batches there too, where the
    reference's 1.2 x buffers overrun (SS/engine/server.cu:277)."""
    B, fanout, epoch = 16, [5, 3], 1
    work, (indptr, col, feats, labels, train, valid, test, N, D) = _hub_validation_dataset(tmp_path, B)
    ns = f"_o{os.getpid()}"
    env = dict(os.environ, LEGION_IPC_NAMESPACE=ns, **server_env)
    views = not ({"LEGION_NO_DIRECT_VIEWS", "LEGION_RUNNER_HANDOVER", "LEGION_RUNNER_GRAPH"} & set(server_env))
    server, log = start_server([os.path.join(ROOT, "legion_amd", "bin", "sampling_server"), "1", "0"] + [str(f) for f in fanout],
                               work, env, work / "server.log")
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
        cache.candidate_selection([node_acc], [edge_acc])
        cache.cost_model(50_000, indptr, (0, 0), [max_ids], st.train_step)
        cache.fill_up(feats, indptr, col)
        g.attach_cache(cache)
        out_npz = tmp_path / "trainer.npz"
        tr = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fake_trainer.py"), "0", str(D), str(epoch), str(out_npz)],
                            env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, stdin=subprocess.DEVNULL, text=True, timeout=300)
        assert tr.returncode == 0, tr.stdout[-3000:] + "\n---- server ----\n" + open(work / "server.log").read()[-2000:]
        got = np.load(out_npz)
        check_trainer_batches(got, st, pool, g, cache, feats, {0: train, 1: valid, 2: test}, labels, fanout, D, epoch)
        server.wait(timeout=60)
        text = open(work / "server.log").read()
        assert server.returncode == 0 and "Server Stopped" in text, text[-2000:]
        # the validation batches really were larger than what a lane holds, and they went out through the overflow buffers
        lane_rows = int(max_ids * 1.2) * ((max_bs + B - 1) // B)
        n_over = sum(int(got[f"b{gb}_ids"].size) > lane_rows for gb in range(st.train_step + st.valid_step + st.test_step))
        assert n_over >= 1
        if views:
            assert "handed over from the pipe slot's overflow buffer" in text
            assert f"{n_over} batches handed over from an overflow buffer" in text, text[-1500:]
        else:
            assert "overflow buffer" not in text and "tail rows were not gathered" not in text, text[-1500:]
    finally:
        if server.poll() is None:
            server.kill()
        log.close()
        for name in os.listdir("/dev/shm"):
            if name.endswith(ns):
                os.unlink(os.path.join("/dev/shm", name))


def test_server_stops_instead_of_posting_a_corrupt_batch(hip, tmp_path):
    """Device-side corruption ends the server before IPCPost (include/legion_hip.h error convention; the reference's
    cudaCheckError).  Forced here with LEGION_RUNNER_OVERFLOW=0 (no overflow buffers): a validation batch whose rows do not fit its
    lane's buffer (LG_ERR_FEATURE_ROWS) cannot go out as a VIEW -- a view with more rows than the buffer behind it would show the
    trainer the next lane's arrays as rows.  The PreSC epoch and the training batches are served; the validation batch is
    not posted, the server exits non-zero and wakes the trainer blocked on its semaphore.  (A trainer end that gets its rows gathered
    into the pipe slot's own buffer is served the rows that fit, with a warning: the reference overruns there, SS/engine/server.cu:277.)"""
    B, fanout = 16, [5, 3]
    work, (indptr, col, feats, labels, train, valid, test, N, D) = _hub_validation_dataset(tmp_path, B)
    ns = f"_c{os.getpid()}"
    env = dict(os.environ, LEGION_IPC_NAMESPACE=ns, LEGION_RUNNER_LANES="4", LEGION_RUNNER_OVERFLOW="0")
    server, log = start_server([os.path.join(ROOT, "legion_amd", "bin", "sampling_server"), "1", "0"] + [str(f) for f in fanout],
                               work, env, work / "server.log")
    trainer = subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "fake_trainer.py"), "0", str(D), "1", str(work / "out.npz")],
                               env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, stdin=subprocess.DEVNULL)
    try:
        server.wait(timeout=240)
        text = open(work / "server.log").read()
        assert server.returncode not in (0, None), text[-2000:]
        assert "more rows than the feature buffer" in text and "not posted" in text and "Server Stopped" not in text, text[-2000:]
        assert not os.path.exists(work / "out.npz")          # the trainer never got the whole schedule
        # ... and it does not hang on the semaphore of the batch that never came: the server woke it before it went
        t_out = trainer.communicate(timeout=60)[0].decode()
        assert trainer.returncode not in (0, None) and "the sampling server stopped on an error" in t_out, t_out[-1500:]
        left = [n for n in os.listdir("/dev/shm") if n.endswith(ns)]
        assert not [n for n in left if n.startswith(("simpleIPCshm", "legionIPCext", "sem.sem_w", "sem.sem_r"))], left
    finally:
        if server.poll() is None:
            server.kill()
        if trainer.poll() is None:
            trainer.kill()
        trainer.wait()
        log.close()
        for name in os.listdir("/dev/shm"):
            if name.endswith(ns):
                os.unlink(os.path.join("/dev/shm", name))


@pytest.mark.parametrize("lanes,handover", [("16", "auto"), ("5", "auto"), ("16", "gather"), ("5", "gather")])
def test_boundary_soak_every_batch_verified(hip, lanes, handover):
    """600+ consecutive hand-overs through the binary and the two pipe slots with a consumer that checks EVERY batch on the
    device (rows = the generator's rows of the batch's ids, unique ids, edge endpoints inside the batch, the seeds are the
    training batch's): a wrong slot, a stale or half-copied batch, a lost or duplicated post shows up here."""
    import json
    env = dict(os.environ, LEGION_RUNNER_LANES=lanes, LEGION_RUNNER_HANDOVER=handover)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "server_throughput.py"), "--scale", "16", "--batch", "100",
                          "--dim", "32", "--fanout", "6,4", "--train-batches", "620", "--verify-every", "1", "--watchdog", "150",
                          "--cache-memory", str(1 << 20)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         stdin=subprocess.DEVNULL, timeout=400)
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert res.returncode == 0 and lines, (res.stdout[-1500:], res.stderr[-3000:])
    d = json.loads(lines[-1])
    assert d["verified_batches"] >= 620 and d["batches_per_sec"] > 0


@pytest.mark.timeout(1500)
def test_server_loads_a_uk_union_sized_dataset(hip):
    """The reference's file formats at uk-union's REAL size through the server's own loaders (SS/storage/
    storage_management_impl.cuh:46-159; legion_server.py:65-72): N = 133 633 040, E = 5 507 679 822 -- an `edge_dst` file of
    22 GB (> 16 GiB, > 2^32 entries), `edge_src` offsets beyond 2^32 -- written to /tmp, loaded into HBM by `sampling_server`,
    PreSC + cache set-up, then every served batch verified on the device by the consumer (rows = the generator's rows of
    the batch's ids, unique ids, edge endpoints inside the batch, the seeds are the training batch's).  D = 4 keeps the
    features file at 2 GB; what is under test is everything that scales with E."""
    import json
    import shutil
    if shutil.disk_usage("/tmp").free < (40 << 30):
        pytest.skip("needs 40 GB of free space in /tmp for the data set files")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "server_throughput.py"), "--nodes", "133633040",
                          "--edges", "5507679822", "--batch", "8000", "--dim", "4", "--fanout", "25,10", "--train-batches", "12",
                          "--verify-every", "1", "--watchdog", "1200", "--cache-memory", str(1 << 30)],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, stdin=subprocess.DEVNULL, timeout=1400)
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert res.returncode == 0 and lines, (res.stdout[-1500:], res.stderr[-3000:])
    d = json.loads(lines[-1])
    assert d["verified_batches"] >= 12 and d["edges_per_sec"] > 0 and "E=5507679822" in d["workload"]
