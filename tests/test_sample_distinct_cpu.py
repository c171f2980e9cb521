"""Sampling without replacement without a GPU: the numpy reference (tests/distinct_ref.py) against a slow pure-Python
statement, the invariants of the picks, their subset distribution, the launcher's --sample_replace, the binary's
--sample-replace parsing and the new C entry points."""
import os
import re
import stat
import subprocess

import numpy as np
import pytest

from legion_amd import launcher
from oracle import ffi
from tests import distinct_ref as ref
from tests.test_oracle_sampler import tiny_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "legion_hip.h")
LIB = os.path.join(ROOT, "legion_amd", "liblegion_hip.so")
BINARY = os.path.join(ROOT, "legion_amd", "bin", "sampling_server")
NEW_SYMBOLS = ("legion_pool_set_sample_replace", "legion_pool_sample_replace", "legion_pipeline_set_sample_replace",
               "legion_server_set_sample_replace", "legion_draw_distinct_batch")


def py_picks(q, f, D):
    """One entry's picks, slot by slot, with the oracle's own draw."""
    L = ffi.load()
    if D <= f:
        return list(range(D))
    out = []
    for k in range(f):
        j = D - f + k
        t = int(L.lgo_draw(q * f + k, j + 1))
        out.append(j if t in out else t)
    return out


def py_batch(indptr, col, seeds, fanout):
    """Distinct mode in plain Python, slot order (tests/test_oracle_sampler.py py_batch with the picks swapped)."""
    ids = list(seeds)
    pos = {v: i for i, v in enumerate(seeds)}
    es, ed = [], []
    frontier = list(seeds)
    ncum, ecum = [len(ids)], [0]
    for f in fanout:
        new = []
        for q, s in enumerate(frontier):
            deg = int(indptr[s + 1] - indptr[s]) if s >= 0 else 0
            for p in py_picks(q, f, deg):
                d = int(col[indptr[s] + p])
                if d not in pos:
                    pos[d] = len(ids)
                    ids.append(d)
                new.append((d, s))
        es += [e[0] for e in new]
        ed += [e[1] for e in new]
        frontier = [e[0] for e in new]
        ncum.append(len(ids))
        ecum.append(len(es))
    return ids, es, ed, [pos[v] for v in es], [pos[v] for v in ed], ncum, ecum


def _check_against_py(indptr, col, seeds, fanout):
    got = ref.run_batch(indptr, col, seeds, np.zeros_like(seeds), len(seeds), 0, fanout)
    ids, es, ed, so, do, ncum, ecum = py_batch(indptr, col, seeds.tolist(), fanout)
    assert got["sampled_ids"].tolist() == ids
    assert got["agg_src_ids"].tolist() == es and got["agg_dst_ids"].tolist() == ed
    assert got["agg_src_off"].tolist() == so and got["agg_dst_off"].tolist() == do
    h = len(fanout)
    assert got["node_counter"][9:9 + h + 1].tolist() == ncum
    assert got["edge_counter"][9:9 + h + 1].tolist() == ecum
    assert got["node_counter"][8] == h


def test_vectorised_draw_is_the_oracle_draw():
    L = ffi.load()
    rng = np.random.RandomState(5)
    idx = rng.randint(0, 2**31 - 1, 4000)
    n = rng.randint(1, 2**30, 4000)
    idx[:4] = [0, 1, 2**31 - 2, 4194303]
    n[:4] = [1, 2**30, 7, 1000000]
    assert ref.draw(idx, n).tolist() == [int(L.lgo_draw(int(a), int(b))) for a, b in zip(idx, n)]


@pytest.mark.parametrize("fanout", [[3, 2], [25, 10], [2, 2, 2], [1], [4, 1, 3], [2, 2, 2, 2, 2, 2]])
def test_reference_against_python_on_tiny_graph(fanout):
    indptr, col = tiny_graph()
    _check_against_py(indptr, col, np.array([0, 6, 7, 3], dtype=np.int32), fanout)


def test_reference_against_python_on_random_graphs():
    hypothesis = pytest.importorskip("hypothesis")
    st = hypothesis.strategies

    @hypothesis.settings(max_examples=40, deadline=None)
    @hypothesis.given(n=st.integers(2, 40), seed=st.integers(0, 2**31 - 1),
                      fanout=st.lists(st.integers(1, 8), min_size=1, max_size=6))
    def run(n, seed, fanout):
        rng = np.random.RandomState(seed)
        deg = rng.randint(0, 12, n)
        indptr = np.zeros(n + 1, np.int64); np.cumsum(deg, out=indptr[1:])
        col = rng.randint(0, n, int(indptr[-1])).astype(np.int32)
        seeds = rng.permutation(n)[:max(1, n // 3)].astype(np.int32)
        hop_cap = len(seeds)
        for f in fanout:
            hop_cap *= f
        hypothesis.assume(hop_cap <= 20000)
        _check_against_py(indptr, col, seeds, fanout)
    run()


@pytest.mark.parametrize("f", [1, 2, 3, 10, 25, 40])
def test_picks_are_distinct_and_all_neighbours_when_deg_fits(f):
    deg = np.array([0, 1, f - 1, f, f + 1, 2 * f, 1000, 10**6, 2**30] * 30, dtype=np.int64)
    base = np.arange(deg.size, dtype=np.int64) * f + 12345
    P = ref.picks(base, deg, f)
    for q in range(deg.size):
        D = int(deg[q])
        row = P[q]
        valid = row[row >= 0]
        assert valid.size == min(f, D)
        assert np.all(row[valid.size:] == -1)
        if D <= f:
            assert valid.tolist() == list(range(D))
        else:
            assert np.unique(valid).size == f and valid.min() >= 0 and valid.max() < D
    for q in range(0, deg.size, 7):                  # the slow statement agrees
        assert [int(v) for v in P[q] if v >= 0] == py_picks_at(int(base[q]), f, int(deg[q]))


def py_picks_at(base, f, D):
    L = ffi.load()
    if D <= f:
        return list(range(D))
    out = []
    for k in range(f):
        j = D - f + k
        t = int(L.lgo_draw(base + k, j + 1))
        out.append(j if t in out else t)
    return out


@pytest.mark.parametrize("D,f,crit", [(4, 2, 20.5), (5, 3, 27.9), (3, 2, 13.8)])
def test_subset_chi_square(D, f, crit):
    """Consecutive frontier entries give every f-subset of [0, D) equally often (critical values: p = 0.001)."""
    from itertools import combinations
    n = 60000
    P = ref.picks(np.arange(n, dtype=np.int64) * f, np.full(n, D), f)
    subsets = {c: i for i, c in enumerate(combinations(range(D), f))}
    counts = np.bincount([subsets[tuple(sorted(r))] for r in P.tolist()], minlength=len(subsets))
    e = n / len(subsets)
    chi2 = float(((counts - e) ** 2 / e).sum())
    assert chi2 < crit, (chi2, counts)


def test_each_hop_has_sum_min_f_d_edges():
    from legion_amd import synth
    indptr, col = synth.rmat_csr_numpy(10, 8, 20231)
    seeds = np.random.RandomState(1).permutation(indptr.size - 1)[:64].astype(np.int32)
    fanout = [5, 3]
    b = ref.run_batch(indptr, col, seeds, np.zeros_like(seeds), 64, 0, fanout)
    nc, ec = b["node_counter"], b["edge_counter"]
    frontier, lo = b["sampled_ids"][:int(nc[9])], 0
    for h, f in enumerate(fanout):
        hi = int(ec[9 + h + 1])
        deg = indptr[frontier.astype(np.int64) + 1] - indptr[frontier.astype(np.int64)]
        assert hi - lo == int(np.minimum(deg, f).sum())
        frontier, lo = b["agg_src_ids"][lo:hi], hi


def _run_launcher(tmp_path, monkeypatch, extra):
    fake = tmp_path / "fake_server"
    record = tmp_path / "argv.txt"
    fake.write_text('#!/bin/sh\nfor a in "$0" "$@"; do echo "$a"; done > %s\nexit 0\n' % record)
    fake.chmod(fake.stat().st_mode | stat.S_IEXEC)
    monkeypatch.setattr(launcher, "server_binary", lambda: str(fake))
    monkeypatch.chdir(tmp_path)
    args = launcher.build_argparser().parse_args(["--dataset_name", "products", "--usenvlink", "0"] + extra)
    assert launcher.Run(args) == 0
    return record.read_text().split("\n")[:-1], (tmp_path / "meta_config").read_text(), str(fake)


def test_launcher_default_leaves_the_launch_unchanged(tmp_path, monkeypatch):
    argv, meta, fake = _run_launcher(tmp_path, monkeypatch, ["--sample_replace", "1"])
    assert argv == [fake, "2", "0", "25", "10"]
    assert meta == launcher.meta_config_line("./dataset", "products", 8000, 38000000, 2)
    assert launcher.build_argparser().parse_args([]).sample_replace == 1


def test_launcher_without_replacement_adds_the_binary_flag(tmp_path, monkeypatch):
    argv, meta, fake = _run_launcher(tmp_path, monkeypatch, ["--sample_replace", "0", "--fanout", "15,10,5"])
    assert argv == [fake, "2", "0", "15", "10", "5", "--sample-replace", "0"]
    assert meta == launcher.meta_config_line("./dataset", "products", 8000, 38000000, 2)


@pytest.mark.parametrize("bad", ["2", "-1", "true", ""])
def test_launcher_rejects_a_bad_value(bad):
    with pytest.raises(SystemExit):
        launcher.build_argparser().parse_args(["--sample_replace", bad])


def test_new_symbols_declared_exported_and_typed():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    from legion_amd import lib
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} not declared in legion_hip.h"
        assert name in exported, f"{name} not exported"
        assert name in lib.SIGNATURES, f"{name} not in lib.SIGNATURES"


def test_setters_refuse_without_a_device():
    from legion_amd import lib
    L = lib.load()
    for bad in (2, -1, 7):
        assert L.legion_server_set_sample_replace(bad) == -1
        assert L.legion_pool_set_sample_replace(None, bad) == -1
        assert L.legion_pipeline_set_sample_replace(None, bad) == -1
    assert L.legion_server_set_sample_replace(0) == 0
    assert L.legion_server_set_sample_replace(1) == 0          # back to the default for this process
    assert L.legion_pool_set_sample_replace(None, 0) == -1     # no pool
    assert L.legion_pool_sample_replace(None) == -1
    for f in (0, -3, 257):
        assert L.legion_draw_distinct_batch(None, None, None, f, None, 1) == -1


def test_engine_rejects_a_bad_replace():
    from legion_amd import engine
    with pytest.raises(ValueError):
        engine.MemoryPool.set_replace(engine.MemoryPool.__new__(engine.MemoryPool), 2)


@pytest.mark.parametrize("value", ["2", "", "yes", "-1"])
def test_server_binary_rejects_a_bad_value_before_touching_a_device(value):
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "legion_amd") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    p = subprocess.run([BINARY, "1", "0", "--sample-replace", value], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       env=env, timeout=60)
    assert p.returncode == 2, p.stdout
    assert b"--sample-replace: expected 0 or 1" in p.stdout


def test_usage_line_names_the_flag():
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "legion_amd") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    p = subprocess.run([BINARY], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, timeout=60)
    assert p.returncode == 2 and b"[--sample-replace 0|1]" in p.stdout
