"""bench.py without --full (tools/bench_legs.py: parse_args, leg_report), host only: a plain run's line carries the headline figure and
what it was measured on; the profiled pass's figures (roofline, sampling_only, feature_gather_GBps) and the cache hit rates come with
--full only."""
import sys
import types

import numpy as np
import torch

from tools import bench_legs as legs


def parse(argv, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return legs.parse_args()


def report(args, world=1):
    G, steps, H, D = 4, 3, 2, 128
    n_timed = G * steps
    cache = types.SimpleNamespace(node_capacity=lambda d: 100, edge_capacity=lambda d: 7, replica_rows=lambda d: 0)
    counted = types.SimpleNamespace(hits=5, feat_hit_rows=30, feat_miss_rows=10, unique=None, tiers=None)
    timed = types.SimpleNamespace(repeats=1, region_s=np.array([0.03]))
    c = types.SimpleNamespace(graph_name="RMAT-18", epoch_batches=64, wrap=None, n_warm=G)
    rows = np.full((n_timed, H + 1), 10, dtype=np.int64)
    edges = np.full(n_timed, 50, dtype=np.int64)
    v = dict(B=1024, D=D, G=G, H=H, achieved=0.0, args=args, bulk=False, bytes_per_row=8 * D + 8, c=c, cache=cache, collective=None,
             counted=counted, counters=(0, 0), d=0, edges=edges, elapsed_max=0.03, elapsed_profiled=0.0, fanout=[25, 10], headline=True,
             hy_cpu=0, hy_gpu=0, last_op=3 * H + 1, lds_buckets=8, n_last=0, n_timed=n_timed, payload_gbps=0.0, pcie_tx=None,
             per_rank=None, replica_memory=0, rocprof_src=None, rocprof_us=None, rows=rows, rows_last=int(rows[:, H].sum()), samp_bytes=0.0,
             setup_s=1.0, shape_leg=False, state_bytes=64, stripe=False, t_all_gathers=0.0, t_last=0.0, t_sampling=0.03, timed=timed,
             topo_tx=0, tot_edges=torch.tensor([float(edges.sum())], dtype=torch.float64), traffic_committed=None,
             traffic_committed_src=None, train_step=8, weave=True, world=world, xgmi_tx=None)
    assert set(v) == legs.REPORT_NAMES
    return legs.leg_report(types.SimpleNamespace(**v))


def test_full_is_off_by_default(monkeypatch):
    assert parse(["--gpus", "1", "--steps", "3", "--warmup", "1"], monkeypatch).full is False
    assert parse(["--gpus", "1", "--steps", "3", "--warmup", "1", "--full"], monkeypatch).full is True
    # asking for a leg behind the headline (or for one to fail) asks for those legs
    assert parse(["--gpus", "1", "--cold-leg", "--no-boundary"], monkeypatch).full is True
    assert parse(["--gpus", "2", "--fail-extra-leg", "exit"], monkeypatch).full is True


def test_plain_line_is_the_headline(monkeypatch):
    out = report(parse(["--gpus", "1", "--steps", "3", "--warmup", "1"], monkeypatch))
    assert out["metric"] == "sampled_edges_per_sec" and out["unit"] == "edges/s" and out["higher_is_better"] is True
    assert out["dtype"] == "int32+f32(copy)" and out["steps"] == 3 and out["warmup"] == 1
    assert out["value"] == 12 * 50 / 0.03 and abs(out["ms_per_step"] - 10.0) < 1e-9
    assert out["edges_per_step"] == 200.0 and out["batches_per_step"] == 4 and "config" in out and "timed_region" in out
    for k in ("roofline", "sampling_only", "feature_gather_GBps", "feature_cache_hit_rate", "seed_feature_cache_hits_step0"):
        assert k not in out, k


def test_full_line_keeps_the_profiled_figures(monkeypatch):
    args = parse(["--gpus", "1", "--steps", "3", "--warmup", "1", "--full"], monkeypatch)
    plain = report(parse(["--gpus", "1", "--steps", "3", "--warmup", "1"], monkeypatch))
    out = report(args)
    for k in ("roofline", "sampling_only", "feature_gather_GBps", "feature_gather_GBps_note", "feature_cache_hit_rate",
              "feature_cache_hit_rate_over", "seed_feature_cache_hits_step0"):
        assert k in out, k
    assert out["feature_cache_hit_rate"] == 0.75 and out["roofline"]["rows_per_launch"] == 120
    assert {k: out[k] for k in plain} == plain                     # the plain line is the full line's headline part, unchanged
