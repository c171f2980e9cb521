"""bench.py --dump-outputs (tools/bench_legs.py: dump_outputs), host only: lanes of host tensors laid out as a Pipeline's pools are
written as the concatenation of what engine.read_batch would hand a caller, whole while it fits and as a seeded sample of positions
beyond that -- float64 / float32 only, within the byte budget, the same files from the same lanes."""
import glob
import os

import numpy as np
import torch

from tools import bench_legs as legs

FANOUT, D = [5, 3], 16


class Lane:
    """What dump_outputs reads of an engine.MemoryPool: `device`, `float_feature_len` and buffer(name) at the pool's shapes."""

    def __init__(self, rng, batch, N=1 << 20):
        self.device, self.float_feature_len = torch.device("cpu"), D
        num_ids = batch * (1 + FANOUT[0] + FANOUT[0] * FANOUT[1])
        seeds = int(rng.integers(1, batch + 1))
        nodes = int(rng.integers(seeds, num_ids + 1))
        edges = int(rng.integers(0, num_ids + 1))
        nc, ec = np.zeros(16, np.int32), np.zeros(16, np.int32)
        nc[8], nc[9], nc[9 + len(FANOUT)], ec[9 + len(FANOUT)] = len(FANOUT), seeds, nodes, edges
        ids = lambda n: torch.from_numpy(rng.integers(-1 << 30, 1 << 30, size=n, dtype=np.int32))    # (garbage past the counts)
        self.bufs = {"node_counter": torch.from_numpy(nc), "edge_counter": torch.from_numpy(ec), "labels": ids(batch),
                     "float_features": torch.from_numpy(rng.standard_normal((num_ids, D), dtype=np.float32))}
        for name in ("sampled_ids", "agg_src_off", "agg_dst_off", "agg_src_ids", "agg_dst_ids"):
            self.bufs[name] = ids(num_ids)
        self.counts = {"labels": seeds, "rows": nodes, "edges": edges}

    def buffer(self, name):
        return self.bufs[name]


def lanes(n, batch, seed=3):
    rng = np.random.default_rng(seed)
    return [Lane(rng, batch) for _ in range(n)]


def load(d):
    return {os.path.basename(f)[:-4]: np.load(f) for f in glob.glob(os.path.join(d, "*.npy"))}


def whole(pools, name, set_name):
    return np.concatenate([p.buffer(name)[:p.counts[set_name]].numpy() for p in pools])


def test_a_small_step_is_dumped_whole(tmp_path):
    pools = lanes(6, 32)
    legs.dump_outputs(str(tmp_path), pools, 40)
    out = load(tmp_path)
    assert all(a.dtype == (np.float32 if k == "float_features" else np.float64) for k, a in out.items())
    assert np.array_equal(out["batch_ids"], np.arange(40, 46))
    assert np.array_equal(out["node_counter"], np.stack([p.buffer("node_counter").numpy() for p in pools]))
    assert np.array_equal(out["edge_counter"], np.stack([p.buffer("edge_counter").numpy() for p in pools]))
    for set_name, arrays in legs.DUMP_SETS:
        assert np.array_equal(out[set_name + "_index"], np.arange(sum(p.counts[set_name] for p in pools)))
        for a in arrays:
            assert np.array_equal(out[a], whole(pools, a, set_name)), a


def test_a_large_step_is_a_seeded_sample_within_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(legs, "DUMP_BYTES", 1 << 20)
    pools = lanes(40, 256)
    written = legs.dump_outputs(str(tmp_path / "a"), pools, 0)
    assert written == sum(os.path.getsize(f) for f in glob.glob(str(tmp_path / "a" / "*.npy"))) <= 1 << 20
    out = load(tmp_path / "a")
    for set_name, arrays in legs.DUMP_SETS:
        pos = out[set_name + "_index"].astype(np.int64)
        total = sum(p.counts[set_name] for p in pools)
        assert 0 < pos.size and np.all(np.diff(pos) > 0) and pos[-1] < total
        for a in arrays:
            assert np.array_equal(out[a], whole(pools, a, set_name)[pos]), a
    assert out["rows_index"].size < sum(p.counts["rows"] for p in pools)         # (it was sampled)
    legs.dump_outputs(str(tmp_path / "b"), lanes(40, 256), 0)                   # the same lanes again
    again = load(tmp_path / "b")
    assert out.keys() == again.keys() and all(np.array_equal(out[k], again[k]) for k in out)
