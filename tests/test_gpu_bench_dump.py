"""bench.py --steps / --dump-outputs on the GPU: the default run times exactly --steps steps once, and what the last timed step handed
its caller is written out -- the same files from two runs of the same command, every gathered row the generator's row of its id, every
edge an edge of the graph."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from legion_amd import synth
from tools import bench_legs as legs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE, EF, G, B = 18, 16, 8, 1024
CMD = ["--gpus", "1", "--scale", str(SCALE), "--edge-factor", str(EF), "--group", str(G), "--batch", str(B), "--presc-steps", "8",
       "--cpu-seconds", "0", "--no-boundary", "--steps", "3", "--warmup", "1", "--cache-memory", str(64 << 20)]


def run_dump(out_dir):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + CMD + ["--dump-outputs", str(out_dir)], cwd=ROOT,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0]), {os.path.basename(f)[:-4]: np.load(f) for f in glob.glob(os.path.join(out_dir, "*.npy"))}


def test_exact_steps_and_the_last_steps_outputs(hip, tmp_path):
    d, out = run_dump(tmp_path / "a")
    assert d["steps"] == 3 and d["timed_region"]["repeats"] == 1 and d["ms_per_step"] > 0
    assert "roofline" not in d and "sampling_only" not in d            # a run without --full: the headline and nothing beside it
    assert abs(d["ms_per_step"] / 1e3 * 3 - d["timed_region"]["median_s"]) < 1e-9
    assert sum(os.path.getsize(f) for f in glob.glob(str(tmp_path / "a" / "*.npy"))) <= legs.DUMP_BYTES
    assert all(a.dtype == (np.float32 if k == "float_features" else np.float64) for k, a in out.items())
    assert out["batch_ids"].size == G and np.all(np.diff(out["batch_ids"]) == 1)
    assert np.all(out["node_counter"][:, 9] == B) and np.all(out["edge_counter"][:, 11] > 0)
    ids = out["sampled_ids"].astype(np.int64)
    assert ids.size > 0 and np.array_equal(out["float_features"].view(np.uint32),
                                           synth.feature_rows_numpy(ids, 128, 7).view(np.uint32))
    indptr, col = synth.rmat_csr_numpy(SCALE, EF, 20231)
    dst, src = out["agg_dst_ids"].astype(np.int64), out["agg_src_ids"].astype(np.int64)
    n = indptr.size - 1
    graph_keys = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr)) * n + col
    assert src.size > 0 and np.isin(dst * n + src, graph_keys).all()
    _, again = run_dump(tmp_path / "b")                          # same command, same inputs: the same outputs
    assert out.keys() == again.keys() and all(np.array_equal(out[k], again[k]) for k in out)
