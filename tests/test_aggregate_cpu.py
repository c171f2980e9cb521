"""The fused neighbour aggregation without a GPU: the entry points in the header, the ctypes table and the library, the scratch rule,
every refusal of legion_aggregate_rows (aggregate_rule.h decides them before any HIP call) and the Python methods' ValueErrors."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from legion_amd import engine, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["legion_aggregate_scratch_bytes", "legion_aggregate_rows"]
SUM, MEAN, MAX = 0, 1, 2
PTR = ctypes.c_void_p(4096)                                            # not null; n == 0 enqueues nothing, so it is never followed


def test_symbols_in_header_ctypes_table_and_library():
    text = open(os.path.join(ROOT, "include", "legion_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "legion_amd", "liblegion_hip.so")], check=True,
                         capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NAMES:
        assert re.search(r"\bint(32|64)_t\s+" + name + r"\s*\(", text) and name in exported, name
    for k, name in enumerate(("SUM", "MEAN", "MAX")):
        assert re.search(rf"#define\s+LEGION_REDUCE_{name}\s+{k}\b", text)
    c_p, c_i32, c_i64 = lib.c_p, lib.c_i32, lib.c_i64
    assert lib.SIGNATURES["legion_aggregate_scratch_bytes"] == (c_i64, [c_i32, c_i64, c_i32])
    assert lib.SIGNATURES["legion_aggregate_rows"] == (c_i32, [c_p, c_i32, c_i32, c_p, c_p, c_p, c_i32, c_i32, c_p, c_i32, c_p, c_i64, c_p,
                                                              c_i32, c_p, c_p, c_i64])
    assert engine.FeatureStorage.REDUCES == {"sum": SUM, "mean": MEAN, "max": MAX}


def test_scratch_is_monotone_in_m_and_zero_safe():
    size = lib.load().legion_aggregate_scratch_bytes
    assert size(0, 0, 4) == 16 and size(0, 0, 1) >= 0 and size(5, 0, 128) == 64
    for n, D in ((0, 1), (7, 128), (2 ** 20 + 1, 3)):
        sizes = [size(n, M, D) for M in (0, 1, 255, 256, 257, 4096, 2 ** 20, 2 ** 28)]
        assert sizes == sorted(sizes) and sizes[0] >= 8 * (n + 1) and sizes[-1] > sizes[0], (n, D, sizes)
    assert size(7, 2 ** 28, 128) - size(7, 0, 128) <= (2 ** 28 // 128) * (4 * 128 + 4), "at most M / 128 partial rows and their counts"
    for bad in ((-1, 0, 4), (0, -1, 4), (0, 0, 0), (2 ** 28 + 1, 0, 4)):
        assert size(*bad) == -1, bad


REFUSALS = {
    "reduce": dict(reduce=3), "reduce-negative": dict(reduce=-1), "dtype": dict(dtype=2), "out_dtype": dict(out_dtype=2),
    "weights-mean": dict(weights=PTR, reduce=MEAN), "weights-max": dict(weights=PTR, reduce=MAX),
    "cache-without-map": dict(cache=PTR), "map-without-cache": dict(node_map=PTR), "bf16-pitch": dict(dtype=1, D=2 ** 31 - 5),
    "n": dict(n=-1), "n-too-many": dict(n=2 ** 28 + 1, nbytes=2 ** 40), "M": dict(M=-1), "D": dict(D=0), "D-negative": dict(D=-4),
    "null-table": dict(table=None), "null-offsets": dict(offsets=None), "null-ids": dict(ids=None), "null-out": dict(out=None),
    "null-scratch": dict(scratch=None), "scratch-short": dict(nbytes=15), "scratch-negative": dict(nbytes=-1),
    "scratch-short-for-M": dict(M=2 ** 20, nbytes=16),
}


def call(L, **change):
    a = dict(dtype=0, out_dtype=0, table=PTR, cache=None, node_map=None, D=4, N=10, offsets=PTR, n=0, ids=PTR, M=0, weights=None,
             reduce=SUM, out=PTR, scratch=PTR, nbytes=16)
    a.update(change)
    return L.legion_aggregate_rows(None, a["dtype"], a["out_dtype"], a["table"], a["cache"], a["node_map"], a["D"], a["N"], a["offsets"],
                                   a["n"], a["ids"], a["M"], a["weights"], a["reduce"], a["out"], a["scratch"], a["nbytes"])


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_every_refusal_returns_minus_one_without_a_device(name):
    L = lib.load()
    assert call(L) == 0, "no segments: accepted, nothing enqueued"
    assert call(L, weights=PTR) == 0 and call(L, cache=PTR, node_map=PTR, dtype=1, out_dtype=1, reduce=MAX) == 0
    assert call(L, **REFUSALS[name]) == -1, name


def test_argument_errors_are_value_errors_before_any_device():
    f = engine.FeatureStorage.__new__(engine.FeatureStorage)          # (no handle: the checks come before the library call)
    f._lib, f.float_feature_len, f.total_num_nodes, f.feature_dtype = lib.load(), 4, 10, "float32"
    off, ids = np.array([0, 2], np.int64), np.array([1, 2], np.int32)
    for kw, match in ((dict(reduce="min"), "reduce"), (dict(out_dtype="fp8"), "out_dtype"), (dict(cache=object()), "UnifiedCache"),
                      (dict(reduce="mean", weights=np.ones(2, np.float32)), "weights"), (dict(dev_id="0"), "dev_id"),
                      (dict(weights=np.ones(3, np.float32)), "3 weights for 2 ids"), (dict(weights=torch.ones(2, dtype=torch.float64)), "float32")):
        with pytest.raises(ValueError, match=match):
            f.aggregate(off, ids, **kw)
    with pytest.raises(ValueError, match="int64"):
        f.aggregate(torch.tensor([0, 2], dtype=torch.int32), ids)
    with pytest.raises(ValueError, match="one-dimensional"):
        f.aggregate(off, ids.reshape(1, 2))
    g = engine.GraphStorage.__new__(engine.GraphStorage)
    g.node_num = 10
    with pytest.raises(ValueError, match="FeatureStorage"):
        g.full_neighbor_aggregate(object(), ids)
