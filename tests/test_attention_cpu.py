"""The fused attention aggregation without a GPU: the entry points in the ctypes table and the library, the scratch rule, every
refusal of legion_attention_rows (attention_rule.h decides them before any HIP call) and the Python methods' ValueErrors."""
import ctypes

import numpy as np
import pytest
import torch

from legion_amd import engine, lib

PTR = ctypes.c_void_p(4096)                                            # not null; n == 0 enqueues nothing, so it is never followed


def test_signatures():
    c_p, c_i32, c_i64, c_f32 = lib.c_p, lib.c_i32, lib.c_i64, lib.c_f32
    assert lib.SIGNATURES["legion_attention_scratch_bytes"] == (c_i64, [c_i32, c_i64, c_i32, c_i32])
    assert lib.SIGNATURES["legion_attention_rows"] == (c_i32, [c_p, c_i32, c_i32, c_p, c_p, c_p, c_i32, c_i32, c_p, c_i32, c_p, c_i64, c_p,
                                                              c_i32, c_f32, c_p, c_p, c_p, c_p, c_p, c_i64])
    assert engine.FeatureStorage.ATTENTION_MAX_HEADS == 8


def test_scratch_follows_the_rule():
    """The aggregation's first words, then 2 (M / 256) records of heads x (2 + D) float32."""
    L = lib.load()
    size, first = L.legion_attention_scratch_bytes, lambda n: L.legion_aggregate_scratch_bytes(n, 0, 1)
    for n, M, D, H in ((0, 0, 4, 1), (5, 0, 128, 8), (7, 255, 128, 4), (7, 256, 128, 4), (7, 1000, 3, 3), (2 ** 20 + 1, 2 ** 28, 100, 8)):
        assert size(n, M, D, H) == first(n) + 2 * (M // 256) * 4 * H * (2 + D), (n, M, D, H)
    for bad in ((-1, 0, 4, 1), (0, -1, 4, 1), (0, 0, 0, 1), (2 ** 28 + 1, 0, 4, 1), (0, 0, 4, 0), (0, 0, 4, 9)):
        assert size(*bad) == -1, bad


REFUSALS = {
    "dtype": dict(dtype=2), "out_dtype": dict(out_dtype=-1), "heads-zero": dict(heads=0), "heads-nine": dict(heads=9),
    "cache-without-map": dict(cache=PTR), "map-without-cache": dict(node_map=PTR), "no-logit": dict(queries=None),
    "n": dict(n=-1), "n-too-many": dict(n=2 ** 28 + 1, nbytes=2 ** 40), "M": dict(M=-1), "D": dict(D=0), "bf16-pitch": dict(dtype=1, D=2 ** 31 - 5),
    "width-f32": dict(D=1028), "width-f32-heads": dict(D=516, heads=8), "width-f32-odd": dict(D=257), "width-bf16": dict(dtype=1, D=520, heads=8),
    "null-table": dict(table=None), "null-offsets": dict(offsets=None), "null-ids": dict(ids=None), "null-out": dict(out=None),
    "null-scratch": dict(scratch=None), "scratch-short": dict(nbytes=15), "scratch-short-for-M": dict(M=2 ** 20, nbytes=16),
}


def call(L, **change):
    a = dict(dtype=0, out_dtype=0, table=PTR, cache=None, node_map=None, D=4, N=10, offsets=PTR, n=0, ids=PTR, M=0, queries=PTR, heads=1,
             bias=None, out=PTR, scores=None, lse=None, scratch=PTR, nbytes=16)
    a.update(change)
    return L.legion_attention_rows(None, a["dtype"], a["out_dtype"], a["table"], a["cache"], a["node_map"], a["D"], a["N"], a["offsets"],
                                   a["n"], a["ids"], a["M"], a["queries"], a["heads"], 1.0, a["bias"], a["out"], a["scores"], a["lse"],
                                   a["scratch"], a["nbytes"])


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_every_refusal_returns_minus_one_without_a_device(name):
    L = lib.load()
    assert call(L) == 0, "no segments: accepted, nothing enqueued"
    assert call(L, queries=None, bias=PTR, heads=8, D=512) == 0 and call(L, cache=PTR, node_map=PTR, dtype=1, out_dtype=1, D=2048, heads=2) == 0
    assert call(L, **REFUSALS[name]) == -1, name


def test_argument_errors_are_value_errors_before_any_device():
    f = engine.FeatureStorage.__new__(engine.FeatureStorage)          # (no handle: the checks come before the library call)
    f._lib, f.float_feature_len, f.total_num_nodes, f.feature_dtype = lib.load(), 4, 10, "float32"
    off, ids, q = np.array([0, 2], np.int64), np.array([1, 2], np.int32), np.zeros((1, 2, 4), np.float32)
    for kw, match in ((dict(), "queries, bias or both"), (dict(queries=q, out_dtype="fp8"), "out_dtype"), (dict(queries=q, cache=object()), "UnifiedCache"),
                      (dict(queries=q[:, :, :3]), "queries must be"), (dict(queries=q.astype(np.float64)), "queries must be"),
                      (dict(queries=np.zeros((2, 4), np.float32)), "queries must be"), (dict(queries=q, bias=np.zeros((2, 3), np.float32)), "bias must be"),
                      (dict(bias=np.zeros((3, 1), np.float32)), "bias must be"), (dict(bias=np.zeros((2, 9), np.float32)), "9 heads"),
                      (dict(queries=q, scale="1"), "scale"), (dict(queries=q, scale=float("nan")), "scale"), (dict(queries=q, dev_id="0"), "dev_id"),
                      (dict(queries=q, return_scores=1), "return_scores"), (dict(queries=q, return_lse=None), "return_lse")):
        with pytest.raises(ValueError, match=match):
            f.attention(off, ids, **kw)
    with pytest.raises(ValueError, match="int64"):
        f.attention(torch.tensor([0, 2], dtype=torch.int32), ids, queries=q)
    f.float_feature_len = 1028
    with pytest.raises(ValueError, match="register plan"):
        f.attention(off, ids, queries=np.zeros((1, 1028), np.float32))
    g = engine.GraphStorage.__new__(engine.GraphStorage)
    g.node_num = 10
    with pytest.raises(ValueError, match="FeatureStorage"):
        g.full_neighbor_attention(object(), ids, q)
