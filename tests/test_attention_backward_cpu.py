"""The backward pass of the fused attention aggregation without a GPU: the entry points in the ctypes table, the scratch rule, every
refusal of legion_attention_rows_backward (attention_backward_rule.h decides them before any HIP call), the Python method's
ValueErrors, and the autograd reference against the forward's."""
import ctypes

import numpy as np
import pytest

from legion_amd import engine, lib
from tests import attention_backward_ref, attention_ref

PTR = ctypes.c_void_p(4096)                                            # not null; n == 0 enqueues nothing, so it is never followed


def test_signatures():
    c_p, c_i32, c_i64, c_f32 = lib.c_p, lib.c_i32, lib.c_i64, lib.c_f32
    assert lib.SIGNATURES["legion_attention_backward_scratch_bytes"] == (c_i64, [c_i32, c_i64, c_i32, c_i32])
    assert lib.SIGNATURES["legion_attention_rows_backward"] == (c_i32, [c_p, c_i32, c_p, c_p, c_p, c_i32, c_i32, c_p, c_i32, c_p, c_i64, c_p, c_i32,
                                                                       c_f32] + [c_p] * 8 + [c_i64])


def test_scratch_follows_the_rule():
    """The aggregation's first words, then 2 (M / 256) records of heads x D float32."""
    L = lib.load()
    size, first = L.legion_attention_backward_scratch_bytes, lambda n: L.legion_aggregate_scratch_bytes(n, 0, 1)
    for n, M, D, H in ((0, 0, 4, 1), (5, 0, 128, 8), (7, 255, 128, 4), (7, 256, 128, 4), (7, 1000, 3, 3), (2 ** 20 + 1, 2 ** 28, 100, 8)):
        assert size(n, M, D, H) == first(n) + 2 * (M // 256) * 4 * H * D, (n, M, D, H)
    for bad in ((-1, 0, 4, 1), (0, -1, 4, 1), (0, 0, 0, 1), (2 ** 28 + 1, 0, 4, 1), (0, 0, 4, 0), (0, 0, 4, 9)):
        assert size(*bad) == -1, bad


REFUSALS = {
    "dtype": dict(dtype=2), "heads-zero": dict(heads=0), "heads-nine": dict(heads=9), "cache-without-map": dict(cache=PTR),
    "map-without-cache": dict(node_map=PTR), "no-logit": dict(queries=None, gq=None), "n": dict(n=-1), "n-too-many": dict(n=2 ** 28 + 1, nbytes=2 ** 40),
    "M": dict(M=-1), "D": dict(D=0), "bf16-pitch": dict(dtype=1, D=2 ** 31 - 5), "width-forward": dict(D=1028),
    "width-f32-heads": dict(D=260, heads=8), "width-f32-wide": dict(D=1024, heads=3), "width-bf16-heads": dict(dtype=1, D=128, heads=8),
    "null-table": dict(table=None), "null-offsets": dict(offsets=None), "null-ids": dict(ids=None), "null-scratch": dict(scratch=None),
    "null-grad-out": dict(grad_out=None), "null-out": dict(out=None), "null-lse": dict(lse=None), "no-output": dict(gq=None, gb=None, gr=None),
    "grad-queries-without-queries": dict(queries=None, bias=PTR), "scratch-short": dict(nbytes=15), "scratch-short-for-M": dict(M=2 ** 20, nbytes=16),
}


def call(L, **change):
    a = dict(dtype=0, table=PTR, cache=None, node_map=None, D=4, N=10, offsets=PTR, n=0, ids=PTR, M=0, queries=PTR, heads=1, bias=None,
             grad_out=PTR, out=PTR, lse=PTR, gq=PTR, gb=PTR, gr=PTR, scratch=PTR, nbytes=16)
    a.update(change)
    return L.legion_attention_rows_backward(None, a["dtype"], a["table"], a["cache"], a["node_map"], a["D"], a["N"], a["offsets"], a["n"],
                                            a["ids"], a["M"], a["queries"], a["heads"], 1.0, a["bias"], a["grad_out"], a["out"], a["lse"],
                                            a["gq"], a["gb"], a["gr"], a["scratch"], a["nbytes"])


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_every_refusal_returns_minus_one_without_a_device(name):
    L = lib.load()
    assert call(L) == 0, "no segments: accepted, nothing enqueued"
    assert call(L, queries=None, bias=PTR, gq=None, gb=None, heads=8, D=256) == 0 and call(L, D=1024, heads=2, gq=None, gr=None) == 0
    assert call(L, cache=PTR, node_map=PTR, dtype=1, D=2048) == 0 and call(L, D=128, heads=8) == 0 and call(L, D=256, heads=4) == 0
    assert call(L, **REFUSALS[name]) == -1, name


def test_argument_errors_are_value_errors_before_any_device():
    f = engine.FeatureStorage.__new__(engine.FeatureStorage)          # (no handle: the checks come before the library call)
    f._lib, f.float_feature_len, f.total_num_nodes, f.feature_dtype = lib.load(), 4, 10, "float32"
    off, ids, q = np.array([0, 2], np.int64), np.array([1, 2], np.int32), np.zeros((1, 2, 4), np.float32)
    g, lse = np.zeros((1, 2, 4), np.float32), np.zeros((1, 2), np.float32)
    for args, kw, match in (((g, g, lse), dict(), "queries, bias or both"), ((g, g, lse), dict(queries=q[:, :, :3]), "queries must be"),
                            ((g, g, lse), dict(queries=q, cache=object()), "UnifiedCache"), ((g, g, lse), dict(queries=q, grads=()), "grads must be"),
                            ((g, g, lse), dict(queries=q, grads="rows"), "grads must be"), ((g, g, lse), dict(queries=q, grads=("rows", "out")), "grads must be"),
                            ((g, g, lse), dict(queries=q, grads=("bias", "bias")), "grads must be"),
                            ((g, g, lse), dict(bias=np.zeros((2, 2), np.float32)), "has no queries"),
                            ((g[:, :1], g, lse), dict(queries=q), "grad_out must be"), ((g, g.astype(np.float64), lse), dict(queries=q), "out must be"),
                            ((g[0], g[0], lse), dict(queries=q), "grad_out must be"), ((g, g, lse[:, :1]), dict(queries=q), "lse must be")):
        with pytest.raises(ValueError, match=match):
            f.attention_backward(off, ids, *args, **kw)
    f.float_feature_len = 260                                          # (inside the forward's plan at 8 heads, outside the backward's)
    wide = np.zeros((1, 8, 260), np.float32)
    with pytest.raises(ValueError, match="backward's register plan"):
        f.attention_backward(off, ids, wide, wide, np.zeros((1, 8), np.float32), queries=wide)


def test_the_reference_agrees_with_the_forward_reference():
    rng = np.random.default_rng(5)
    N, D, H = 50, 6, 3
    offsets = np.array([0, 0, 4, 9, 12], np.int64)
    ids = rng.integers(0, N, 12).astype(np.int32)
    ids[[2, 9, 10, 11]] = [-1, N, -3, N + 4]                           # a dead entry, and the last segment dead ids only
    X, q = rng.standard_normal((N, D)).astype(np.float32), rng.standard_normal((4, H, D)).astype(np.float32)
    b, dO = rng.standard_normal((12, H)).astype(np.float32), rng.standard_normal((4, H, D))
    node_map = np.where(np.arange(N) % 3 == 0, np.arange(N) // 3, -2).astype(np.int32)
    cache = X[::3] + np.float32(1000)
    for kw in (dict(queries=q, bias=b, scale=0.4), dict(bias=b), dict(queries=q, scale=0.4, node_map=node_map, cache=cache)):
        out, gq, gb, gx = attention_backward_ref.attention_backward(X, offsets, ids, dO, **kw)
        assert np.allclose(out, attention_ref.attention(X, offsets, ids, **kw)[0], rtol=1e-12, atol=1e-12)
        assert (gq is None) == ("queries" not in kw) and (gb is None) == ("bias" not in kw)
        assert np.all(gx[[2, 9, 10, 11]] == 0) and np.any(gx[3] != 0) and (gq is None or np.all(gq[[0, 3]] == 0))
