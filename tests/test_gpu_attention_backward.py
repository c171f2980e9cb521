"""legion_attention_rows_backward and its Python surface on the GPU against tests/attention_backward_ref.py (torch.autograd in float64).
Random floats are held to a bound derived from the rule; where the inputs make every float32 step exact (integer values, one dominant
entry a head) the gradients are compared bit for bit.  The lists, the stored tables and the cache are test_gpu_aggregate.py's."""
import ctypes

import numpy as np
import pytest
import torch

from tests import attention_backward_ref as ref, attention_ref
from tests.test_gpu_aggregate import DEV, K, N, WAVES, groups, same, segments, stored
from tests.test_gpu_attention import SHAPES, cache_of
from tests.test_gpu_attention import run as run_forward

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

U24, TINY = 2.0 ** -24, 2.0 ** -126


def run(L, dtype, table, D, offsets, ids, grad_out, out, lse, queries=None, bias=None, scale=1.0, cache=None, node_map=None):
    """The C ABI over outputs filled with a sentinel, one row more than written, and a scratch filled with NaN bits; returns
    (grad_queries [n, H, D] or None, grad_bias [M, H], grad_rows [M, D]) as float32 numpy, or None for a refused call."""
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(DEV) if x is not None else None
    n, M, H = offsets.size - 1, ids.size, grad_out.shape[1]
    fill = lambda *shape: torch.full(shape, -12288.0, dtype=torch.float32, device=DEV)
    gq, gb, gr = fill(n + 1, H, D) if queries is not None else None, fill(M + 1, H), fill(M + 1, D)
    nbytes = int(L.legion_attention_backward_scratch_bytes(n, M, D, H))
    scratch = torch.full((nbytes // 8 + 2,), -1, dtype=torch.int64, device=DEV)
    keep = [torch.from_numpy(offsets).to(DEV), torch.from_numpy(ids).to(DEV)] + [dev(x) for x in (queries, bias, grad_out, out, lse)]
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.legion_attention_rows_backward(s, {"float32": 0, "bfloat16": 1}[dtype], P(table), P(cache), P(node_map), D, N, P(keep[0]), n, P(keep[1]),
                                          M, P(keep[2]), H, scale, P(keep[3]), P(keep[4]), P(keep[5]), P(keep[6]), P(gq), P(gb), P(gr), P(scratch), nbytes)
    if rc != 0:
        return None
    torch.cuda.synchronize()
    got = [t.cpu().numpy() if t is not None else None for t in (gq, gb, gr)]
    assert all(g is None or np.all(g[-1] == -12288.0) for g in got), "written past the last row"
    return got[0][:n] if gq is not None else None, got[1][:M], got[2][:M]


def bound_check(L, dtype, D, H, lengths, rng, with_queries, cached, skipped=None):
    """u = 2^-24; per segment d, head h, live entry e, with the float64 values of the rule.  (1) A dot of D terms, fmas in a lane and a
    tree over the lanes, errs by at most (D + 2) u times the sum of its terms' magnitudes: t by et = (D + 2) u sum |dO x|, delta (whose
    out is the reference's rounded once) by ed = (D + 2) u sum |dO out|, the logit s by es = (D + 2) u (scale sum |q x| + |bias|), as the
    forward's test derives.  (2) p^ = expf(fl(s^ - lse^)), lse the reference's rounded once, expf within 1 ulp (2^-23, HIP's documented
    bound): relatively eta = es + u |lse| + u |s - lse| + 2^-23.  (3) dS^ = fl(p^ fl(t^ - delta^)): the difference cancels, so its error
    et + ed + u |t - delta| is absolute in |dO| |x|, not relative to dS: eS = p ((eta + 2 u) |t - delta| + et + ed), the bound of
    grad_bias.  (4) grad_rows[e, c] is 2 H fmas and H products: sum_h (eta p |dO_c| + |scale| eS |q_c|) + (2 H + 2) u sum_h (p |dO_c| +
    |scale dS q_c|).  (5) grad_queries[d, h, c] is len fmas in some order and a product: |scale| (sum_e eS |x_c| + (len + 2) u sum_e |dS x_c|).
    (6) A float32 result below the normal range, 2^-126, is rounded to the subnormal grid or flushed: its error is at most 2^-126 in
    place of u times itself.  The cache's rows lie 1000 off the table's, so weights do underflow: p errs by eta p + 2^-126, and every
    later operation adds 2^-126 once (2 for dS, 2 H + 2 for a grad_rows element, len + 2 for a grad_queries element).
    Prints the worst fraction of its bound per output and returns what the kernel gave."""
    offsets, ids = segments(lengths, rng, skipped=skipped)
    n, M, scale = len(lengths), ids.size, float(np.float32(D ** -0.5))
    table, X = stored(rng.standard_normal((N, D)).astype(np.float32), dtype)
    m, node_map, cache, C = cache_of(X, dtype) if cached else (None,) * 4
    q = rng.standard_normal((n, H, D)).astype(np.float32) if with_queries else None
    b, dO = rng.standard_normal((M, H)).astype(np.float32), rng.standard_normal((n, H, D)).astype(np.float32)
    out, want_q, want_b, want_r = ref.attention_backward(X, offsets, ids, dO, q, b, scale, m, C)
    lse = attention_ref.attention(X, offsets, ids, q, b, scale, m, C)[2]
    got = run(L, dtype, table, D, offsets, ids, dO, out, lse, q, b, scale, cache, node_map)
    if H == 8 and (dtype == "bfloat16" or D == 260):                   # attention_backward_rule.h: heads' x U x W = 64 > 32 floats a lane
        assert got is None, "a width outside the backward's register plan is refused"
        return None
    x, live = ref.gathered(X, ids, m, C)
    seg, q0, ax = np.repeat(np.arange(n), lengths), np.zeros((n, H, D)) if q is None else q.astype(np.float64), np.abs(x)
    s = scale * np.einsum("mhd,md->mh", q0[seg], x) + b
    a = np.where(live[:, None], s - np.where(np.isinf(lse), 0, lse)[seg], -np.inf)
    p, t, delta = np.exp(a), np.einsum("mhd,md->mh", dO[seg], x), np.einsum("nhd,nhd->nh", dO, out)[seg]
    dS = p * (t - delta)
    et, ed = (D + 2) * U24 * np.einsum("mhd,md->mh", np.abs(dO)[seg], ax), ((D + 2) * U24 * np.einsum("nhd,nhd->nh", np.abs(dO), np.abs(out)))[seg]
    es = (D + 2) * U24 * (scale * np.einsum("mhd,md->mh", np.abs(q0)[seg], ax) + np.abs(b))
    eta = es + U24 * np.abs(np.where(np.isinf(lse), 0, lse))[seg] + U24 * np.abs(np.where(live[:, None], a, 0)) + 2.0 ** -23
    ep = np.where(live[:, None], eta * p + TINY, 0)
    eS = ep * (np.abs(t - delta) + et + ed) + p * (2 * U24 * np.abs(t - delta) + et + ed) + np.where(live[:, None], 2 * TINY, 0)
    eR = (np.einsum("mh,mhd->md", ep, np.abs(dO)[seg]) + scale * np.einsum("mh,mhd->md", eS, np.abs(q0)[seg]) + np.where(live[:, None], (2 * H + 2) * TINY, 0)
          + (2 * H + 2) * U24 * (np.einsum("mh,mhd->md", p, np.abs(dO)[seg]) + scale * np.einsum("mh,mhd->md", np.abs(dS), np.abs(q0)[seg])))
    eQ, mass = np.zeros((n, H, D)), np.zeros((n, H, D))
    np.add.at(eQ, seg, eS[:, :, None] * ax[:, None, :])
    np.add.at(mass, seg, np.abs(dS)[:, :, None] * ax[:, None, :])
    eQ = scale * (eQ + (np.array(lengths)[:, None, None] + 2) * U24 * mass) + (np.array(lengths)[:, None, None] + 2) * TINY * (eQ > 0)
    tiny = np.finfo(np.float64).tiny                                   # (a bound of 0 goes with an exact 0: a dead entry, an empty segment)
    worst = {name: float(np.max(np.abs(g - w) / (e + tiny))) for name, g, w, e in (("queries", got[0], want_q, eQ), ("bias", got[1], want_b, eS),
                                                                                    ("rows", got[2], want_r, eR)) if g is not None}
    print(f"{dtype} D {D} H {H}: worst fraction of the bound: {worst}")
    assert max(worst.values()) <= 1, worst
    assert (~live).any() and np.all(got[1][~live] == 0) and np.all(got[2][~live] == 0), "dead entries give exact zeros"
    again = run(L, dtype, table, D, offsets, ids, dO, out, lse, q, b, scale, cache, node_map)
    for g, h in zip(got, again):
        assert g is None or np.array_equal(g.view(np.uint32), h.view(np.uint32)), "the same call twice"
    return got


@pytest.mark.parametrize("cached", [False, True], ids=["no-cache", "cache"])
@pytest.mark.parametrize("with_queries", [True, False], ids=["queries", "bias-only"])
@pytest.mark.parametrize("H", [1, 3, 8])
@pytest.mark.parametrize("dtype,D", SHAPES)
def test_random_floats_within_the_derived_bound(hip, dtype, D, H, with_queries, cached):
    G = groups(dtype, D)
    lengths = [0, 1, max(G - 1, 0), G + 1, K - 1, K, K + 1, 3 * K + 5, 9]
    got = bound_check(hip, dtype, D, H, lengths, np.random.default_rng(D + H), with_queries, cached, skipped=8)
    assert got is None or not with_queries or np.all(got[0][[0, 8]] == 0), "no live entry: a zero grad_queries row"


def test_more_chunks_than_the_grid_has_waves(hip):
    rng = np.random.default_rng(7)
    assert bound_check(hip, "float32", 4, 1, rng.integers(1, 3, WAVES + 37).tolist(), rng, True, False) is not None


@pytest.mark.parametrize("with_queries", [True, False], ids=["queries", "bias-only"])
@pytest.mark.parametrize("dtype,D,H", [("float32", 20, 1), ("float32", 20, 3), ("float32", 20, 8), ("bfloat16", 128, 3)])
def test_a_dominant_integer_logit_gives_exact_gradients(hip, dtype, D, H, with_queries):
    """Integer rows, queries, biases and grad_out; one entry's bias lifts it 200 above every other logit of its segment and head (the
    forward's placements: first, last, a group other than 0, the last of four chunks).  The forward gives lse = that logit and out =
    that row, so p is exactly 1 for it and expf(<= -200) = 0 elsewhere, and delta = t of the dominant entry: grad_bias and grad_queries
    are zeros and grad_rows[e] is the sum of dO[d, h] over the heads whose dominant entry e is, bit for bit."""
    rng = np.random.default_rng(D + H)
    offsets, ids = segments([9, 3 * K + 5], rng)
    table, X = stored(rng.integers(-8, 9, (N, D)).astype(np.float32), dtype)
    queries = rng.integers(-2, 3, (2, H, D)).astype(np.float32) if with_queries else None
    bias, dO = rng.integers(-5, 6, (ids.size, H)).astype(np.float32), rng.integers(-4, 5, (2, H, D)).astype(np.float32)
    spots = {0: [0, 8, 1, 5], 1: [0, 3 * K + 4, 1, 2 * K + 44, 3 * K, K - 1, K, 77]}
    want = np.zeros((ids.size, D), np.float32)
    for d, where in spots.items():
        for h in range(H):
            e = offsets[d] + where[h % len(where)]
            bias[e, h] = 2 * 16 * D + 10 + 200                         # |dot| <= 16 D, |bias| <= 5
            ids[e] = (7 * e + h) % N                                   # live, whatever segments() drew
            want[e] += dO[d, h]
    out, _, lse = run_forward(hip, dtype, "float32", table, D, offsets, ids, queries, bias, 1.0)
    gq, gb, gr = run(hip, dtype, table, D, offsets, ids, dO, out, lse, queries, bias, 1.0)
    assert np.all(gb == 0) and (gq is None or np.all(gq == 0))
    same(gr, want, "grad_rows")


def test_the_python_surface(hip):
    from legion_amd import engine
    rng = np.random.default_rng(3)
    V, D, H = 300, 20, 2
    deg = rng.integers(0, 12, V)
    deg[5] = 700
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = rng.integers(0, V, int(indptr[-1])).astype(np.int32)
    X = rng.integers(-8, 9, (V, D)).astype(np.float32)
    graph = engine.GraphStorage(1, torch.from_numpy(indptr).to(DEV), torch.from_numpy(col).to(DEV))
    feature = engine.FeatureStorage(1, torch.from_numpy(X).to(DEV))
    try:
        rows = np.concatenate([rng.permutation(V)[:90], [5, 5, -1, V]]).astype(np.int32)
        q = (rng.integers(-4, 5, (rows.size, H, D)) / 8).astype(np.float32)
        dO = torch.from_numpy(rng.standard_normal((rows.size, H, D)).astype(np.float32)).to(DEV)
        out, lse = graph.full_neighbor_attention(feature, rows, q, return_lse=True)
        offsets, _, src = graph.in_edges(rows)
        gq, gb, gr = feature.attention_backward(offsets, src, dO, out, lse, queries=q)
        off, ids = offsets.cpu().numpy(), src.cpu().numpy()
        _, want_q, _, want_r = ref.attention_backward(X, off, ids, dO.cpu().numpy(), q, None, np.float32(D ** -0.5))
        tol = 1e-4 * np.abs(X).max() * float(dO.abs().max())           # (the bound itself: test_random_floats; here the plumbing)
        near = lambda g, w: np.allclose(g.cpu().numpy(), w, rtol=0, atol=tol)
        assert gq.shape == q.shape and gb.shape == (ids.size, H) and gr.shape == (ids.size, D) and near(gq, want_q) and near(gr, want_r)
        # [n, D] queries: [n, D] grad_out and out, [n, D] grad_queries; the subsets of grads; bias alone; the empty call
        flat = feature.attention_backward(offsets, src, dO[:, 1], *feature.attention(offsets, src, queries=q[:, 1], return_lse=True), queries=q[:, 1])
        assert flat[0].shape == (rows.size, D) and flat[1].shape == (ids.size, 1) and near(flat[0], want_q[:, 1])
        only = feature.attention_backward(offsets, src, dO, out, lse, queries=q, grads=("rows", "queries"))
        assert len(only) == 2 and torch.equal(only[0], gq) and torch.equal(only[1], gr)
        b = torch.from_numpy(rng.integers(-3, 4, (ids.size, H)).astype(np.float32)).to(DEV)
        b_out, b_lse = feature.attention(offsets, src, bias=b, return_lse=True)
        (b_gb,) = feature.attention_backward(offsets, src, dO, b_out, b_lse, bias=b, grads=("bias",))
        assert near(b_gb, ref.attention_backward(X, off, ids, dO.cpu().numpy(), None, b.cpu().numpy())[2])
        empty = feature.attention_backward(np.zeros(4, np.int64), np.zeros(0, np.int32), dO[:3], out[:3], lse[:3], queries=q[:3])
        assert [tuple(t.shape) for t in empty] == [(3, H, D), (0, H), (0, D)] and not empty[0].any()
        # one SGD step on the entries' rows is X - lr * index_add(grad_rows)
        feature.update_rows(src, gr, optimizer="sgd", lr=0.5, combine="sum")
        torch.cuda.synchronize()
        step = np.zeros((V, D))
        np.add.at(step, ids, want_r)
        assert np.allclose(feature.features.cpu().numpy(), X - 0.5 * step, rtol=0, atol=tol)
    finally:
        torch.cuda.synchronize()
        graph.close()
        feature.close()
