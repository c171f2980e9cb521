"""legion_attention_rows and its Python surface on the GPU against tests/attention_ref.py.  Where the inputs make every float32 step
exact (zero queries: the mean; integer logits with one dominant entry: a row), the result is compared bit for bit; random floats are
held to a bound derived from the rule.  The lists, the stored tables and the cache (rows off by 1000) are test_gpu_aggregate.py's."""
import ctypes

import numpy as np
import pytest
import torch

from tests import aggregate_ref, attention_ref as ref
from tests.test_gpu_aggregate import DEV, K, N, WAVES, groups, same, segments, stored
from tests.test_gpu_aggregate import run as run_aggregate

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

U24 = 2.0 ** -24
# C = 1, a middle C, one float32 a lane over two units, C = 64, two units of 16 bytes a lane; bf16 narrow, padded and 128 wide
SHAPES = [("float32", D) for D in (1, 20, 70, 256, 260)] + [("bfloat16", D) for D in (8, 100, 128)]


def run(L, dtype, out_dtype, table, D, offsets, ids, queries=None, bias=None, scale=1.0, cache=None, node_map=None):
    """The C ABI over outputs filled with a sentinel and a scratch filled with NaN bits; returns (out [n, H, D], scores [M, H], lse
    [n, H]) as float32 numpy."""
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV) if x is not None else None
    n, M, H = offsets.size - 1, ids.size, (queries if queries is not None else bias).shape[1]
    d_off, d_ids, d_q, d_b = dev(offsets), dev(ids), dev(queries), dev(bias)
    out = torch.full((n + 1, H, D), -12288.0, dtype=torch.float32 if out_dtype == "float32" else torch.bfloat16, device=DEV)
    scores = torch.full((M + 1, H), -12288.0, dtype=torch.float32, device=DEV)
    lse = torch.full((n + 1, H), -12288.0, dtype=torch.float32, device=DEV)
    nbytes = int(L.legion_attention_scratch_bytes(n, M, D, H))
    scratch = torch.full((nbytes // 8 + 2,), -1, dtype=torch.int64, device=DEV)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    code = {"float32": 0, "bfloat16": 1}
    assert L.legion_attention_rows(s, code[dtype], code[out_dtype], P(table), P(cache), P(node_map), D, N, P(d_off), n, P(d_ids), M, P(d_q),
                                   H, scale, P(d_b), P(out), P(scores), P(lse), P(scratch), nbytes) == 0
    torch.cuda.synchronize()
    got = [t.float().cpu().numpy() for t in (out, scores, lse)]
    assert all(np.all(g[-1] == -12288.0) for g in got), "written past the last row"
    return got[0][:n], got[1][:M], got[2][:n]


def cache_of(X, dtype):
    """A third of the ids hit; their rows are the table's + 1000: (node_map on the host, on the device, the cache table, its values)."""
    m = np.where(np.arange(N) % 3 == 0, np.arange(N) // 3, -2).astype(np.int32)
    cache, C = stored(X[::3] + np.float32(1000), dtype)
    return m, torch.from_numpy(m).to(DEV), cache, C


def mean_check(L, dtype, D, H, lengths, rng, cached, skipped=None):
    """Zero queries: every weight is exp(0) = 1, so out is the mean of integer rows -- the float64 mean rounded once, and
    aggregate(reduce="mean") bit for bit -- and lse = 0 + logf(count) within the 2 ulp HIP documents for its logf (log 1 = 0 exactly)."""
    offsets, ids = segments(lengths, rng, skipped=skipped)
    table, X = stored(rng.integers(-8, 9, (N, D)).astype(np.float32), dtype)
    m, node_map, cache, C = cache_of(X, dtype) if cached else (None,) * 4
    want, live = aggregate_ref.aggregate(X, offsets, ids, "mean", None, m, C)
    queries = np.zeros((len(lengths), H, D), np.float32)
    for out_dtype in ("float32", "bfloat16"):
        out, scores, lse = run(L, dtype, out_dtype, table, D, offsets, ids, queries, None, 0.25, cache, node_map)
        mean = aggregate_ref.final(want, live, "mean", out_dtype == "bfloat16")
        for h in range(H):
            same(out[:, h], mean, f"{dtype} D {D} head {h} of {H} -> {out_dtype}")
        same(out[:, 0], run_aggregate(L, dtype, out_dtype, table, D, offsets, ids, "mean", None, cache, node_map), "aggregate's mean")
        assert np.all(scores == 0)
        some = live > 0
        log_count = np.log(live[some].astype(np.float64))[:, None]
        assert np.all(lse[~some] == -np.inf) and np.all(np.abs(lse[some] - log_count) <= 2 * np.spacing(np.float32(log_count)))
    return live


@pytest.mark.parametrize("cached", [False, True], ids=["no-cache", "cache"])
@pytest.mark.parametrize("H", [1, 3, 8])
@pytest.mark.parametrize("dtype,D", SHAPES)
def test_zero_queries_are_the_mean_exactly(hip, dtype, D, H, cached):
    G = groups(dtype, D)
    lengths = [0, 1, max(G - 1, 0), G + 1, K - 1, K, K + 1, 3 * K + 5, 9]
    live = mean_check(hip, dtype, D, H, lengths, np.random.default_rng(D + H), cached, skipped=8)
    assert live[8] == 0 and live[7] > 2 * K, "a segment of dead ids only, a hub of four chunks"


def test_more_chunks_than_the_grid_has_waves(hip):
    rng = np.random.default_rng(7)
    live = mean_check(hip, "float32", 4, 1, rng.integers(1, 3, WAVES + 37).tolist(), rng, False)
    assert live.size > WAVES and np.any(live[WAVES:] > 0)


@pytest.mark.parametrize("with_queries", [True, False], ids=["queries", "bias-only"])
@pytest.mark.parametrize("H", [1, 3, 8])
@pytest.mark.parametrize("dtype,D", [("float32", 20), ("bfloat16", 128)])
def test_a_dominant_integer_logit_selects_its_row_exactly(hip, dtype, D, H, with_queries):
    """Integer rows, queries and biases: every logit is an exact float32.  One entry's bias lifts it 200 above every other logit of its
    segment and head, so every other weight is expf(<= -200) = 0: out is that row, lse its logit, bit for bit -- wherever the entry
    lies (first, last, a group other than 0, the last of four chunks; another entry for every head).  Segment 2 has two tied dominant
    entries in different chunks: out = (x_a + x_b) / 2, exactly.  Without queries this is GAT's path; scores_out is the logit."""
    rng = np.random.default_rng(D + H)
    lengths = [9, 3 * K + 5, 3 * K + 5]
    offsets, ids = segments(lengths, rng)
    table, X = stored(rng.integers(-8, 9, (N, D)).astype(np.float32), dtype)
    queries = rng.integers(-2, 3, (3, H, D)).astype(np.float32) if with_queries else None
    if with_queries:
        queries[2] = 0                                                 # (the tie is the biases')
    bias = rng.integers(-5, 6, (ids.size, H)).astype(np.float32)
    top = np.float32(2 * 16 * D + 10 + 200)                            # |dot| <= 16 D, |bias| <= 5
    spots = {0: [0, 8, 1, 5], 1: [0, 3 * K + 4, 1, 2 * K + 44, 3 * K, K - 1, K, 77]}
    pick = np.zeros((3, H), np.int64)
    for d, where in spots.items():
        for h in range(H):
            pick[d, h] = offsets[d] + where[h % len(where)]
            bias[pick[d, h], h] = top
    tie = offsets[2] + np.array([10, 2 * K + 88])
    bias[tie] = top
    ids[np.concatenate([pick[:2].ravel(), tie])] = rng.integers(0, N, 2 * H + 2)       # live, whatever segments() drew
    dead = (ids < 0) | (ids >= N)
    out, scores, lse = run(hip, dtype, "float32", table, D, offsets, ids, queries, bias, 1.0)
    want = ref.attention(X, offsets, ids, queries, bias, 1.0)
    for d in (0, 1):
        for h in range(H):
            same(out[d, h], X[ids[pick[d, h]]], f"segment {d} head {h}")
            assert lse[d, h] == scores[pick[d, h], h] == np.float32(want[1][pick[d, h], h])
    same(out[2], np.broadcast_to((X[ids[tie[0]]] + X[ids[tie[1]]]) / np.float32(2), (H, D)).copy(), "two tied entries")
    assert np.all(np.abs(lse[2] - want[2][2]) <= 2.0 ** -23 * (np.abs(want[2][2]) + 1))
    same(scores, want[1].astype(np.float32), "scores_out")
    assert dead.any() and np.all(scores[dead] == 0) and (with_queries or np.all(scores[~dead] == bias[~dead]))


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_random_floats_within_the_derived_bound(hip, dtype):
    """u = 2^-24.  (1) A logit is D fmas, the product with scale and the sum with bias: |s^ - s| <= delta = (D + 2) u (scale sum |q x| +
    |bias|), the worst entry of the segment -- the bound of scores_out.  (2) An entry's weight relative to the final maximum is its
    own expf times the rescales on its way: one per block of its group (at most 256 / (G B) <= 32), one per level of the group tree
    (<= 6) and one chunk merge, 40 exponentials at the most, each within 1 ulp (2^-23, HIP's documented expf) of the exponential
    of an argument rounded once (u |argument|; the arguments of a chain telescope to at most the segment's logit range S, as the
    entry's own does): log-error eta = delta + 40 2^-23 + 2 u S.  (3) Numerator and l are float32 sums of len terms with one
    rescale rounding a step, and one division: (len + 3) u each.  A normalised weight moves by at most 2 eta relatively, and
    sum alpha |x| <= max |x|: |out^ - out| <= (2 eta + 2 (len + 3) u) max |x|.  lse = m + logf(l): delta + 40 2^-23 + 2 u S for
    the weights, (len + 3) u for the sum, 2^-22 log(len) for logf (2 ulp), u |lse| for the sum with m.  bf16 out: rounding is
    monotone, so out^ lies between the rounded ends of the bound."""
    rng = np.random.default_rng(11)
    D, H, scale = 128, 4, float(np.float32(128 ** -0.5))
    lengths = [1, 2, 3, 7, K - 1, K, K + 1, 1001]
    offsets, ids = segments(lengths, rng)
    ids[:13] = np.abs(ids[:13]) % N                                    # (the four short segments: live entries only)
    table, X = stored(rng.standard_normal((N, D)).astype(np.float32), dtype)
    queries = rng.standard_normal((len(lengths), H, D)).astype(np.float32)
    bias = rng.standard_normal((ids.size, H)).astype(np.float32)
    want, want_s, want_lse, live, mass = ref.attention(X, offsets, ids, queries, bias, scale)
    ln = np.array(lengths, np.float64)[:, None]
    seg = np.repeat(np.arange(len(lengths)), lengths)
    xmax = np.array([np.abs(X[ids[a:b][(ids[a:b] >= 0) & (ids[a:b] < N)]]).max() for a, b in zip(offsets[:-1], offsets[1:])])
    S = np.array([np.ptp(want_s[a:b][(ids[a:b] >= 0) & (ids[a:b] < N)], axis=0) for a, b in zip(offsets[:-1], offsets[1:])])
    delta = (D + 2) * U24 * (mass + np.abs(bias).max())
    eta = delta + 40 * 2.0 ** -23 + 2 * U24 * S
    bound = (2 * eta + 2 * (ln + 3) * U24)[:, :, None] * xmax[:, None, None]
    lse_bound = eta + (ln + 3) * U24 + 2.0 ** -22 * np.log(ln) + U24 * np.abs(want_lse)
    out, scores, lse = run(hip, dtype, "float32", table, D, offsets, ids, queries, bias, scale)
    worst = [float(np.max(np.abs(out - want) / bound)), float(np.max(np.abs(scores - want_s) / delta[seg])), float(np.max(np.abs(lse - want_lse) / lse_bound))]
    print(f"{dtype}: worst fraction of the bound: out {worst[0]:.4f} scores {worst[1]:.4f} lse {worst[2]:.4f}")
    assert max(worst) <= 1, worst
    narrow = lambda v: aggregate_ref.final(v.reshape(-1, D), None, "sum", True).reshape(v.shape)
    out16 = run(hip, dtype, "bfloat16", table, D, offsets, ids, queries, bias, scale)[0]
    assert np.all((narrow(want - bound) <= out16) & (out16 <= narrow(want + bound)))
    same(run(hip, dtype, "float32", table, D, offsets, ids, queries, bias, scale)[0], out, "the same call twice")


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
        got, lse = graph.full_neighbor_attention(feature, rows, q, return_lse=True)
        offsets, _, src = graph.in_edges(rows)
        offsets, src = offsets.cpu().numpy(), src.cpu().numpy()
        want, want_s, want_lse, live, _ = ref.attention(X, offsets, src, q, None, np.float32(D ** -0.5))
        assert got.shape == (rows.size, H, D) and live.max() == 700 and (live == 0).sum() >= 2
        tol = 1e-4 * np.abs(X).max()                                   # (the bound itself: test_random_floats; here the plumbing)
        assert np.allclose(got.cpu().numpy(), want, rtol=0, atol=tol) and np.allclose(lse.cpu().numpy(), want_lse, rtol=0, atol=1e-4)
        # [n, D] queries: one head, [n, D] back; scale=None is 1 / sqrt(D); every extra; a bf16 result
        flat, scores, lse = feature.attention(offsets, src, queries=q[:, 1], return_scores=True, return_lse=True)
        assert flat.shape == (rows.size, D) and scores.shape == (src.size, 1) and lse.shape == (rows.size, 1)
        assert torch.equal(flat, got[:, 1]) and np.allclose(scores.cpu().numpy()[:, 0], want_s[:, 1], rtol=0, atol=1e-4)
        out16 = feature.attention(offsets, src, queries=q, out_dtype="bfloat16")
        assert out16.dtype == torch.bfloat16 and torch.equal(out16, got.to(torch.bfloat16))
        b = rng.integers(-3, 4, (src.size, H)).astype(np.float32)
        same(feature.attention(offsets, src, bias=b, return_scores=True)[1].cpu().numpy(), ref.attention(X, offsets, src, None, b)[1].astype(np.float32), "bias")
        empty = feature.attention(np.zeros(4, np.int64), np.zeros(0, np.int32), queries=q[:3], return_lse=True)
        assert empty[0].cpu().tolist() == [[[0.0] * D] * H] * 3 and torch.all(empty[1] == -np.inf)
    finally:
        torch.cuda.synchronize()
        graph.close()
        feature.close()
