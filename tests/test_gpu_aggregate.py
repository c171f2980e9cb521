"""legion_aggregate_rows and its Python surface on the GPU against tests/aggregate_ref.py.  Features are small integers and weights
come from {0.5, 1, 2, -1}, so every float32 sum is exact whatever its order: sums, weighted sums and maxima equal the float64
reference exactly, the mean equals float32(sum) / float32(count), bf16 output its round to nearest even.  One list of segments holds
every length at which the kernel takes another path (the groups G of a row width, the chunk K = 256, a hub of 20 K), skipped ids and
a segment of skipped ids only; cache rows differ from the table's by 1000, so a wrong source shows."""
import ctypes

import numpy as np
import pytest
import torch

from tests import aggregate_ref as ref

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

DEV = "cuda:0"
N, K = 500, 256
REDUCE = {"sum": 0, "mean": 1, "max": 2}
WAVES = 2048 * 4                                                       # the grid's waves: chunks past them are a second trip
SHAPES = [("float32", D) for D in (1, 3, 4, 100, 128, 260)] + [("bfloat16", D) for D in (8, 100, 128, 520)]


def groups(dtype, D):
    """G: the rows a wave has in flight (legion_hip.h, rule 9)."""
    units = -(-D // 8) if dtype == "bfloat16" else (D // 4 if D % 4 == 0 else D)
    return 64 // min(64, 1 << (units - 1).bit_length())


def segments(lengths, rng, skipped=None):
    """offsets and ids of segments of these lengths: ids repeat (N is small), one in sixteen is -1 or N; segment `skipped` only those."""
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    ids = rng.integers(0, N, int(offsets[-1])).astype(np.int32)
    dead = rng.integers(0, 16, ids.size) == 0
    ids[dead] = np.where(rng.integers(0, 2, int(dead.sum())) == 0, -1, N)
    if skipped is not None:
        ids[offsets[skipped]:offsets[skipped + 1]] = np.resize(np.array([-1, N, N + 7, -(2 ** 31)], np.int32), lengths[skipped])
    return offsets, ids


def stored(values, dtype):
    """(the table on the device as the library stores it, the values it holds as float32).  bf16: rows round_up(D, 8) apart, the pad
    filled with 77 -- a pad that reaches out shows."""
    x = torch.from_numpy(values)
    if dtype == "float32":
        return x.to(DEV), values
    table = torch.full((x.shape[0], (x.shape[1] + 7) // 8 * 8), 77.0, dtype=torch.bfloat16)
    table[:, :x.shape[1]] = x.to(torch.bfloat16)
    return table.to(DEV), table[:, :x.shape[1]].float().numpy()


def run(L, dtype, out_dtype, table, D, offsets, ids, reduce, weights=None, cache=None, node_map=None):
    """The C ABI over an output filled with a sentinel and a scratch filled with NaN bits; returns out as float32 numpy."""
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    n, M = offsets.size - 1, ids.size
    d_off, d_ids = torch.from_numpy(offsets).to(DEV), torch.from_numpy(ids).to(DEV)
    d_w = torch.from_numpy(weights).to(DEV) if weights is not None else None
    out = torch.full((n + 1, D), -12288.0, dtype=torch.float32 if out_dtype == "float32" else torch.bfloat16, device=DEV)
    nbytes = int(L.legion_aggregate_scratch_bytes(n, M, D))
    scratch = torch.full((nbytes // 8 + 2,), -1, dtype=torch.int64, device=DEV)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    code = {"float32": 0, "bfloat16": 1}
    assert L.legion_aggregate_rows(s, code[dtype], code[out_dtype], P(table), P(cache), P(node_map), D, N, P(d_off), n, P(d_ids), M,
                                   P(d_w), REDUCE[reduce], P(out), P(scratch), nbytes) == 0
    torch.cuda.synchronize()
    got = out.float().cpu().numpy()
    assert np.all(got[n] == -12288.0), "written past row n"
    return got[:n]


def same(got, want, what):
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, f"{what}: {len(bad)} elements differ, first at {bad[0]}: got {got[tuple(bad[0])]} want {want[tuple(bad[0])]}"


@pytest.mark.parametrize("cached", [False, True], ids=["no-cache", "cache"])
@pytest.mark.parametrize("reduce,weighted", [("sum", False), ("sum", True), ("mean", False), ("max", False)])
@pytest.mark.parametrize("dtype,D", SHAPES)
def test_exact_against_the_reference(hip, dtype, D, reduce, weighted, cached):
    rng = np.random.default_rng(D)
    G = groups(dtype, D)
    lengths = [0, 1, max(G - 1, 0), G, G + 1, K - 1, K, K + 1, 2 * K + 1, 20 * K + 3, 9, 0]
    offsets, ids = segments(lengths, rng, skipped=10)
    weights = rng.choice(np.array([0.5, 1, 2, -1], np.float32), ids.size) if weighted else None
    table, X = stored(rng.integers(-8, 9, (N, D)).astype(np.float32), dtype)
    cache = node_map = C = None
    if cached:                                                         # a third of the ids hit; their rows are the table's + 1000
        m = np.where(np.arange(N) % 3 == 0, np.arange(N) // 3, -2).astype(np.int32)
        node_map = torch.from_numpy(m).to(DEV)
        cache, C = stored(X[::3] + np.float32(1000), dtype)
    want, live = ref.aggregate(X, offsets, ids, reduce, weights, m if cached else None, C)
    mass, _ = ref.aggregate(np.abs(X), offsets, ids, "sum", None if weights is None else np.abs(weights), m if cached else None,
                            np.abs(C) if cached else None)
    assert live[10] == 0 and live[9] > 18 * K,"a segment of skipped ids only, a hub"
    assert np.all(mass < 2 ** 23), "halves below 2^23: every partial sum is exact in float32, in any order"
    for out_dtype in ("float32", "bfloat16"):
        got = run(hip, dtype, out_dtype, table, D, offsets, ids, reduce, weights, cache, node_map)
        same(got, ref.final(want, live, reduce, out_dtype == "bfloat16"), f"{dtype} D {D} {reduce} -> {out_dtype}")
        again = run(hip, dtype, out_dtype, table, D, offsets, ids, reduce, weights, cache, node_map)
        same(again, got, "the same call twice")


def test_more_chunks_than_the_grid_has_waves(hip):
    rng = np.random.default_rng(7)
    lengths = rng.integers(1, 3, WAVES + 37).tolist()
    offsets, ids = segments(lengths, rng)
    table, X = stored(rng.integers(-8, 9, (N, 4)).astype(np.float32), "float32")
    want, live = ref.aggregate(X, offsets, ids)
    assert len(lengths) > WAVES and np.any(want[WAVES:] != 0)
    same(run(hip, "float32", "float32", table, 4, offsets, ids, "sum"), ref.final(want, live, "sum"), "past the grid")


@pytest.mark.parametrize("reduce", ["sum", "mean"])
def test_random_floats_within_the_bound_of_a_float32_sum(hip, reduce):
    """|error| <= (len + 2) 2^-24 sum |w x|: the standard bound of a float32 sum in any order (the mean: that over the count, its
    one more rounding inside the + 2)."""
    rng = np.random.default_rng(11)
    lengths = [0, 1, 2, 3, K - 1, K, K + 1, 2 * K + 1, 20 * K + 3]
    offsets, ids = segments(lengths, rng)
    table, X = stored(rng.standard_normal((N, 128)).astype(np.float32), "float32")
    want, live = ref.aggregate(X, offsets, ids, reduce)
    mass, _ = ref.aggregate(np.abs(X), offsets, ids, reduce)
    count = np.maximum(live, 1)[:, None] if reduce == "mean" else 1
    got = run(hip, "float32", "float32", table, 128, offsets, ids, reduce)
    bound = (np.array(lengths)[:, None] + 2) * 2.0 ** -24 * mass / count
    assert np.all(np.abs(got.astype(np.float64) - want / count) <= bound), float(np.max(np.abs(got - want / count) - bound))


def test_the_python_surface(hip):
    from legion_amd import engine
    rng = np.random.default_rng(3)
    V, D = 300, 20
    deg = rng.integers(0, 12, V)
    deg[5] = 700
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = rng.integers(0, V, int(indptr[-1])).astype(np.int32)
    X = rng.integers(-8, 9, (V, D)).astype(np.float32)
    graph = engine.GraphStorage(1, torch.from_numpy(indptr).to(DEV), torch.from_numpy(col).to(DEV))
    feature = engine.FeatureStorage(1, torch.from_numpy(X).to(DEV))
    try:
        rows = np.concatenate([rng.permutation(V)[:90], [5, 5, -1, V]]).astype(np.int32)
        got = graph.full_neighbor_aggregate(feature, rows, reduce="mean")
        offsets, _, src = graph.in_edges(rows)
        want, live = ref.aggregate(X, offsets.cpu().numpy(), src.cpu().numpy(), "mean")
        assert got.shape == (rows.size, D) and live.max() == 700 and (live == 0).sum() >= 2
        same(got.cpu().numpy(), ref.final(want, live, "mean"), "full_neighbor_aggregate")
        # a pinsage_neighbors-shaped list: [n, k] neighbours padded with -1, the visit counts as weights
        n, k = 50, 7
        nbrs = rng.integers(0, V, (n, k)).astype(np.int32)
        nbrs[rng.integers(0, 3, (n, k)) == 0] = -1
        counts = rng.integers(1, 9, (n, k)).astype(np.float32)
        offsets = np.arange(n + 1, dtype=np.int64) * k
        got = feature.aggregate(offsets, torch.from_numpy(nbrs).to(DEV).reshape(-1), weights=counts.reshape(-1))
        want, live = ref.aggregate(X, offsets, nbrs.reshape(-1), "sum", counts.reshape(-1))
        same(got.cpu().numpy(), ref.final(want, live, "sum"), "aggregate")
        assert feature.aggregate(np.zeros(4, np.int64), np.zeros(0, np.int32), reduce="max").cpu().tolist() == [[0.0] * D] * 3
    finally:
        torch.cuda.synchronize()
        graph.close()
        feature.close()
