"""The weighted table build (kernels_weights.hip) past both of its capped grids, bit for bit against tests/setup_ref.cdf_segmented.

    edge_cdf_rows_kernel         8192 workgroups x 4 waves x 64 rows = 2 097 152 rows a pass     2^21 + 4099 rows, nearly all empty
    edge_cdf_long_rows_kernel    512 workgroups, one long row each                               more than 600 rows of 4097 entries

Short rows of 1 to 130 entries stand in the first block of 64 rows, in the blocks on both sides of row 2 097 152 (the last of the first
pass, the first of the second) and in the last block, which has 3 rows; a 4096-entry row and a 4097-entry row are neighbours (the last row
of the wave class beside the first of the workgroup class); long rows stand in both passes.  Weights are eighths with runs of zeros, so
every partial sum is exact and the table is the reference's whatever the order of the additions."""
import numpy as np
import pytest
import torch

from tests import setup_ref as ref

DEV = "cuda:0"
N_ROWS = (1 << 21) + 4099
N_LONG = 600
LONG_DEG = ref.CDF_LONG + 1


def stride_rows():
    rng = np.random.RandomState(61)
    deg = np.zeros(N_ROWS, dtype=np.int64)
    short = np.concatenate([np.arange(0, 64), np.arange(ref.PASS_CDF_ROWS - 130, ref.PASS_CDF_ROWS + 131), np.arange(N_ROWS - 3, N_ROWS),
                            rng.randint(64, N_ROWS - 64, 300)])
    deg[short] = rng.randint(1, 131, short.size)
    deg[[0, 63, ref.PASS_CDF_ROWS - 1, ref.PASS_CDF_ROWS, N_ROWS - 1]] = [130, 1, 129, 65, 64]
    long = 1000 + 3491 * np.arange(N_LONG - 10)                              # 590 in the first pass ...
    assert long.max() < ref.PASS_CDF_ROWS - 1000
    deg[long] = LONG_DEG
    deg[ref.PASS_CDF_ROWS + 200 + 300 * np.arange(12)] = LONG_DEG             # ... 12 in the second
    deg[[70_000, 70_001]] = [ref.CDF_LONG, LONG_DEG]
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    E = int(indptr[-1])
    w = (rng.randint(1, 33, E) / 8).astype(np.float32)
    for v in np.nonzero(deg >= 2)[0]:
        s, n = int(indptr[v]), int(deg[v])
        k = int(v) % 7
        if k in (0, 1):
            w[s:s + max(n // 5, 1)] = 0                                       # a leading run of zeros
        if k in (1, 2):
            w[s + n - max(n // 7, 1):s + n] = 0                               # a trailing run
        if n >= 60 and k != 3:
            w[s + n // 2:s + n // 2 + n // 9] = 0                             # an inner run, across a wave's / a step's boundary
    return indptr, w


@pytest.fixture(scope="module")
def rows():
    indptr, w = stride_rows()
    return {"indptr": indptr, "w": w, "want": ref.cdf_segmented(indptr, w)}


def test_rows_cross_both_caps(rows):
    """From indptr alone, before any launch."""
    deg = np.diff(rows["indptr"])
    assert deg.size == N_ROWS > ref.PASS_CDF_ROWS
    assert (deg > ref.CDF_LONG).sum() > ref.PASS_CDF_LONG_ROWS, "more long rows than the second launch has workgroups"
    assert (deg[ref.PASS_CDF_ROWS:] > 0).sum() > 100 and (deg[ref.PASS_CDF_ROWS:] > ref.CDF_LONG).sum() >= 10
    assert 0 < N_ROWS % ref.CDF_BLOCK < ref.CDF_BLOCK and deg[-(N_ROWS % ref.CDF_BLOCK):].min() > 0, "a partial last block, with entries"
    assert deg[:64].min() > 0 and deg[ref.PASS_CDF_ROWS - 64:ref.PASS_CDF_ROWS + 64].min() > 0
    pair = np.nonzero(deg == ref.CDF_LONG)[0]
    assert pair.size == 1 and deg[pair[0] + 1] == ref.CDF_LONG + 1
    assert (deg == 0).mean() > 0.99 and deg.max() == LONG_DEG


def test_reference_table_over_these_rows(rows):
    """Exact sums: every entry is a multiple of 1/8 below 2^15, a zero weight repeats its predecessor, a row restarts from its own first
    entry -- and a long row whose second step of 1024 started from 0 again, or a second pass that never ran, would differ."""
    indptr, w, want = rows["indptr"], rows["w"], rows["want"]
    assert np.array_equal(want * 8, np.round(want * 8)) and want.max() < (1 << 15)
    first = indptr[:-1][np.diff(indptr) > 0]
    assert np.array_equal(want[first], w[first])
    prev = np.concatenate([[np.float32(0)], want[:-1]])
    inner = np.ones(w.size, dtype=bool)
    inner[first] = False
    assert np.array_equal(want[inner & (w == 0)], prev[inner & (w == 0)]) and (w == 0).mean() > 0.1
    long = np.nonzero(np.diff(indptr) > ref.CDF_LONG)[0]
    assert all(want[indptr[v] + 1024] > want[indptr[v] + 1023] >= 100 for v in long[[0, 1, ref.PASS_CDF_LONG_ROWS, -1]])
    assert want[indptr[ref.PASS_CDF_ROWS]:].max() > 0


@pytest.mark.gpu
def test_table_past_both_grid_caps(hip, rows):
    from legion_amd import engine
    indptr, w, want = rows["indptr"], rows["w"], rows["want"]
    col = (np.arange(w.size, dtype=np.int64) % N_ROWS).astype(np.int32)
    graph = engine.GraphStorage(1, torch.from_numpy(indptr).to(DEV), torch.from_numpy(col).to(DEV))
    try:
        graph.set_edge_weights(w)
        torch.cuda.synchronize()
        got = graph.edge_cdf().cpu().numpy()
        assert got.dtype == np.float32 and got.shape == want.shape
        bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
        rows_of = np.searchsorted(indptr, bad[:5], side="right") - 1
        assert bad.size == 0, f"{bad.size} entries differ, first at {bad[:5]} (rows {rows_of}): got {got[bad[:5]]} want {want[bad[:5]]}"
    finally:
        torch.cuda.synchronize()
        graph.close()
