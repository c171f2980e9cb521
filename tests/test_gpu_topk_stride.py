"""The grid-stride loops of legion_row_topk: n = three trips of the capped wave-per-row grid (LG_TOPK_GRID workgroups of four waves:
8 192 rows a trip) plus 5 rows, and 300 of them rows of the workgroup class, more than the LG_TOPK_LONG_GRID = 256 workgroups of the
second launch, so that both loops go round.  Bit for bit against tests/topk_ref.py; a trip that repeated the rows one stride earlier, and
a second launch that stopped after its first trip, are shown from the reference to differ before anything runs."""
import numpy as np
import pytest
import torch

from tests import topk_ref as ref
from tests.test_gpu_topk import abi, compare

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHORT_ROWS = 400
LONG_DEGREES = [4097, 5000, 9001]
N_ROWS = 3 * ref.GRID_ROWS + 5
N_LONG = 300
K = 25


def stride_graph():
    rng = np.random.RandomState(77)
    deg = np.concatenate([rng.randint(0, 131, SHORT_ROWS), LONG_DEGREES]).astype(np.int64)
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    E, N = int(indptr[-1]), deg.size
    col = rng.randint(0, N, E).astype(np.int32)
    col[rng.rand(E) < 0.03] = -1
    w = (rng.randint(0, 33, E) / 8).astype(np.float32)
    rows = rng.randint(-1, SHORT_ROWS + 1, N_ROWS).astype(np.int32)
    rows[rows == SHORT_ROWS] = N                                   # outside the graph
    at = rng.choice(N_ROWS, N_LONG, replace=False)
    rows[at] = SHORT_ROWS + rng.randint(0, len(LONG_DEGREES), N_LONG)
    rows[-1] = SHORT_ROWS + 2                                      # the last row of the last trip is a long one
    return indptr, col, w, rows


def test_both_grid_stride_loops(hip):
    from legion_amd import engine
    indptr, col, w, rows = stride_graph()
    long = np.nonzero((rows >= SHORT_ROWS) & (rows < indptr.size - 1))[0]
    assert rows.size == N_ROWS > 3 * ref.GRID_ROWS and long.size > ref.LONG_GRID and np.all(np.diff(indptr)[rows[long]] > ref.LONG)
    wants = {mode: ref.row_topk(indptr, col, w, rows, K, mode, 9) for mode in (ref.LARGEST, ref.SAMPLE)}
    for mode, (src, eid, cnt) in wants.items():
        stale = np.concatenate([eid[:ref.GRID_ROWS], eid[:-ref.GRID_ROWS]])
        assert (stale != eid).any(axis=1).sum() > N_ROWS // 2, "a trip that repeats the one before differs"
        assert cnt[long[ref.LONG_GRID:]].min() == K, "the long rows beyond the first trip of the second launch have picks"
        assert (cnt == 0).sum() >= 50 and (cnt == K).sum() >= 1000
    graph = engine.GraphStorage(1, torch.from_numpy(indptr).to(DEV), torch.from_numpy(col).to(DEV))
    try:
        d_w = torch.from_numpy(w).to(DEV)
        for mode, want in wants.items():
            compare(abi(hip, graph, rows, K, mode, d_w, 9), want, f"mode {mode}")
    finally:
        torch.cuda.synchronize()
        graph.close()
