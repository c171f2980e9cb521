"""The per-row selection at edge offsets beyond 2^31 and 2^32: the layout of tests/far_rows.py, whose live rows straddle the boundary
behind ballast rows of L entries, put on the device with its weights by far_rows.device_world.  The rows are the live seeds of the
layout with the straddling hub every fifth, every live row once, and one whole ballast row (L = 2^20 at the far boundaries: a row of the
workgroup class, all of vertex 0 with weight 1) in the middle.  The hash takes the TRUE edge id and eid_out returns it, so a position
that went through 32 bits picks other entries and names other ids.  A failure at 5000 is a fault at any size; at 2^31 but not at 5000 an
offset that went through a signed 32-bit value; at 2^32 only, through an unsigned one."""
import numpy as np
import pytest
import torch

from tests import far_rows
from tests import topk_ref as ref
from tests.test_gpu_topk import abi, compare

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SALT = 5


@pytest.fixture(scope="module", params=list(far_rows.BOUNDARIES))
def world(hip, request):
    with far_rows.device_world(hip, request.param, weights=True) as w:
        yield w


def want_topk(g, k, mode):
    """(rows, src, true eids, counts) on the reference view; the ballast row's from a view of its own."""
    ballast_row = g.B - 2
    live = np.arange(g.B, g.node_num, dtype=np.int32)
    rows = np.concatenate([g.seeds(300), [ballast_row], live, [g.hub, -1, g.node_num]]).astype(np.int32)
    at = 300
    src, eid, cnt = ref.row_topk(g.indptr_ref, g.col_ref, g.w_ref, np.where(rows == ballast_row, -1, rows), k, mode, SALT, add=g.offset)
    L = int(g.deg[ballast_row])
    b = ref.row_topk(np.array([0, L], dtype=np.int64), np.zeros(L, np.int32), np.ones(L, np.float32), [0], k, mode, SALT,
                     add=int(g.indptr[ballast_row]))
    src[at], eid[at], cnt[at] = b[0][0], b[1][0], b[2][0]
    # what makes the case worth running at this boundary
    assert L == g.L and cnt[at] == min(k, L) and np.all(eid[at, :cnt[at]] < g.indptr[ballast_row + 1])
    took = eid >= 0
    live_rows = rows >= g.B
    low, high = took & (eid < g.boundary) & live_rows[:, None], took & (eid >= g.boundary)
    assert low.sum() >= 10 and high.sum() >= 10, "picked edge ids on both sides of the boundary"
    hub = np.nonzero(rows == g.hub)[0]
    if k >= 5:
        assert low[hub[0]].sum() >= 1 and high[hub[0]].sum() >= 1 or mode != ref.SAMPLE, "the straddling row's picks come from both sides"
    assert np.array_equal(eid[hub[0]], eid[hub[-1]]) and hub.size >= 3
    r = rows[np.nonzero(took)[0]].astype(np.int64)
    assert np.all(g.indptr[r] <= eid[took]) and np.all(eid[took] < g.indptr[r + 1])
    return rows, src, eid, cnt


@pytest.mark.parametrize("mode", ref.MODES, ids=["largest", "smallest", "sample"])
def test_row_topk(world, mode):
    g = world["g"]
    for k in (5, 64):
        rows, src, eid, cnt = want_topk(g, k, mode)
        got = abi(world["L"], world["graph"], rows, k, mode, world["w"], SALT)
        compare(got, (src, eid, cnt), f"k {k} mode {mode}" + world["why"])


def test_the_straddling_hub_is_sampled_from_both_sides(world):
    g = world["g"]
    rows, src, eid, cnt = want_topk(g, 64, ref.SAMPLE)
    hub = int(np.nonzero(rows == g.hub)[0][0])
    assert (eid[hub] < g.boundary).sum() >= 10 and (eid[hub] >= g.boundary).sum() >= 10
    got = world["graph"].sample_distinct(torch.from_numpy(rows).to(DEV), 64, weights=world["w"], salt=SALT, return_eids=True)
    torch.cuda.synchronize()
    compare((got[0], got[2], got[1]), (src, eid, cnt), "sample_distinct" + world["why"])
