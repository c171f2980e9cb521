"""Layer-neighbour sampling at edge offsets beyond 2^31 and 2^32: the layout of tests/far_rows.py, whose live rows straddle the boundary
behind ballast rows of L zeros, put on the device by far_rows.device_world.  The seeds are live rows on both sides of the
boundary, the straddling hub and one ballast row in the middle, so the kept edge ids lie on both sides of the boundary and col is read
beyond it.  Every entry of the ballast row is vertex 0, which has one number: at fan-out 5 the row keeps nothing (whole tiles of it), at
a fan-out of its degree everything (whole tiles again).  Through m a prefix that ends inside the ballast row is looked at; its degree
stays L.  The whole column array exists on the device only.  A failure at 5000 is a fault at any size; at 2^31 but not at 5000 an offset
that went through a signed 32-bit value; at 2^32 only, through an unsigned one.  No row of these layouts has 2^32 entries (L is 2^20 at
most), so a product h * d truncated to 64 bits cannot differ here: labor_rule.h's table (tests/cpu/labor_rule_test.cpp) is where degrees
from 2^32 on are pinned, over the text the device runs."""
import numpy as np
import pytest
import torch

from tests import far_rows
from tests import labor_ref as ref
from tests.compare import same_arrays
from tests.test_gpu_labor import abi

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SALT = 0                                                           # labor_hash(0, 0) = 0xa706dd2f: 0.65 of 2^32
NAMES = ("dst", "src", "eid")


@pytest.fixture(scope="module", params=list(far_rows.BOUNDARIES))
def world(hip, request):
    """The whole graph on the device at one boundary (far_rows.device_world)."""
    with far_rows.device_world(hip, request.param) as w:
        yield w


def want_labor(g, fanout, m=None):
    """(rows, offsets, m, K, dst, src, true eids): the live seeds of the layout with the straddler every fifth, one whole ballast row in
    the middle and every live row once behind it; m None: every slot, else the first m.  The live entries come from the reference view,
    the ballast row's are vertex 0."""
    ballast_row = g.B - 2
    rows, offsets, i, r, eid, is_live, src = far_rows.expand_rows(g, ballast_row, m)
    M = int(offsets[-1])
    m = M if m is None else m
    ok = src >= 0
    kept = np.zeros(m, dtype=bool)
    kept[ok] = ref.keeps(ref.hashes(src[ok], SALT), g.deg[r[ok]], fanout)
    # what makes the case worth running at this boundary
    assert g.deg[ballast_row] == g.L >= 64 and (~is_live).sum() == min(g.L, max(m - int(offsets[300]), 0)), "one ballast row"
    whole = ref.keep_one(ref.hashes([0], SALT)[0], g.L, fanout)
    assert whole == (fanout >= g.L) and np.all(kept[~is_live] == whole), "the ballast row is kept whole or not at all"
    if m == M:
        low, high = kept & is_live & (eid < g.boundary), kept & is_live & (eid >= g.boundary)
        assert low.sum() >= 10 and high.sum() >= 10, "kept live edge ids on both sides"
        hub = r == g.hub
        assert fanout < g.L or ((hub & low).sum() >= 3 and (hub & high).sum() >= 3), "the straddling row keeps entries on both sides"
        assert (ok & is_live & ~kept).sum() >= 100 or fanout >= g.L, "the predicate thins the live rows"
    assert M < 2 ** 21 + 2 ** 16
    return rows, offsets, m, int(kept.sum()), i.astype(np.int32)[kept], src[kept], eid[kept]


def test_labor_edges(world):
    g = world["g"]
    for fanout in (5, g.L):                                            # the ballast row keeps nothing, then everything
        rows, off, m, K, dst, src, eid = want_labor(g, fanout)
        got = world["graph"].labor_edges(torch.from_numpy(rows).to(DEV), fanout, salt=SALT, return_eids=True)
        torch.cuda.synchronize()
        assert got[0].shape == (K,), f"fanout {fanout}: K {got[0].shape[0]} want {K}" + world["why"]
        same_arrays(got, (dst, src, eid), f"fanout {fanout}" + world["why"], names=NAMES)


def test_a_prefix_that_ends_inside_the_ballast_row(world):
    """m ends inside the ballast row, L / 2 + 3 slots into it, and the fan-out is that number: with the row's whole degree L vertex 0's
    number decides (at this salt: not kept), with the slots below m as the degree every one of them would be kept."""
    g = world["g"]
    below = g.L // 2 + 3
    m = int(want_labor(g, 5)[1][300]) + below
    rows, off, m, K, dst, src, eid = want_labor(g, below, m)
    assert m - int(off[300]) == below < g.L and m % ref.TILE != 0
    assert not ref.keep_one(ref.hashes([0], SALT)[0], g.L, below) and ref.keep_one(ref.hashes([0], SALT)[0], below, below)
    assert np.all(rows[dst] >= g.B) and K >= 100, "live entries only"
    k, *out = abi(world["L"], world["graph"], rows, off, m, below, SALT, K + 5)
    assert k == K, f"K {k} want {K} ({K + below} if the degree were the slots below m)" + world["why"]
    same_arrays([x[:k] for x in out], (dst, src, eid), "prefix" + world["why"], names=NAMES)
    assert all(np.all(x[k:] == -1) for x in out)
