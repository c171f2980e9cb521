"""Induced edges at edge offsets beyond 2^31 and 2^32: the layout of tests/far_rows.py, whose live rows straddle the boundary behind
ballast rows of L zeros, put on the device by far_rows.device_world.  The rows are far_rows.expand_rows': live rows on both sides of the
boundary, the straddling hub and one ballast row in the middle.  The set holds every other live vertex, the straddling hub among them,
in descending order (local != global), so the kept edge ids lie on both sides of the boundary and col is read beyond it; every entry of
the ballast row is vertex 0: without it in the set the row's whole tiles keep nothing and are skipped, with it they keep all 1 024
slots.  A failure at 5000 is a fault at any size; at 2^31 but not at 5000 an offset that went through a signed 32-bit value; at 2^32
only, through an unsigned one: the model of e in 32 bits differs at the two far boundaries and nowhere at 5000."""
import numpy as np
import pytest
import torch

from tests import far_rows
from tests import induced_ref as ref
from tests.compare import same_arrays
from tests.test_gpu_induced import NAMES, abi

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module", params=list(far_rows.BOUNDARIES))
def world(hip, request):
    """The whole graph on the device at one boundary (far_rows.device_world)."""
    with far_rows.device_world(hip, request.param) as w:
        yield w


def node_set(g, with_zero):
    live = np.arange(g.B, g.node_num, dtype=np.int32)
    nodes = live[(live - g.hub) % 2 == 0][::-1]
    assert g.hub in nodes and (g.indptr[nodes] < g.boundary).sum() >= 50 and (g.indptr[nodes] >= g.boundary).sum() >= 50, "both sides"
    return np.concatenate([nodes, [0]]).astype(np.int32) if with_zero else nodes.copy()


def want_induced(g, with_zero, m=None):
    """(rows, offsets, m, nodes, K, dst, src_local, true eids)."""
    ballast_row = g.B - 2
    rows, offsets, i, r, eid, is_live, src = far_rows.expand_rows(g, ballast_row, m)
    M = int(offsets[-1])
    m = M if m is None else m
    nodes = node_set(g, with_zero)
    local = ref.pos(nodes, src)
    kept = (src >= 0) & (local >= 0)
    assert g.deg[ballast_row] == g.L >= 64 and (~is_live).sum() == min(g.L, max(m - int(offsets[300]), 0)), "one ballast row"
    assert np.all(kept[~is_live] == with_zero), "the ballast row is kept whole or not at all"
    low, high = kept & is_live & (eid < g.boundary), kept & is_live & (eid >= g.boundary)
    assert low.sum() >= 10 and high.sum() >= 10, "kept live edge ids on both sides"
    hub = r == g.hub
    assert (hub & low).sum() >= 3 and (hub & high).sum() >= 3, "the straddling row keeps entries on both sides"
    assert (is_live & (src >= 0) & ~kept).sum() >= 100, "the set thins the live rows"
    assert np.all(local[kept & is_live] != src[kept & is_live]), "local != global"
    wrapped = ((eid + 2 ** 31) % 2 ** 32) - 2 ** 31                           # e through a signed 32-bit value
    changed = int((wrapped[kept] != eid[kept]).sum())
    assert changed >= 10 if g.boundary >= 2 ** 31 else changed == 0, "e in 32 bits differs at the far boundaries only"
    assert M < 2 ** 21 + 2 ** 16
    return rows, offsets, m, nodes, int(kept.sum()), i.astype(np.int32)[kept], local[kept], eid[kept]


@pytest.mark.parametrize("with_zero", [False, True], ids=["ballast-skipped", "ballast-kept"])
def test_induced_edges(world, with_zero):
    g = world["g"]
    rows, off, m, nodes, K, dst, local, eid = want_induced(g, with_zero)
    got = world["graph"].induced_edges(torch.from_numpy(rows).to(DEV), nodes, return_eids=True)
    torch.cuda.synchronize()
    assert got[0].shape == (K,), f"K {got[0].shape[0]} want {K}" + world["why"]
    same_arrays(got, (dst, local, eid), f"with vertex 0 {with_zero}" + world["why"], names=NAMES)


def test_a_prefix_through_the_c_abi(world):
    """m ends inside the ballast row, and the capacity lies above K: the eid_out stores and the col reads lie on both sides."""
    g = world["g"]
    m = int(want_induced(g, False)[1][300]) + g.L // 2 + 3
    rows, off, m, nodes, K, dst, local, eid = want_induced(g, True, m)
    assert m % ref.TILE != 0 and K >= g.L // 2
    k, *out = abi(world["L"], world["graph"], rows, off, m, nodes, K + 5)
    assert k == K, f"K {k} want {K}" + world["why"]
    same_arrays([x[:k] for x in out], (dst, local, eid), "prefix" + world["why"], names=NAMES)
    assert all(np.all(x[k:] == -1) for x in out)
