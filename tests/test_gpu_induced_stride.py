"""Induced edges past one trip of the capped grid (2 048 workgroups), bit for bit against tests/induced_ref.py: seeds_for(5000) on the
symmetric graph of tests/node2vec_ref.py, 4 126 670 slots, more than one stride of 2 048 x 1 024, with 999 copies of the hub.  Against
the half set a second trip that repeats the tile one stride earlier keeps other slots; against the set of eight most tiles keep nothing
and are skipped in both trips."""
import numpy as np
import pytest
import torch

from tests import in_edges_ref
from tests import induced_ref as ref
from tests import node2vec_ref
from tests.compare import same_arrays
from tests.test_gpu_induced import EIGHT, NAMES, half_set

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HUB = 6
BIG_M = 4126670


def slot_case(indptr, col, nodes):
    """(rows, kept mask, K, dst, src_local, eid) of seeds_for(5000) against nodes."""
    rows = node2vec_ref.seeds_for(5000)
    off = in_edges_ref.row_offsets(indptr, rows)
    M = int(off[-1])
    assert M == BIG_M > ref.STRIDE and (rows == HUB).sum() == 999
    kept = ref.slot_mask(indptr, col, rows, off, M, nodes)[0]
    K, dst, local, eid = ref.edges(indptr, col, rows, off, M, nodes)
    stale = ref.stale_second_trip(kept)
    assert (stale != kept).sum() >= 1000 and int(stale.sum()) != K, "a stale second trip keeps other slots, and another number of them"
    assert int(kept[ref.STRIDE:].sum()) >= 1000, "the second trip keeps entries"
    t = ref.tile_counts(kept)
    if nodes.size == EIGHT.size:
        first, second = t[:2048], t[2048:]
        assert (first == 0).sum() > first.size // 2 and (second == 0).sum() > second.size // 2, "most tiles are skipped in both trips"
    return rows, kept, K, dst, local, eid


def test_the_cases_hold_their_conditions_before_any_launch():
    indptr, col, _ = node2vec_ref.sym_graph()
    for nodes in (half_set(), EIGHT):
        slot_case(indptr, col, nodes)


@pytest.mark.parametrize("which", ["half", "eight"])
def test_more_slots_than_one_stride(hip, which):
    from legion_amd import engine
    indptr, col, _ = node2vec_ref.sym_graph()
    nodes = half_set() if which == "half" else EIGHT
    rows, kept, K, dst, local, eid = slot_case(indptr, col, nodes)
    g = engine.GraphStorage(1, torch.from_numpy(indptr).to(DEV), torch.from_numpy(col).to(DEV))
    try:
        ns = engine.NodeSet(nodes, device=DEV)
        got = g.induced_edges(torch.from_numpy(rows).to(DEV), ns, return_eids=True)
        torch.cuda.synchronize()
        same_arrays(got, (dst, local, eid), f"5 000 rows, {which}", names=NAMES)
        got = g.induced_edges(torch.from_numpy(rows).to(DEV), ns)
        torch.cuda.synchronize()
        same_arrays(got, (dst, local), f"5 000 rows, {which}, no edge ids", names=NAMES)
    finally:
        torch.cuda.synchronize()
        g.close()
