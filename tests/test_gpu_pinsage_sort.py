"""The sort, count and top-k steps of pinsage_neighbors_kernel over segments whose content is chosen, not drawn: on graphs whose rows
have at most one entry (tests/functional_ref.py) a walk is the iterated successor whatever is drawn, so a path over a chosen id order
fills a seed's visit segment in that order.  The expectation takes no draw and no reference walk: iterate the successor, np.unique,
order by (count descending, id ascending).  tests/test_walk_ref_cpu.py holds it against the references on these graphs and checks
that every index the references read there lies inside its array.  random_walk runs on the same graphs."""
import numpy as np
import pytest
import torch

from tests import functional_ref as fn

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


class Graph:
    """A functional graph on the device with its weights set, and the successor each pick mode sees."""

    def __init__(self, succ, zero_weight=()):
        from legion_amd import engine
        indptr, col, w = fn.graph_of(succ, zero_weight)
        assert int(np.diff(indptr).max()) <= 1 and col.size > 0 and int(col.max()) < succ.size and int(col.min()) >= 0
        self.indptr = indptr
        self.g = engine.GraphStorage(1, torch.from_numpy(indptr).to(DEV), torch.from_numpy(col).to(DEV))
        self.g.set_edge_weights(w)
        self.succ = {False: succ, True: fn.without(succ, zero_weight)}

    def same_neighbors(self, seeds, R, T, k, ctx, base=0, p=0.0):
        for weighted in (False, True):
            want = fn.expected_neighbors(self.succ[weighted], seeds, R, T, k)
            got = self.g.pinsage_neighbors(seeds, R, T, k, termination_prob=p, weighted=weighted, base=base)
            torch.cuda.synchronize()
            nb, ct = (x.cpu().numpy() for x in got)
            assert nb.dtype == ct.dtype == np.int32 and nb.shape == want[0].shape and ct.shape == want[1].shape, ctx
            bad = np.argwhere((nb != want[0]) | (ct != want[1]))
            assert bad.size == 0, f"{ctx}, (R, T, k) = {(R, T, k)}, {'weighted' if weighted else 'uniform'}: {len(bad)} slots differ, " \
                                  f"first at seed {bad[0][0]} (vertex {seeds[bad[0][0]]}), slot {bad[0][1]}: got " \
                                  f"{nb[tuple(bad[0])]} x {ct[tuple(bad[0])]} want {want[0][tuple(bad[0])]} x {want[1][tuple(bad[0])]}"

    def same_walks(self, seeds, length, ctx, base=0):
        for weighted in (False, True):
            want = fn.expected_walk(self.succ[weighted], self.indptr, seeds, length)
            got = self.g.random_walk(seeds, length, weighted=weighted, return_eids=True, base=base)
            only = self.g.random_walk(seeds, length, weighted=weighted, base=base)
            torch.cuda.synchronize()
            traces, eids = (x.cpu().numpy() for x in got)
            assert traces.dtype == np.int32 and eids.dtype == np.int64
            for a, b, what in ((traces, want[0], "traces"), (eids, want[1], "edge ids"), (only.cpu().numpy(), want[0], "traces alone")):
                bad = np.argwhere(a != b)
                assert a.shape == b.shape and bad.size == 0, f"{ctx}, length {length}, {'weighted' if weighted else 'uniform'}: {len(bad)} " \
                    f"{what} differ, first at walk, position {bad[0]}: got {a[tuple(bad[0])]} want {b[tuple(bad[0])]}"

    def close(self):
        torch.cuda.synchronize()
        self.g.close()


@pytest.mark.parametrize("T", fn.PATH_T)
@pytest.mark.parametrize("order", fn.ORDERS)
def test_paths_over_a_chosen_id_order(hip, order, T):
    """R = 1: a segment holds T distinct ids in the path's order (T = VPAD: no sentinel), less near the path's end; k around T."""
    succ, seeds = fn.path_case(order, 1, T)
    g = Graph(succ)
    try:
        for k in fn.ks_for(T):
            g.same_neighbors(seeds, 1, T, k, f"{order} path, {seeds.size} seeds", base=7)
    finally:
        g.close()


@pytest.mark.parametrize("shape", fn.RUN_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("order", fn.ORDERS)
def test_runs_of_length_r(hip, order, shape):
    """R identical walks: every visited vertex is a run of R in the sorted segment; (1024, 1) is one run of the whole segment."""
    R, T = shape
    succ, seeds = fn.path_case(order, R, T)
    g = Graph(succ)
    try:
        for k in fn.ks_for(T):
            g.same_neighbors(seeds, R, T, k, f"{order} path, {seeds.size} seeds")
    finally:
        g.close()


def test_unequal_counts_and_ties_without_a_draw(hip):
    """A self-loop (one run of R * T at each class size), a cycle of three under 1 024 steps (342 / 341 / 341, the larger count at
    the largest id), a tail into a cycle, and a path edge of weight 0 where a weighted walk ends and an unweighted one goes on."""
    g = Graph(fn.misc_succ(), fn.MISC_ZERO)
    try:
        for R, T, k in fn.MISC_SHAPES:
            g.same_neighbors(fn.MISC_SEEDS, R, T, k, "the small graph", base=3)
            g.same_neighbors(fn.MISC_SEEDS, R, T, k, "the small graph at the largest base", base=2 ** 31 - 1 - fn.MISC_SEEDS.size * R * T)
        g.same_walks(fn.MISC_SEEDS, 17, "the small graph", base=11)
    finally:
        g.close()


@pytest.mark.parametrize("shape", [(1, 1), (4, 8)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_wide_write_out(hip, shape):
    """k = 1024 over the 32-slot class and a full tile and one seed: live * K reaches 64 * 1024, and every slot from VPAD on is -1 / 0."""
    R, T = shape
    ids = fn.id_order("shuffled", 100)
    g = Graph(fn.path_succ(ids))
    try:
        g.same_neighbors(ids[:65].astype(np.int32), R, T, 1024, "65 seeds on a shuffled path of 100")
        g.same_neighbors(ids[-64:].astype(np.int32), R, T, 1024, "the last 64 of a shuffled path of 100")
    finally:
        g.close()


@pytest.mark.parametrize("order", fn.ORDERS)
def test_walks_are_the_iterated_successor(hip, order):
    """257 walks of 16, 17 and 1 024 steps on a path of 1 100 vertices: some run their length, some off the path's end."""
    ids = fn.id_order(order, 1100)
    seeds = np.concatenate([ids[np.arange(256) * 4], [-1]]).astype(np.int32)
    g = Graph(fn.path_succ(ids))
    try:
        for length in (16, 17, 1024):
            g.same_walks(seeds, length, f"{order} path of 1100", base=11)
    finally:
        g.close()
