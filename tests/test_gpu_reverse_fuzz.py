"""reverse, out_degrees and out_edges over 24 small random graphs from RandomState(62000 + seed), bit for bit against
tests/reverse_ref.py.  A seed draws the number of vertices, the reverse rows' lengths from a mix that reaches every class of the sort,
the dead and out-of-graph entries and the nodes asked for.  Over the set every sort class, a merge, dead entries, entries outside the
graph and parallel edges occur (asserted from the reference before any launch)."""
import numpy as np
import pytest
import torch

from tests import reverse_ref as ref
from tests.compare import same_arrays

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEEDS = list(range(24))


def reverse_shape(seed):
    """dict of indptr, col, nodes and the reference."""
    rng = np.random.RandomState(62000 + seed)
    N = int(rng.choice([1, 2, 3, 17, 64, 65, 300, 1000]))
    lengths = rng.randint(0, 6, N)
    kind = seed % 4
    if kind >= 1:                                                  # some rows of a wave's class at its edges
        lengths[rng.randint(0, N, 3)] = rng.choice([2, 63, 64], 3)
    if kind >= 2:                                                  # some of a workgroup's
        lengths[rng.randint(0, N, 2)] = rng.choice([65, 700, ref.TILE], 2)
    if kind == 3:                                                  # a long one: 2 to 4 runs
        lengths[rng.randint(0, N)] = int(rng.choice([ref.TILE + 1, 2 * ref.TILE + 9, 3 * ref.TILE + 1]))
    dead, outside = int(rng.randint(0, 30)), int(rng.randint(0, 10))
    if seed % 6 == 5:
        dead = outside = 0
    indptr, col = ref.class_graph(lengths, 62000 + seed, dead=dead, outside=outside)
    n = int(rng.choice([0, 1, 7, 300]))
    nodes = rng.randint(-1, N + 1, n).astype(np.int32)
    return dict(indptr=indptr, col=col, nodes=nodes, want=ref.reverse(indptr, col), lengths=lengths)


def seed_set_conditions(shape_of):
    classes, run_counts, dead, outside, parallel, empty_nodes = set(), set(), 0, 0, 0, 0
    for seed in SEEDS:
        s = shape_of(seed)
        rindptr, rcol, reid = s["want"]
        assert np.array_equal(np.diff(rindptr), s["lengths"])
        c, r = ref.classes_of(rindptr)
        classes |= c
        run_counts |= set(r)
        N = s["indptr"].size - 1
        dead += int((s["col"] == -1).sum() > 0)
        outside += int((s["col"] >= N).sum() > 0)
        pairs = rcol.astype(np.int64) * (N + 1) + np.repeat(np.arange(N), np.diff(rindptr))
        parallel += int(np.unique(pairs).size < pairs.size)
        empty_nodes += int(s["nodes"].size == 0)
    assert classes == {"none", "wave", "tile", "long"} and len(run_counts) >= 2, (classes, run_counts)
    assert dead >= 5 and outside >= 5 and parallel >= 5 and empty_nodes >= 1 and dead < len(SEEDS), (dead, outside, parallel, empty_nodes)


@pytest.fixture(scope="module")
def shapes():
    made = {seed: reverse_shape(seed) for seed in SEEDS}
    seed_set_conditions(lambda seed: made[seed])
    return made


@pytest.mark.parametrize("seed", SEEDS)
def test_reverse_fuzz(hip, shapes, seed):
    from legion_amd import engine
    s = shapes[seed]
    col = torch.from_numpy(s["col"]).to(DEV) if s["col"].size else torch.zeros(0, dtype=torch.int32, device=DEV)
    g = engine.GraphStorage(1, torch.from_numpy(s["indptr"]).to(DEV), col)
    rev = g.reverse()
    same_arrays([rev.indptr, rev.col, rev.eids], s["want"], f"seed {seed}", ("rindptr", "rcol", "reid"))
    assert rev.rows_sorted() is True
    same_arrays(g.out_degrees(s["nodes"]), ref.out_degrees(s["indptr"], s["col"], s["nodes"]), f"seed {seed} out_degrees")
    same_arrays(g.out_edges(s["nodes"], return_eids=True), ref.out_edges(s["indptr"], s["col"], s["nodes"]), f"seed {seed}", ("src", "dst", "eid"))
    torch.cuda.synchronize()
    g.close()
