"""Seeded random shapes through the link seed ops, bit for bit against tests/link_ref.py: the sorted-row graphs of
tests/test_gpu_node2vec_fuzz.fuzz_shape (the four kinds of tests/test_gpu_fuzz.random_case, symmetrised on some seeds, dead first
entries on the odd ones) with 1 to 3 000 seed edges drawn with repeats from [-2, E + 2], k from {1, 2, 5, 17, 64}, every exclusion,
max_tries from {1, 2, 3, 16, 256} and a base up to the largest legal one.  Per seed: find_edges, negative_sample on its rows, unique_ids
on the concatenation, and edge_prediction_seeds in one call.

Before the kernels run every index the reference reads is shown inside its array, and one test over the seed set asserts from the
references that the 24 cases hold what they are there for.  A failure names the seed and the shape."""
import numpy as np
import pytest
import torch

from tests import link_ref as ref
from tests import walk_ref
from tests.compare import same_arrays
from tests.test_gpu_node2vec_fuzz import fuzz_shape

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
M31 = 2 ** 31 - 1
SEEDS = range(24)
KS = [1, 2, 5, 17, 64]
TRIES = [1, 2, 3, 16, 256]


def link_shape(seed):
    """Everything of a case that needs no GPU: the graph, the arguments, the references and their counters."""
    c = fuzz_shape(seed)
    indptr, col = c["indptr"], c["col"]
    rng = np.random.RandomState(53000 + seed)
    B = int(rng.randint(1, 3001))
    k = int(rng.choice(KS))
    exclude = int(rng.randint(0, 4))
    tries = int(rng.choice(TRIES))
    base = int(rng.randint(0, M31 - B * k + 1))
    E, node_num = col.size, indptr.size - 1
    eids = rng.randint(-2, E + 3, B).astype(np.int64)
    assert not ref.negative_refused(B, k, exclude, tries, base, 1) and B * (2 + k) <= ref.MAX_IDS
    reads, stats = {}, ref.new_stats(node_num)
    row, cc = ref.find_edges(indptr, col, eids, reads=reads)
    neg = ref.negative_sample(indptr, col, row, k, exclude, tries, base, reads=reads, stats=stats)
    walk_ref.assert_reads_in_bounds(reads, node_num, E)
    want = ref.edge_prediction_seeds(indptr, col, eids, k, exclude, tries, base)
    assert np.array_equal(want["row"], row) and np.array_equal(want["col"], cc) and np.array_equal(want["neg"], neg)
    inside = (eids >= 0) & (eids < E)
    return dict(seed=seed, indptr=indptr, col=col, B=B, k=k, exclude=exclude, tries=tries, base=base, eids=eids, want=want, stats=stats,
                dead_rows=int((row[inside] < 0).sum()))


def seed_set_conditions(shape_of):
    """What the seed set must hold, from the references alone."""
    cs = [shape_of(seed) for seed in SEEDS]
    assert all(c["col"].size > 0 for c in cs), "a graph without edges"
    exhausted = sum(c["stats"]["exhausted"] for c in cs)
    hits = sum(c["stats"]["hit"] for c in cs)
    dead = sum(c["dead_rows"] for c in cs)
    largest = max(c["B"] * (2 + c["k"]) for c in cs)
    print("exhausted", exhausted, "search hits", hits, "rows -1 by a dead entry", dead, "largest concatenation", largest)
    assert {c["exclude"] for c in cs} == {0, 1, 2, 3} and {c["tries"] for c in cs} == set(TRIES)
    assert exhausted >= 1 and hits >= 1 and dead >= 1 and largest > 65536


@pytest.fixture(scope="module")
def cases(hip):
    """seed -> the case on the device with its reference, built once and shared by the per-seed tests and the test of the seed set."""
    from legion_amd import engine
    made = {}

    def get(seed):
        if seed not in made:
            c = link_shape(seed)
            c["graph"] = engine.GraphStorage(1, torch.from_numpy(c["indptr"]).to(DEV), torch.from_numpy(c["col"]).to(DEV))
            made[seed] = c
        return made[seed]

    yield get
    torch.cuda.synchronize()
    for c in made.values():
        c["graph"].close()


@pytest.mark.parametrize("seed", SEEDS)
def test_random_link_seeds_match_the_reference(cases, seed):
    from legion_amd import engine
    c = cases(seed)
    g, want, k = c["graph"], c["want"], c["k"]
    kw = dict(exclude_self=bool(c["exclude"] & 1), exclude_edges=bool(c["exclude"] & 2), max_tries=c["tries"], base=c["base"])
    ctx = f"seed {seed} (kind {seed % 4}, N {c['indptr'].size - 1}, E {c['col'].size}): B {c['B']} k {k} {kw}: "
    row, col = g.find_edges(c["eids"])
    neg = g.negative_sample(row, k, **kw)
    unique, local, count = engine.unique_ids(torch.cat([row, col, neg.reshape(-1)]))
    seeds, num, pos_row, pos_col, neg_col = g.edge_prediction_seeds(c["eids"], k, **kw)
    torch.cuda.synchronize()
    B = c["B"]
    same_arrays(row, want["row"], ctx + "row")
    same_arrays(col, want["col"], ctx + "col")
    same_arrays(neg, want["neg"], ctx + "neg")
    same_arrays(unique, want["seeds"], ctx + "unique")
    same_arrays(local, np.concatenate([want["pos_row"], want["pos_col"], want["neg_col"].reshape(-1)]), ctx + "local")
    same_arrays(seeds, want["seeds"], ctx + "seeds")
    same_arrays(pos_row, want["pos_row"], ctx + "pos_row")
    same_arrays(pos_col, want["pos_col"], ctx + "pos_col")
    same_arrays(neg_col, want["neg_col"], ctx + "neg_col")
    assert int(count.item()) == int(num.item()) == want["num_seeds"], ctx + "count"
    assert seeds.shape == (B * (2 + k),) and neg_col.shape == (B, k)


def test_the_seed_set_holds_its_conditions(cases):
    seed_set_conditions(cases)
