"""Seeded random shapes through node2vec_random_walk, bit for bit against tests/node2vec_ref.py: the four kinds of graph of
tests/test_gpu_fuzz.random_case with their rows sorted, every second one symmetrised first (reciprocal edges and triangles: all three
classes of candidate), dead column entries on some, arbitrary float32 weights, random legal p, q and max_tries, random bases up to the
largest legal one, seeds with repeats, a -1 and a node_num.

As in tests/test_gpu_walk_fuzz.py the reference takes the prefix table read back from the GPU (the association of its sums is free under
the contract), and before the kernel runs every index the reference reads is shown inside its array.  A failure names the seed and the
shape."""
import numpy as np
import pytest
import torch

from tests import node2vec_ref as ref
from tests import walk_ref
from tests.test_gpu_fuzz import random_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
M31 = 2 ** 31 - 1
SEEDS = range(24)


def fuzz_shape(seed):
    """Everything of a case that needs no GPU: the graph, the weights and the arguments of its call."""
    c = random_case(seed)
    rng = np.random.RandomState(47000 + seed)
    indptr, col = c["indptr"], c["col"]
    node_num = indptr.size - 1
    rows = np.repeat(np.arange(node_num, dtype=np.int64), np.diff(indptr))
    cols = col.astype(np.int64)
    if (seed // 4) % 2:                                            # symmetrised: every kind of graph both ways
        rows, cols = np.concatenate([rows, cols]), np.concatenate([cols, rows])
    order = np.lexsort((cols, rows))
    rows, col = rows[order], cols[order].astype(np.int32)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=node_num))]).astype(np.int64)
    if seed % 2 and col.size:                                      # dead entries: the first of some rows, so the rows stay sorted
        starts = indptr[:-1][np.diff(indptr) > 0]
        col[starts[rng.rand(starts.size) < 0.05]] = -1
    assert ref.rows_sorted(indptr, col)
    E = col.size
    w = (rng.rand(E) * 10.0 ** rng.randint(-3, 4, E)).astype(np.float32)
    w[rng.rand(E) < 0.1] = 0
    odd = rng.rand(E) < 0.02
    w[odd] = np.array([np.nan, -1.5, np.inf, -np.inf, -0.0], dtype=np.float32)[rng.randint(0, 5, int(odd.sum()))]
    n, length = int(rng.randint(1, 701)), int(rng.randint(1, 41))
    while True:                                                    # legal: finite, > 0, the ratio of the weights at most 16
        p, q = (float(np.float32(2.0 ** rng.uniform(-4, 4))) for _ in range(2))
        if not ref.refused(n, length, p, q, 0, 1, 0, False, 1):
            break
    tries = int(rng.choice([1, 2, 3, 5, 16, 256]))
    s = rng.randint(0, node_num, n).astype(np.int32)
    if n >= 3:
        s[rng.randint(0, n)] = s[0]
        at = rng.choice(n, 2, replace=False)
        s[at[0]], s[at[1]] = -1, node_num
    return dict(seed=seed, indptr=indptr, col=col, w=w, n=n, length=length, p=p, q=q, tries=tries, eids=bool(rng.randint(2)),
                weighted=bool(rng.randint(2)), base=int(rng.randint(0, M31 - n * length + 1)), seeds=s)


@pytest.fixture(scope="module")
def cases(hip):
    """seed -> the case on the device with its reference, built once and shared by the per-seed tests and the test of the seed set."""
    from legion_amd import engine
    made = {}

    def get(seed):
        if seed in made:
            return made[seed]
        c = fuzz_shape(seed)
        g = engine.GraphStorage(1, torch.from_numpy(c["indptr"]).to(DEV), torch.from_numpy(c["col"]).to(DEV))
        made[seed] = c
        c["graph"] = g
        g.set_edge_weights(c["w"])
        torch.cuda.synchronize()
        table = g.edge_cdf().cpu().numpy().copy()
        reads, c["stats"] = {}, ref.new_stats()
        c["want"] = ref.walk(c["indptr"], c["col"], c["seeds"], c["length"], c["p"], c["q"], table=table if c["weighted"] else None,
                             max_tries=c["tries"], base=c["base"], reads=reads, stats=c["stats"])
        walk_ref.assert_reads_in_bounds(reads, c["indptr"].size - 1, c["col"].size)
        return c

    yield get
    torch.cuda.synchronize()
    for c in made.values():
        c["graph"].close()


def _ctx(c):
    shape = {k: v for k, v in c.items() if k in ("n", "length", "p", "q", "tries", "eids", "weighted", "base")}
    return f"seed {c['seed']} (kind {c['seed'] % 4}, N {c['indptr'].size - 1}, E {c['col'].size}): {shape}"


@pytest.mark.parametrize("seed", SEEDS)
def test_random_node2vec_walks_match_the_reference(cases, seed):
    c = cases(seed)
    ctx = _ctx(c)
    got = c["graph"].node2vec_random_walk(c["seeds"], c["p"], c["q"], c["length"], weighted=c["weighted"], return_eids=c["eids"],
                                          max_tries=c["tries"], base=c["base"])
    torch.cuda.synchronize()
    got = [x.cpu().numpy() for x in (got if c["eids"] else (got,))]
    for g, w, what in zip(got, c["want"], ("traces", "edge ids")):
        bad = np.argwhere(g != w) if g.shape == w.shape else None
        assert g.dtype == w.dtype and bad is not None and bad.size == 0, \
            f"{ctx}: {what}: {g.shape} against {w.shape}" if bad is None else \
            f"{ctx}: {len(bad)} {what} differ, first at walk, position {bad[0]}: got {g[tuple(bad[0])]} want {w[tuple(bad[0])]}"
    if c["eids"]:
        walk_ref.check(c["indptr"], c["col"], c["seeds"], got[0], got[1])


def seed_set_conditions(cases_of):
    """What the seed set must hold, from the references alone; a set that fails is replaced (the salt of fuzz_shape), not the condition."""
    acc, rej, forced, searches, eids, weighted = [0, 0, 0], [0, 0, 0], 0, 0, 0, 0
    for seed in SEEDS:
        c = cases_of(seed)
        assert not ref.refused(c["n"], c["length"], c["p"], c["q"], int(c["weighted"]), c["tries"], c["base"], True, 1), seed
        for k in range(3):
            acc[k] += c["stats"]["accepted"][k]
            rej[k] += c["stats"]["rejected"][k]
        forced += c["stats"]["forced"] if c["tries"] > 1 else 0
        searches += c["stats"]["searches"]
        eids += int(c["eids"])
        weighted += int(c["weighted"])
    print("accepted", acc, "rejected", rej, "forced", forced, "searches", searches, "edge ids", eids, "weighted", weighted)
    assert min(acc) >= 100 and min(rej) >= 100 and forced >= 100 and searches >= 100
    assert 0 < eids < len(SEEDS) and 0 < weighted < len(SEEDS)


def test_the_seed_set_holds_its_conditions(cases):
    seed_set_conditions(cases)
