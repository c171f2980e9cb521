"""Seeded random shapes through random_walk and pinsage_neighbors, bit for bit against tests/walk_ref.py and tests/pinsage_ref.py: the
four kinds of graph of tests/test_gpu_fuzz.random_case, dead column entries on odd seeds, arbitrary float32 weights (a tenth zero, a few
NaN, negative or infinite), random bases up to the largest legal one, seeds with repeats, a -1 and a node_num.

The association of the prefix table's sums is free under the contract, so the reference takes the table read back from the GPU, after
its contract properties have been asserted as tests/test_gpu_sample_weighted.test_table_properties_with_arbitrary_floats does: the walk
comparison is then exact and independent of the scan.  Before either kernel runs, every index the reference reads is shown inside its
array.  A failure names the seed and the shape."""
import numpy as np
import pytest
import torch

from tests import functional_ref
from tests import mode_ref
from tests import pinsage_ref
from tests import walk_ref
from tests import weighted_ref
from tests.test_gpu_fuzz import random_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
M31 = 2 ** 31 - 1
SEEDS = range(24)
CLASS_EDGES = {32: (1, 32), 64: (33, 64), 256: (65, 256), 1024: (257, 1024)}


def _seeds(rng, n, node_num):
    """n seeds with repeats; a -1 and a node_num among them where there is room."""
    s = rng.randint(0, node_num, n).astype(np.int32)
    if n >= 3:
        s[rng.randint(0, n)] = s[0]
        at = rng.choice(n, 2, replace=False)
        s[at[0]], s[at[1]] = -1, node_num
    return s


def fuzz_shape(seed):
    """Everything of a case that needs no GPU: the graph, the weights and the arguments of its two calls."""
    c = random_case(seed)
    indptr, col = c["indptr"], c["col"]
    if seed % 2:
        col = mode_ref.with_dead_columns(col, seed)
    rng = np.random.RandomState(31000 + seed)
    E, node_num = col.size, indptr.size - 1
    w = (rng.rand(E) * 10.0 ** rng.randint(-3, 4, E)).astype(np.float32)
    w[rng.rand(E) < 0.1] = 0
    odd = rng.rand(E) < 0.02
    w[odd] = np.array([np.nan, -1.5, np.inf, -np.inf, -0.0], dtype=np.float32)[rng.randint(0, 5, int(odd.sum()))]
    n, length = int(rng.randint(1, 701)), int(rng.randint(1, 41))
    walk = dict(n=n, length=length, eids=bool(rng.randint(2)), restart=float(rng.choice([0.0, 0.1, 0.5])), weighted=bool(rng.randint(2)),
                base=int(rng.randint(0, M31 - n * length + 1)), seeds=_seeds(rng, n, node_num))
    lo, hi = CLASS_EDGES[(32, 64, 256, 1024)[(seed // 4) % 4]]      # the visit class: every class meets every kind of graph
    while True:
        T = int(rng.randint(1, min(hi, 40) + 1))
        R = int(rng.randint(lo, hi + 1)) // T
        if R >= 1 and lo <= R * T <= hi:
            break
    n = int(rng.randint(1, 301))
    k = [int(rng.randint(1, 9)), int(rng.randint(1, min(R * T + 1, 1024) + 1)), int(rng.randint(1, 1025))][int(rng.randint(3))]
    pin = dict(n=n, R=R, T=T, k=k, p=float(rng.choice([0.0, 0.1, 0.5, 0.9])), weighted=bool(rng.randint(2)),
               base=int(rng.randint(0, M31 - n * R * T + 1)), seeds=_seeds(rng, n, node_num))
    return dict(seed=seed, indptr=indptr, col=col, w=w, walk=walk, pin=pin)


def _table_properties(indptr, w, got, ctx):
    """The contract of the table: finite, non-decreasing in a row, unmoved by a sanitised zero, within 2^-23 (relative) of the exact sum."""
    ws = weighted_ref.sanitise(w)
    assert got.dtype == np.float32 and got.shape == ws.shape and np.isfinite(got).all(), ctx
    for v in range(indptr.size - 1):
        s, e = int(indptr[v]), int(indptr[v + 1])
        if e == s:
            continue
        row, x = got[s:e], ws[s:e]
        prev = np.concatenate([[np.float32(0)], row[:-1]])
        assert np.all(row >= prev), f"{ctx}: row {v}: decreasing"
        assert np.all(row[x == 0] == prev[x == 0]), f"{ctx}: row {v}: a zero weight moved the table"
        exact = np.cumsum(x.astype(np.longdouble))
        assert np.all(np.abs(row.astype(np.longdouble) - exact) <= np.longdouble(2.0 ** -23) * exact), f"{ctx}: row {v}: off the exact sum"


@pytest.fixture(scope="module")
def cases(hip):
    """seed -> the case on the device with its references, built once and shared by the per-seed tests and the test of the seed set."""
    from legion_amd import engine
    made = {}

    def get(seed):
        if seed in made:
            return made[seed]
        c = fuzz_shape(seed)
        indptr, col = c["indptr"], c["col"]
        node_num, E = indptr.size - 1, col.size
        g = engine.GraphStorage(1, torch.from_numpy(indptr).to(DEV), torch.from_numpy(col).to(DEV))
        made[seed] = c
        c["graph"] = g
        g.set_edge_weights(c["w"])
        torch.cuda.synchronize()
        table = g.edge_cdf().cpu().numpy().copy()
        _table_properties(indptr, c["w"], table, f"seed {seed}")
        a = c["walk"]
        reads = {}
        a["want"] = walk_ref.walk(indptr, col, a["seeds"], a["length"], table=table if a["weighted"] else None, restart_prob=a["restart"],
                                  base=a["base"], reads=reads)
        b = c["pin"]
        b["vis"] = pinsage_ref.visits(indptr, col, b["seeds"], b["R"], b["T"], table=table if b["weighted"] else None,
                                      termination_prob=b["p"], base=b["base"], reads=reads)
        walk_ref.assert_reads_in_bounds(reads, node_num, E)
        b["want"] = pinsage_ref.topk(b["vis"], b["k"])
        return c

    yield get
    torch.cuda.synchronize()
    for c in made.values():
        c["graph"].close()


def _ctx(c, which):
    a = c[which]
    shape = {k: v for k, v in a.items() if k not in ("seeds", "want", "vis")}
    return f"seed {c['seed']} (kind {c['seed'] % 4}, N {c['indptr'].size - 1}, E {c['col'].size}): {which} {shape}"


@pytest.mark.parametrize("seed", SEEDS)
def test_random_walks_match_the_reference(cases, seed):
    c = cases(seed)
    a, ctx = c["walk"], _ctx(c, "walk")
    got = c["graph"].random_walk(a["seeds"], a["length"], weighted=a["weighted"], restart_prob=a["restart"], return_eids=a["eids"],
                                 base=a["base"])
    torch.cuda.synchronize()
    got = [x.cpu().numpy() for x in (got if a["eids"] else (got,))]
    for g, w, what in zip(got, a["want"], ("traces", "edge ids")):
        bad = np.argwhere(g != w) if g.shape == w.shape else None
        assert g.dtype == w.dtype and bad is not None and bad.size == 0, \
            f"{ctx}: {what}: {g.shape} against {w.shape}" if bad is None else \
            f"{ctx}: {len(bad)} {what} differ, first at walk, position {bad[0]}: got {g[tuple(bad[0])]} want {w[tuple(bad[0])]}"
    if a["eids"]:
        walk_ref.check(c["indptr"], c["col"], a["seeds"], got[0], got[1])


@pytest.mark.parametrize("seed", SEEDS)
def test_random_neighbourhoods_match_the_reference(cases, seed):
    c = cases(seed)
    b, ctx = c["pin"], _ctx(c, "pin")
    got = c["graph"].pinsage_neighbors(b["seeds"], b["R"], b["T"], b["k"], termination_prob=b["p"], weighted=b["weighted"], base=b["base"])
    torch.cuda.synchronize()
    nb, ct = (x.cpu().numpy() for x in got)
    assert nb.dtype == ct.dtype == np.int32 and nb.shape == b["want"][0].shape and ct.shape == b["want"][1].shape, ctx
    bad = np.argwhere((nb != b["want"][0]) | (ct != b["want"][1]))
    assert bad.size == 0, f"{ctx}: {len(bad)} slots differ, first at seed, slot {bad[0]}: got {nb[tuple(bad[0])]} x {ct[tuple(bad[0])]} " \
                          f"want {b['want'][0][tuple(bad[0])]} x {b['want'][1][tuple(bad[0])]}"


def seed_set_conditions(cases_of):
    """What the seed set must hold, from the references alone; a set that fails is replaced (the salt of fuzz_shape), not the condition."""
    per_class = {v: [] for v in CLASS_EDGES}
    tie = short = empty = eids = restart = 0
    for seed in SEEDS:
        c = cases_of(seed)
        a, b = c["walk"], c["pin"]
        assert not walk_ref.refused(a["n"], a["length"], int(a["weighted"]), a["restart"], a["base"], True), seed
        assert not pinsage_ref.refused(b["n"], b["R"], b["T"], b["k"], int(b["weighted"]), b["p"], b["base"], True), seed
        per_class[functional_ref.vpad(b["R"] * b["T"])].append(b["weighted"])
        full, counts = pinsage_ref.topk(b["vis"], 1024)
        distinct = (full >= 0).sum(axis=1)
        k = b["k"]
        tie += int(any(d > k and counts[i, k - 1] == counts[i, k] for i, d in enumerate(distinct) if k < 1024))
        short += int(((distinct > 0) & (distinct < k)).any())
        empty += int((distinct == 0).any())
        eids += int(a["eids"])
        restart += int(a["restart"] > 0)
    print("classes:", {v: len(m) for v, m in per_class.items()}, "cut decided by the id:", tie, "fewer than k:", short, "an empty row:", empty,
          "edge ids:", eids, "restart:", restart)
    for v, modes in per_class.items():
        assert len(modes) >= 4 and True in modes and False in modes, (v, modes)
    assert tie >= 4 and short >= 4 and empty >= 4 and 0 < eids < len(SEEDS) and 0 < restart < len(SEEDS)


def test_the_seed_set_holds_its_conditions(cases):
    seed_set_conditions(cases)
