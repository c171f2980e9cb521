"""Seeded random shapes through the per-row selection, bit for bit against tests/topk_ref.py: small random graphs of 5 to 400 rows with
one to three hubs (up to 9 000 entries, so both kernel classes occur), 5 % dead entries, weights in eighths mixed with NaN, +-inf, -0,
denormals and FLT_MAX; 1 to 3 000 rows drawn with repeats from [-2, N + 2]; k in [1, 64], the mode, the salt and whether the weights,
eid_out and count_out are given come from RandomState(83000 + seed).  Per seed: the C ABI's call, and the Python op of that mode.  One
test over the seed set asserts from the references that the 20 cases hold what they are there for.  A failure names the seed and the
shape."""
import numpy as np
import pytest
import torch

from tests import topk_ref as ref
from tests.compare import same_arrays
from tests.test_gpu_topk import SPECIALS, abi, compare

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEEDS = range(20)


def topk_shape(seed):
    """Everything of a case that needs no GPU: the graph, the arguments and the reference."""
    rng = np.random.RandomState(83000 + seed)
    N = int(rng.randint(5, 401))
    deg = rng.randint(0, 40, N).astype(np.int64)
    deg[rng.rand(N) < 0.1] = 0
    hubs = rng.choice(N, int(rng.randint(1, 4)), replace=False)
    deg[hubs] = rng.choice([63, 64, 65, 130, 1000, 4096, 4097, 9000], hubs.size)
    if seed % 5 == 0:
        deg[hubs[0]] = 4097 + int(rng.randint(0, 5000))
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    E = int(indptr[-1])
    col = rng.randint(0, N, E).astype(np.int32)
    col[rng.rand(E) < 0.05] = -1
    w = (rng.randint(-4, 33, E) / 8).astype(np.float32)
    odd = rng.rand(E) < 0.05
    w[odd] = SPECIALS[rng.randint(0, SPECIALS.size, int(odd.sum()))]
    n = int(rng.randint(1, 3001))
    rows = rng.randint(-2, N + 2, n).astype(np.int32)
    rows[rng.randint(0, n)] = hubs[0]
    k = int(rng.choice([1, 2, 3, 10, 25, 40, 63, 64])) if seed % 2 else int(rng.randint(1, 65))
    mode = seed % 3
    salt = int(rng.randint(-2 ** 31, 2 ** 31)) * (2 ** 32 if seed % 2 else 1) + seed
    has_w = mode != ref.SAMPLE or bool(seed % 4)
    want = ref.row_topk(indptr, col, w if has_w else None, rows, k, mode, salt)
    return dict(seed=seed, indptr=indptr, col=col, w=w, rows=rows, n=n, k=k, mode=mode, salt=salt, has_w=has_w, eids=bool(rng.randint(2)),
                count=bool(rng.randint(2)), want=want, long=int((deg[np.clip(rows, 0, N - 1)] > ref.LONG).sum()),
                short=int((want[2] < k).sum()), full=int((want[2] == k).sum()), outside=int(((rows < 0) | (rows >= N)).sum()))


@pytest.fixture(scope="module")
def cases(hip):
    """seed -> the case, built once and shared by the per-seed tests and the test of the seed set."""
    made = {}

    def get(seed):
        if seed not in made:
            made[seed] = topk_shape(seed)
        return made[seed]

    return get


def test_the_seed_set_holds_its_conditions(cases):
    cs = [cases(seed) for seed in SEEDS]
    figures = {key: sum(c[key] for c in cs) for key in ("long", "short", "full", "outside")}
    print(figures, "k", [c["k"] for c in cs], "modes", [c["mode"] for c in cs])
    assert all(v >= 20 for v in figures.values()), figures
    assert {c["mode"] for c in cs} == set(ref.MODES) and {c["eids"] for c in cs} == {False, True} == {c["count"] for c in cs}
    assert min(c["k"] for c in cs) <= 3 and max(c["k"] for c in cs) >= 60
    assert any(c["salt"] < 0 for c in cs) and any(c["salt"] > 2 ** 32 for c in cs)
    assert any(not c["has_w"] for c in cs) and sum(c["long"] > 0 for c in cs) >= 5


@pytest.mark.parametrize("seed", SEEDS)
def test_random_rows_match_the_reference(cases, hip, seed):
    from legion_amd import engine
    c = cases(seed)
    ctx = (f"seed {seed} (N {c['indptr'].size - 1}, E {c['col'].size}): n {c['n']} k {c['k']} mode {c['mode']} salt {c['salt']} weights {c['has_w']} "
           f"eids {c['eids']} count {c['count']}")
    g = engine.GraphStorage(1, torch.from_numpy(c["indptr"]).to(DEV), torch.from_numpy(c["col"]).to(DEV))
    try:
        d_w = torch.from_numpy(c["w"]).to(DEV) if c["has_w"] else None
        compare(abi(hip, g, c["rows"], c["k"], c["mode"], d_w, c["salt"], c["eids"], c["count"]), c["want"], ctx)
        if c["mode"] == ref.SAMPLE:
            got = g.sample_distinct(c["rows"], c["k"], weights=d_w, salt=c["salt"], return_eids=True)
        else:
            got = g.select_topk(c["rows"], c["k"], d_w, ascending=c["mode"] == ref.SMALLEST, return_eids=True)
            if c["salt"] != 0:                                     # the salt plays no part outside SAMPLE
                assert all(np.array_equal(a, b) for a, b in zip(c["want"], ref.row_topk(c["indptr"], c["col"], c["w"], c["rows"], c["k"], c["mode"], 0)))
        torch.cuda.synchronize()
        same_arrays((got[0], got[2], got[1]), c["want"], ctx + " (python)", names=("src", "eid", "count"))
    finally:
        torch.cuda.synchronize()
        g.close()
