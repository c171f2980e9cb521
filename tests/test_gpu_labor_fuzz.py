"""Seeded random shapes through layer-neighbour sampling, bit for bit against tests/labor_ref.py: the sorted-row graphs of
tests/test_gpu_node2vec_fuzz.fuzz_shape (the four kinds of tests/test_gpu_fuzz.random_case, symmetrised on some seeds, dead first entries
on the odd ones) with 1 to 3 000 rows drawn with repeats from [-2, N + 2]; fan-out in [1, 40], salt, m (the rows' M, or a prefix of it)
and cap come from RandomState(62000 + seed).  Per seed: labor_edges sized exactly, the C ABI's pair with m and cap, and labor_block over
distinct seeds.

Before the kernels run every index the reference reads is shown inside its array, and one test over the seed set asserts from the
references that the 24 cases hold what they are there for.  A failure names the seed and the shape."""
import numpy as np
import pytest
import torch

from tests import in_edges_ref
from tests import labor_ref as ref
from tests import link_ref, walk_ref
from tests.compare import same_arrays
from tests.test_gpu_labor import abi
from tests.test_gpu_node2vec_fuzz import fuzz_shape

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEEDS = range(24)


def labor_shape(seed):
    """Everything of a case that needs no GPU: the graph, the arguments and the references."""
    c = fuzz_shape(seed)
    indptr, col = c["indptr"], c["col"]
    node_num, E = indptr.size - 1, col.size
    rng = np.random.RandomState(62000 + seed)
    n = int(rng.randint(1, 3001))
    rows = rng.randint(-2, node_num + 2, n).astype(np.int32)
    if seed % 3 == 0:                                              # a run of rows without entries in the middle
        rows[n // 3:n // 3 + n // 4] = -1
    fanout = int(rng.randint(1, 41))
    salt = int(rng.randint(-2 ** 31, 2 ** 31)) * (2 ** 32 if seed % 2 else 1) + seed
    eids = bool(rng.randint(2))
    if seed % 8 == 5:                                              # a case that keeps nothing: rows without entries only
        rows = np.where(np.diff(indptr)[np.clip(rows, 0, node_num - 1)] == 0, rows, -1).astype(np.int32)
    reads = {}
    offsets = in_edges_ref.row_offsets(indptr, rows, reads=reads)
    M = int(offsets[-1])
    m = M if seed % 4 else max(M - int(rng.randint(1, 1500)), 0)   # every fourth: a prefix
    K, dst, src, eid = ref.edges(indptr, col, rows, offsets, m, fanout, salt, reads=reads)
    walk_ref.assert_reads_in_bounds(reads, node_num, E)
    full = ref.edges_full(indptr, col, rows, fanout, salt)
    caps = sorted({max(K - int(rng.randint(1, 300)), 0), K, K + int(rng.randint(1, 1500))})
    assert not ref.refused("edges", n, m, fanout, cap=caps[-1])
    k = int(rng.randint(1, min(node_num, 400) + 1))
    seeds = rng.choice(node_num, k, replace=False).astype(np.int32)
    block = ref.block(indptr, col, seeds, fanout, salt)
    assert k + block["dst"].size <= link_ref.MAX_IDS
    deg = in_edges_ref.degrees(indptr, rows)
    inside = (rows >= 0) & (rows < node_num)
    entries = in_edges_ref.in_edges(indptr, col, rows, offsets, m)[1]
    return dict(seed=seed, indptr=indptr, col=col, n=n, rows=rows, fanout=fanout, salt=salt, eids=eids, offsets=offsets, M=M, m=m, K=K,
                want=(dst, src, eid), full=full, caps=caps, seeds=seeds, block=block, empty=int(((deg == 0) & inside).sum()),
                outside=int((~inside).sum()), dead=int((entries < 0).sum()) if m else 0, thinned=int(m - (entries < 0).sum() - K) if m else 0)


def seed_set_conditions(shape_of):
    """What the seed set must hold, from the references alone."""
    cs = [shape_of(seed) for seed in SEEDS]
    figures = {key: sum(c[key] for c in cs) for key in ("empty", "outside", "dead", "thinned")}
    print(figures, "K", [c["K"] for c in cs], "fanouts", [c["fanout"] for c in cs], "caps", [c["caps"] for c in cs][:4])
    assert all(v >= 24 for v in figures.values()), figures
    assert {c["eids"] for c in cs} == {False, True} and max(c["m"] for c in cs) > 4 * ref.TILE
    assert any(c["K"] == 0 for c in cs), "some case keeps nothing"
    assert any(c["caps"][0] < c["K"] for c in cs) and all(c["caps"][-1] > c["K"] for c in cs), "some case has cap < K"
    assert any(0 < c["m"] < c["M"] for c in cs) and min(c["fanout"] for c in cs) <= 5 and max(c["fanout"] for c in cs) >= 35
    assert any(c["salt"] < 0 for c in cs) and any(c["salt"] > 2 ** 32 for c in cs)
    assert any(0 < c["K"] < c["m"] for c in cs) and sum(c["thinned"] > 0 for c in cs) >= 12, "the predicate thins most cases"


@pytest.fixture(scope="module")
def cases(hip):
    """seed -> the case on the device with its reference, built once and shared by the per-seed tests and the test of the seed set."""
    from legion_amd import engine
    made = {}

    def get(seed):
        if seed not in made:
            c = labor_shape(seed)
            c["graph"] = engine.GraphStorage(1, torch.from_numpy(c["indptr"]).to(DEV), torch.from_numpy(c["col"]).to(DEV))
            made[seed] = c
        return made[seed]

    yield get
    torch.cuda.synchronize()
    for c in made.values():
        c["graph"].close()


@pytest.mark.parametrize("seed", SEEDS)
def test_random_rows_match_the_reference(cases, hip, seed):
    c = cases(seed)
    g = c["graph"]
    ctx = (f"seed {seed} (kind {seed % 4}, N {c['indptr'].size - 1}, E {c['col'].size}): n {c['n']} M {c['M']} m {c['m']} fanout {c['fanout']} "
           f"salt {c['salt']} K {c['K']} eids {c['eids']}: ")
    got = g.labor_edges(c["rows"], c["fanout"], salt=c["salt"], return_eids=c["eids"])
    torch.cuda.synchronize()
    for name, x, w in zip(("dst", "src", "eid"), got, c["full"]):
        same_arrays(x, w, ctx + name)
    for cap in c["caps"]:
        want = ref.edges(c["indptr"], c["col"], c["rows"], c["offsets"], c["m"], c["fanout"], c["salt"], cap=cap)
        k, *out = abi(hip, g, c["rows"], c["offsets"], c["m"], c["fanout"], c["salt"], cap, c["eids"])
        assert k == c["K"] == want[0], ctx + f"count {k}"
        for name, x, w in zip(("dst", "src", "eid"), out, want[1:]):
            if x is not None:
                same_arrays(x, w, ctx + f"cap {cap} {name}")
    b = c["block"]
    blk = g.labor_block(c["seeds"], c["fanout"], salt=c["salt"], return_eids=True)
    torch.cuda.synchronize()
    for name, x in zip(("input_nodes", "dst_local", "src_local", "eids"), blk):
        same_arrays(x, b[name], ctx + "block " + name)


def test_the_seed_set_holds_its_conditions(cases):
    seed_set_conditions(cases)
