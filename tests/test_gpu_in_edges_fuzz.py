"""Seeded random shapes through the full-neighbour ops, bit for bit against tests/in_edges_ref.py: the sorted-row graphs of
tests/test_gpu_node2vec_fuzz.fuzz_shape (the four kinds of tests/test_gpu_fuzz.random_case, symmetrised on some seeds, dead first entries
on the odd ones) with 1 to 3 000 rows drawn with repeats from [-2, N + 2], with and without edge ids.  Per seed: row_offsets, in_edges
sized exactly, legion_in_edges with a capacity below, at and above M, and full_neighbor_block over distinct seeds.

Before the kernels run every index the reference reads is shown inside its array, and one test over the seed set asserts from the
references that the 24 cases hold what they are there for.  A failure names the seed and the shape."""
import numpy as np
import pytest
import torch

from tests import in_edges_ref as ref
from tests import link_ref, walk_ref
from tests.compare import same_arrays
from tests.test_gpu_in_edges import abi
from tests.test_gpu_node2vec_fuzz import fuzz_shape

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEEDS = range(24)


def in_edges_shape(seed):
    """Everything of a case that needs no GPU: the graph, the arguments and the references."""
    c = fuzz_shape(seed)
    indptr, col = c["indptr"], c["col"]
    node_num, E = indptr.size - 1, col.size
    rng = np.random.RandomState(61000 + seed)
    n = int(rng.randint(1, 3001))
    rows = rng.randint(-2, node_num + 2, n).astype(np.int32)
    if seed % 3 == 0:                                              # a run of rows without entries in the middle
        rows[n // 3:n // 3 + n // 4] = -1
    eids = bool(rng.randint(2))
    reads = {}
    offsets = ref.row_offsets(indptr, rows, reads=reads)
    M = int(offsets[-1])
    want = ref.in_edges(indptr, col, rows, offsets, M, reads=reads)
    walk_ref.assert_reads_in_bounds(reads, node_num, E)
    assert not ref.refused("in_edges", n, m=M + 1500)
    caps = sorted({max(M - int(rng.randint(1, 1500)), 0), M, M + int(rng.randint(1, 1500))})
    assert np.array_equal(np.unique(want[0]), np.nonzero(np.diff(offsets) > 0)[0]), "no row with entries is skipped"
    k = int(rng.randint(1, min(node_num, 400) + 1))
    seeds = rng.choice(node_num, k, replace=False).astype(np.int32)
    block = ref.full_neighbor_block(indptr, col, seeds)
    assert k + block["dst"].size <= link_ref.MAX_IDS
    deg = ref.degrees(indptr, rows)
    inside = (rows >= 0) & (rows < node_num)
    return dict(seed=seed, indptr=indptr, col=col, n=n, rows=rows, eids=eids, offsets=offsets, M=M, want=want, caps=caps, seeds=seeds,
                block=block, empty=int(((deg == 0) & inside).sum()), outside=int((~inside).sum()), dead=int((want[1] < 0).sum()),
                repeats=n - int(np.unique(rows).size), widest=int(ref.tile_ranges(offsets, M).max()) if M else 0)


def seed_set_conditions(shape_of):
    """What the seed set must hold, from the references alone."""
    cs = [shape_of(seed) for seed in SEEDS]
    figures = {key: sum(c[key] for c in cs) for key in ("empty", "outside", "dead", "repeats")}
    largest, widest = max(c["M"] for c in cs), max(c["widest"] for c in cs)
    print(figures, "largest M", largest, "widest tile range", widest, "caps", [c["caps"] for c in cs][:4])
    assert all(v >= 24 for v in figures.values()), figures
    assert {c["eids"] for c in cs} == {False, True} and largest > 4 * ref.TILE and min(c["n"] for c in cs) < 256 < max(c["n"] for c in cs)
    assert all(len(c["caps"]) >= 2 and c["caps"][0] <= c["M"] < c["caps"][-1] for c in cs)
    assert sum(int((c["block"]["src_local"] < 0).sum()) for c in cs) >= 1, "a dead entry in a block"


@pytest.fixture(scope="module")
def cases(hip):
    """seed -> the case on the device with its reference, built once and shared by the per-seed tests and the test of the seed set."""
    from legion_amd import engine
    made = {}

    def get(seed):
        if seed not in made:
            c = in_edges_shape(seed)
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
    g, want = c["graph"], c["want"]
    ctx = f"seed {seed} (kind {seed % 4}, N {c['indptr'].size - 1}, E {c['col'].size}): n {c['n']} M {c['M']} eids {c['eids']}: "
    off = g.row_offsets(c["rows"])
    got = g.in_edges(c["rows"], return_eids=c["eids"])
    torch.cuda.synchronize()
    same_arrays(off, c["offsets"], ctx + "row_offsets")
    same_arrays(got[0], c["offsets"], ctx + "offsets")
    for name, x, w in zip(("dst", "src", "eid"), got[1:], want):
        same_arrays(x, w, ctx + name)
    for m in c["caps"]:
        capped = ref.in_edges(c["indptr"], c["col"], c["rows"], c["offsets"], m)
        out = abi(hip, g, c["rows"], None, m, c["eids"])
        for name, x, w in zip(("dst", "src", "eid"), out[:3], capped):
            if x is not None:
                same_arrays(x, w, ctx + f"m {m} {name}")
    b = c["block"]
    blk = g.full_neighbor_block(c["seeds"], return_eids=True)
    torch.cuda.synchronize()
    for name, x in zip(("input_nodes", "dst_local", "src_local", "offsets", "eids"), blk):
        same_arrays(x, b[name], ctx + "block " + name)


def test_the_seed_set_holds_its_conditions(cases):
    seed_set_conditions(cases)
