"""Seeded random shapes through induced edges and node_subgraph, bit for bit against tests/induced_ref.py: the sorted-row graphs of
tests/test_gpu_in_edges_fuzz.fuzz_shape (the four kinds of tests/test_gpu_fuzz.random_case, symmetrised on some seeds, dead first entries
on the odd ones) with 1 to 3 000 rows drawn with repeats from [-2, N + 2]; the set (every vertex in order or shuffled, a random part with
repeats, negatives and ids outside the graph, a handful, none), m (the rows' M, or a prefix of it) and cap come from
RandomState(62000 + seed).  Per seed: induced_edges sized exactly, the C ABI's calls with m and cap followed by legion_dst_offsets, and
node_subgraph over distinct vertices.

Before the kernels run every index the reference reads is shown inside its array, and one test over the seed set asserts from the
references that the 24 cases hold what they are there for.  A failure names the seed and the shape."""
import numpy as np
import pytest
import torch

from tests import in_edges_ref
from tests import induced_ref as ref
from tests import walk_ref
from tests.compare import same_arrays
from tests.test_gpu_in_edges_fuzz import fuzz_shape
from tests.test_gpu_induced import NAMES, abi, dst_offsets

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEEDS = range(24)


def draw_set(rng, seed, node_num):
    kind = seed % 6
    everything = np.arange(node_num)
    if kind == 0:
        return everything
    if kind == 1:                                                  # a part, with repeats, negatives and ids outside the graph
        part = rng.choice(node_num, max(node_num // 2, 1), replace=False)
        return np.concatenate([part, part[:part.size // 3], [-1, node_num, node_num + 7, -3], part[-5:]])
    if kind == 2:
        return rng.choice(node_num, min(node_num, 6), replace=False)
    if kind == 3:
        return np.zeros(0, dtype=np.int64) if seed % 12 == 3 else rng.permutation(node_num)
    if kind == 4:
        return rng.choice(node_num, max(node_num // 3, 1), replace=False)
    return np.concatenate([everything[::-1], [-1], everything[:10], [2 ** 31 - 1]])


def induced_shape(seed):
    """Everything of a case that needs no GPU: the graph, the arguments and the references."""
    c = fuzz_shape(seed)
    indptr, col = c["indptr"], c["col"]
    node_num, E = indptr.size - 1, col.size
    rng = np.random.RandomState(62000 + seed)
    n = int(rng.randint(1, 3001))
    rows = rng.randint(-2, node_num + 2, n).astype(np.int32)
    if seed % 3 == 0:                                              # a run of rows without entries in the middle
        rows[n // 3:n // 3 + n // 4] = -1
    nodes = draw_set(rng, seed, node_num).astype(np.int32)
    eids = bool(rng.randint(2))
    reads = {}
    offsets = in_edges_ref.row_offsets(indptr, rows, reads=reads)
    M = int(offsets[-1])
    m = M if seed % 4 else max(M - int(rng.randint(1, 1500)), 0)   # every fourth: a prefix
    kept = ref.slot_mask(indptr, col, rows, offsets, m, nodes, reads=reads)[0]
    K, dst, local, eid = ref.edges(indptr, col, rows, offsets, m, nodes)
    walk_ref.assert_reads_in_bounds(reads, node_num, E)
    full = ref.edges_full(indptr, col, rows, nodes)
    caps = sorted({max(K - int(rng.randint(1, 300)), 0), K, K + int(rng.randint(1, 1500))})
    assert not ref.refused("edges", n, m, nodes.size, cap=caps[-1])
    k = int(rng.randint(1, min(node_num, 400) + 1))
    sub_nodes = rng.choice(node_num, k, replace=False).astype(np.int32)
    if seed % 2:
        sub_nodes.sort()
    entries = in_edges_ref.in_edges(indptr, col, rows, offsets, m)[1]
    t = ref.tile_counts(kept)
    whole = t[:m // ref.TILE]                                      # the tiles of 1 024 slots
    live = nodes[nodes >= 0]
    return dict(seed=seed, indptr=indptr, col=col, n=n, rows=rows, nodes=nodes, eids=eids, offsets=offsets, M=M, m=m, K=K,
                want=(dst, local, eid), full=full, caps=caps, sub_nodes=sub_nodes, sub=ref.node_subgraph(indptr, col, sub_nodes),
                empty_set=int(nodes.size == 0), repeats=int(np.unique(live).size < live.size), outside=int((nodes >= node_num).sum()),
                negative=int((nodes < 0).sum()), dead=int((entries < 0).sum()) if m else 0, none=int((whole == 0).sum()),
                all=int((whole == ref.TILE).sum()), thinned=int(m - (entries < 0).sum() - K) if m else 0)


def seed_set_conditions(shape_of):
    """What the seed set must hold, from the references alone."""
    cs = [shape_of(seed) for seed in SEEDS]
    figures = {key: sum(c[key] for c in cs) for key in ("empty_set", "repeats", "outside", "negative", "dead", "none", "all", "thinned")}
    print(figures, "K", [c["K"] for c in cs], "k", [c["nodes"].size for c in cs])
    assert all(v >= 1 for v in figures.values()), figures
    assert figures["dead"] >= 24 and figures["none"] >= 3 and figures["all"] >= 3
    assert {c["eids"] for c in cs} == {False, True} and max(c["m"] for c in cs) > 4 * ref.TILE
    assert any(c["K"] == 0 for c in cs) and any(0 < c["K"] < c["m"] for c in cs)
    assert any(c["caps"][0] < c["K"] for c in cs) and all(c["caps"][-1] > c["K"] for c in cs), "some case has cap < K"
    assert any(0 < c["m"] < c["M"] for c in cs)
    assert any(c["sub"][1].size > 0 for c in cs)


@pytest.fixture(scope="module")
def cases(hip):
    """seed -> the case on the device with its reference, built once and shared by the per-seed tests and the test of the seed set."""
    from legion_amd import engine
    made = {}

    def get(seed):
        if seed not in made:
            c = induced_shape(seed)
            c["graph"] = engine.GraphStorage(1, torch.from_numpy(c["indptr"]).to(DEV), torch.from_numpy(c["col"]).to(DEV))
            made[seed] = c
        return made[seed]

    yield get
    torch.cuda.synchronize()
    for c in made.values():
        c["graph"].close()


@pytest.mark.parametrize("seed", SEEDS)
def test_random_rows_and_sets_match_the_reference(cases, hip, seed):
    c = cases(seed)
    g = c["graph"]
    ctx = (f"seed {seed} (kind {seed % 4}, N {c['indptr'].size - 1}, E {c['col'].size}): n {c['n']} M {c['M']} m {c['m']} set {c['nodes'].size} "
           f"(kind {seed % 6}) K {c['K']} eids {c['eids']}: ")
    got = g.induced_edges(c["rows"], c["nodes"], return_eids=c["eids"])
    torch.cuda.synchronize()
    same_arrays(list(got), list(c["full"][:len(got)]), ctx, names=NAMES)
    for cap in c["caps"]:
        want = ref.edges(c["indptr"], c["col"], c["rows"], c["offsets"], c["m"], c["nodes"], cap=cap)
        k, *out = abi(hip, g, c["rows"], c["offsets"], c["m"], c["nodes"], cap, c["eids"])
        assert k == c["K"] == want[0], ctx + f"count {k}"
        for name, x, w in zip(NAMES, out, want[1:]):
            if x is not None:
                same_arrays(x, w, ctx + f"cap {cap} {name}")
        same_arrays(dst_offsets(hip, out[0], cap, k, c["n"]), ref.dst_offsets(want[1], cap, k, c["n"]), ctx + f"cap {cap} offsets")
    sub = g.node_subgraph(c["sub_nodes"], return_eids=True)
    torch.cuda.synchronize()
    same_arrays(list(sub), list(c["sub"]), ctx + "node_subgraph", names=("indptr_sub", "col_sub", "eids"))


def test_the_seed_set_holds_its_conditions(cases):
    seed_set_conditions(cases)
