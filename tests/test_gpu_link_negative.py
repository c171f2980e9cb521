"""GraphStorage.negative_sample / legion_negative_sample on the GPU, bit for bit against tests/link_ref.py: on the symmetric graph of
tests/node2vec_ref.py over every workgroup boundary in the row count, three k, the four exclusions, four max_tries and the whole range
of the draw index; and on two graphs of eight vertices, where the self-rejection (1 in 6 000 on the big graph) and the exhausted slot are
the rule rather than the exception; on one vertex; and over 2^24 + 3 and 2^25 + 3 vertices, where the candidate floor(r * N) in double is
not what a float32 product gives.

The grid is the product thinned: case number c of the 18 (rows, k) pairs takes exclude c mod 4, max_tries number (c + c div 4) mod 4
and base number (c div 2) mod 3, so every exclusion meets every max_tries.  The references are computed once, with the counters that
show, before any launch, what the cases exercise."""
import functools

import numpy as np
import pytest
import torch

from tests import link_ref as ref
from tests import node2vec_ref, walk_ref
from tests.compare import same_arrays

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
COUNTS = [1, 63, 64, 65, 257, 5000]
KS = [1, 5, 64]
TRIES = [256, 1, 2, 3]
M31 = 2 ** 31 - 1


def case(n, k):
    c = COUNTS.index(n) * len(KS) + KS.index(k)
    base = [0, 1234567890, M31 - n * k][(c // 2) % 3]
    return dict(n=n, k=k, exclude=c % 4, tries=TRIES[(c + c // 4) % 4], base=base)


CASES = [case(n, k) for n in COUNTS for k in KS]


@pytest.fixture(scope="module")
def world(hip):
    from legion_amd import engine
    indptr, col, _ = node2vec_ref.sym_graph()
    graph = engine.GraphStorage(1, torch.from_numpy(indptr).to(DEV), torch.from_numpy(col).to(DEV))
    small = {}
    for name, (ip, c) in (("complete", ref.complete_graph(8)), ("ring", ref.ring_graph(8))):
        small[name] = (engine.GraphStorage(1, torch.from_numpy(ip).to(DEV), torch.from_numpy(c).to(DEV)), ip, c)
    made = {}

    def want(c):
        key = (c["n"], c["k"])
        if key not in made:
            stats, reads = ref.new_stats(node2vec_ref.NODE_NUM), {}
            out = ref.negative_sample(indptr, col, node2vec_ref.seeds_for(c["n"]), c["k"], c["exclude"], c["tries"], c["base"], reads=reads,
                                      stats=stats)
            walk_ref.assert_reads_in_bounds(reads, node2vec_ref.NODE_NUM, col.size)
            made[key] = (out, stats)
        return made[key]

    yield dict(graph=graph, small=small, indptr=indptr, col=col, want=want)
    torch.cuda.synchronize()
    graph.close()
    for g, _, _ in small.values():
        g.close()


same_negatives = functools.partial(same_arrays, names=("negatives (row, slot)",))


def test_the_cases_show_every_rejection_before_any_launch(world):
    """From the reference's counters alone: the figures of the issue on seeds_for(5000)[:600]; over the grid at least 100 rejections by a
    search hit, at least 100 exhausted slots where max_tries <= 3 and none at 256; the 4 097-entry row is searched and hit; every
    exclusion meets every max_tries; the draw index starts at 0 and ends at 2^31 - 1 somewhere."""
    indptr, col = world["indptr"], world["col"]
    rows = node2vec_ref.seeds_for(5000)[:600]
    two, full = ref.new_stats(node2vec_ref.NODE_NUM), ref.new_stats(node2vec_ref.NODE_NUM)
    ref.negative_sample(indptr, col, rows, 5, 3, 2, 0, stats=two)
    ref.negative_sample(indptr, col, rows, 5, 3, 256, 0, stats=full)
    assert two["rejected_slots"] == full["rejected_slots"] == 408 and two["exhausted"] == 272 and full["exhausted"] == 0
    hits = few = many = 0
    hub = np.zeros(2, dtype=np.int64)
    for c in CASES:
        s = world["want"](c)[1]
        hits += s["hit"]
        hub += (s["searches_of_row"][6], s["hits_of_row"][6])
        if c["tries"] <= 3:
            few += s["exhausted"]
        if c["tries"] == 256:
            many += s["exhausted"]
        rows = node2vec_ref.seeds_for(c["n"])
        assert c["n"] < 4 or (-1 in rows and node2vec_ref.NODE_NUM in rows)
    print("hits", hits, "exhausted at <= 3 tries", few, "at 256", many, "hub searches, hits", hub)
    assert hits >= 100 and few >= 100 and many == 0 and hub[1] >= 100 and node2vec_ref.HUBS[6] == 4097
    assert {(c["exclude"], c["tries"]) for c in CASES} == {(e, t) for e in range(4) for t in TRIES}
    assert {c["k"] for c in CASES} == set(KS)
    assert {(c["base"] == 0, c["base"] + c["n"] * c["k"] == M31) for c in CASES} == {(True, False), (False, True), (False, False)}


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", COUNTS)
def test_negatives_are_the_reference_bit_for_bit(world, n, k):
    c = case(n, k)
    want = world["want"](c)[0]
    rows = torch.from_numpy(node2vec_ref.seeds_for(n)).to(DEV)
    got = world["graph"].negative_sample(rows, k, exclude_self=bool(c["exclude"] & 1), exclude_edges=bool(c["exclude"] & 2),
                                         max_tries=c["tries"], base=c["base"])
    torch.cuda.synchronize()
    same_negatives(got, want, str(c))


@pytest.mark.parametrize("tries", [1, 3, 256])
def test_a_complete_graph_has_no_negatives(world, tries):
    """K_8 without loops: with both exclusions every slot is -1 at any max_tries; excluding the edges only, every value is the row itself."""
    g, ip, c = world["small"]["complete"]
    rows = np.arange(8, dtype=np.int32).repeat(40)
    want = ref.negative_sample(ip, c, rows, 5, 3, tries, 11)
    assert np.all(want == -1)
    own = ref.negative_sample(ip, c, rows, 5, 2, tries, 11)
    assert np.all((own == rows[:, None]) | (own == -1)) and (tries < 256 or np.all(own == rows[:, None]))
    got = g.negative_sample(rows, 5, max_tries=tries, base=11)
    got_own = g.negative_sample(rows, 5, exclude_self=False, max_tries=tries, base=11)
    torch.cuda.synchronize()
    same_negatives(got, want, f"K_8 exclude 3 tries {tries}")
    same_negatives(got_own, own, f"K_8 exclude 2 tries {tries}")


@pytest.mark.parametrize("tries", [1, 2, 256])
def test_a_ring_rejects_the_row_itself(world, tries):
    g, ip, c = world["small"]["ring"]
    rows = np.arange(8, dtype=np.int32).repeat(40)
    stats = ref.new_stats(8)
    want = ref.negative_sample(ip, c, rows, 5, 1, tries, 0, stats=stats)
    assert stats["self"] >= 10 and (tries > 1 or (want == -1).sum() == stats["self"])
    got = g.negative_sample(rows, 5, exclude_edges=False, max_tries=tries)
    both = g.negative_sample(rows, 5, max_tries=tries)
    torch.cuda.synchronize()
    same_negatives(got, want, f"ring exclude 1 tries {tries}")
    same_negatives(both, ref.negative_sample(ip, c, rows, 5, 3, tries, 0), f"ring exclude 3 tries {tries}")


def test_one_vertex(hip):
    """N = 1, a self-loop: the only candidate is 0.  Excluding the row itself (or its edges) every slot is -1; excluding nothing, 0."""
    from legion_amd import engine
    ip, c = np.array([0, 1], dtype=np.int64), np.array([0], dtype=np.int32)
    rows = np.array([0] * 300 + [-1, 1], dtype=np.int32)
    want = {e: ref.negative_sample(ip, c, rows, 5, e, 3, 9) for e in range(4)}
    assert np.all(want[0][:300] == 0) and all(np.all(want[e] == -1) for e in (1, 2, 3)) and np.all(want[0][300:] == -1)
    g = engine.GraphStorage(1, torch.from_numpy(ip).to(DEV), torch.from_numpy(c).to(DEV))
    try:
        for e in range(4):
            got = g.negative_sample(rows, 5, exclude_self=bool(e & 1), exclude_edges=bool(e & 2), max_tries=3, base=9)
            torch.cuda.synchronize()
            same_negatives(got, want[e], f"one vertex, exclude {e}")
    finally:
        torch.cuda.synchronize()
        g.close()


BIG = [2 ** 24 + 3, 2 ** 25 + 3]
BIG_N, BIG_K, BIG_BASE, HUB_ENTRIES, HUB_FROM_DRAWS = 5000, 5, 77, 1000, 300


def draw_in_float32(rows, k, base, node_num):
    """A wrong draw with no exclusion: the unit and the product in float32, floor(float(r) * float(N)), capped at N - 1."""
    x = walk_ref.draws(base, rows.size * k)
    u = np.floor(walk_ref.unit_of(x).astype(np.float32) * np.float32(node_num)).astype(np.int64)
    out = np.where(np.repeat((rows >= 0) & (rows < node_num), k), np.minimum(u, node_num - 1), -1)
    return out.reshape(rows.size, k).astype(np.int32)


def big_case(node_num):
    """(indptr, col, rows, {exclude: reference}) over node_num vertices whose rows are empty except one sorted hub of 1 000 entries, 300
    of them what the hub's own slots draw first (so its search is hit: uniform chance, 1 000 in 2^24, would not) and 2^24 + 1 and
    2^24 + 2 among the rest.  Checked from the reference: the hub's search is hit, a float32 draw differs in at least 100 slots, and
    -- over 2^25 + 3 vertices; over 2^24 + 3 the only such value is 2^24 + 1, drawn once in 16 million -- at least 100 expected values
    are odd and above 2^24, which no float32 holds."""
    hub = 2 ** 24 + 1
    rows = (np.arange(BIG_N, dtype=np.int64) * 2654435761 % node_num).astype(np.int32)
    rows[::5] = hub
    rows[1], rows[2], rows[3] = -1, node_num, node_num - 1
    indptr = np.zeros(node_num + 1, dtype=np.int64)
    free = ref.negative_sample(indptr, np.zeros(0, dtype=np.int32), rows, BIG_K, 0, 1, BIG_BASE)      # no exclusion: try 0 of every slot
    drawn = np.unique(free[rows == hub].reshape(-1))[:HUB_FROM_DRAWS]
    rest = np.concatenate([[0, hub, 2 ** 24 + 2, node_num - 1], np.random.RandomState(5).randint(0, node_num, 2 * HUB_ENTRIES)])
    rest = rest[np.sort(np.unique(rest, return_index=True)[1])]                                     # distinct, the four named ones first
    rest = rest[~np.isin(rest, drawn)]
    col = np.sort(np.concatenate([drawn, rest[:HUB_ENTRIES - drawn.size]])).astype(np.int32)
    assert col.size == HUB_ENTRIES and drawn.size == HUB_FROM_DRAWS and np.unique(col).size == col.size and (col > 2 ** 24).any()
    indptr[hub + 1:] = HUB_ENTRIES
    want = {}
    for exclude in (0, 3):
        reads, stats = {}, ref.new_stats(node_num)
        want[exclude] = ref.negative_sample(indptr, col, rows, BIG_K, exclude, 256, BIG_BASE, reads=reads, stats=stats)
        walk_ref.assert_reads_in_bounds(reads, node_num, col.size)
        assert np.all(want[exclude][1:3] == -1) and want[exclude].max() < node_num
        if exclude:
            assert stats["hits_of_row"][hub] >= HUB_FROM_DRAWS and stats["exhausted"] == 0 and stats["self"] == 0
            assert int((want[3] != want[0]).sum()) >= HUB_FROM_DRAWS
    assert np.array_equal(want[0], free)
    odd_high = int(((want[0] > 2 ** 24) & (want[0] % 2 == 1)).sum())
    off = int((draw_in_float32(rows, BIG_K, BIG_BASE, node_num) != want[0]).sum())
    print(f"N {node_num}: {odd_high} expected values odd and above 2^24, a float32 draw differs in {off} of {want[0].size} slots")
    assert off >= 100 and (node_num < 2 ** 25 or odd_high >= 100)
    return indptr, col, rows, want


@pytest.mark.parametrize("node_num", BIG, ids=["2^24+3", "2^25+3"])
def test_the_draw_over_more_than_2_24_vertices(hip, node_num):
    from legion_amd import engine
    indptr, col, rows, want = big_case(node_num)
    g = engine.GraphStorage(1, torch.from_numpy(indptr).to(DEV), torch.from_numpy(col).to(DEV))
    try:
        for exclude in (0, 3):
            got = g.negative_sample(rows, BIG_K, exclude_self=bool(exclude & 1), exclude_edges=bool(exclude & 2), base=BIG_BASE)
            torch.cuda.synchronize()
            same_negatives(got, want[exclude], f"N {node_num}, exclude {exclude}")
    finally:
        torch.cuda.synchronize()
        g.close()


def test_an_empty_call_returns_an_empty_array(world):
    neg = world["graph"].negative_sample(np.zeros(0, np.int32), 7)
    assert neg.shape == (0, 7) and neg.dtype == torch.int32
