"""GraphStorage.negative_sample / legion_negative_sample on the GPU, bit for bit against tests/link_ref.py: on the symmetric graph of
tests/node2vec_ref.py over every workgroup boundary in the row count, three k, the four exclusions, four max_tries and the whole range
of the draw index; and on two graphs of eight vertices, where the self-rejection (1 in 6 000 on the big graph) and the exhausted slot are
the rule rather than the exception.

The grid is the product thinned: case number c of the 18 (rows, k) pairs takes exclude c mod 4, max_tries number (c + c div 4) mod 4
and base number (c div 2) mod 3, so every exclusion meets every max_tries.  The references are computed once, with the counters that
show, before any launch, what the cases exercise."""
import numpy as np
import pytest
import torch

from tests import link_ref as ref
from tests import node2vec_ref, walk_ref

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


def _same(got, want, ctx):
    got = got.cpu().numpy()
    assert got.dtype == np.int32 and got.shape == want.shape, ctx
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{ctx}: {len(bad)} negatives differ, first at row, slot {bad[0]}: got {got[tuple(bad[0])]} want {want[tuple(bad[0])]}"


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
    _same(got, want, str(c))


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
    _same(got, want, f"K_8 exclude 3 tries {tries}")
    _same(got_own, own, f"K_8 exclude 2 tries {tries}")


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
    _same(got, want, f"ring exclude 1 tries {tries}")
    _same(both, ref.negative_sample(ip, c, rows, 5, 3, tries, 0), f"ring exclude 3 tries {tries}")


def test_an_empty_call_returns_an_empty_array(world):
    neg = world["graph"].negative_sample(np.zeros(0, np.int32), 7)
    assert neg.shape == (0, 7) and neg.dtype == torch.int32
