"""GraphStorage.induced_edges and the C ABI's legion_induced_count / legion_induced_edges / legion_dst_offsets on the GPU, bit for bit
against tests/induced_ref.py on the symmetric graph of tests/node2vec_ref.py (6 000 vertices, 53 448 entries, 30 dead, 6 empty rows, a
4 097-entry hub), with and without edge ids: the plain case, the identity (every live entry, whole tiles kept), the hub's neighbourhood,
a set in shuffled order, a set of eight on all rows (tiles and waves that keep nothing: the skip path), repeats with ids outside the
graph, rows that are not the set at every workgroup boundary in n, and a set whose table wraps; capacities at, below and above K; m
below M ending inside the hub; runs of rows without entries (the search in global memory); the empty set; the small graphs of link_ref;
a scratch that legion_induced_count did not write; legion_dst_offsets at cap below, at and above K and over runs of empty rows; one
captured graph holding count, edges and offsets; another stream; and every refusal of the C ABI over sentinel-filled buffers.  What
makes a wrong kernel fail is asserted from the numpy reference alone before any launch; an input that fails a condition is replaced,
never the condition."""
import ctypes

import numpy as np
import pytest
import torch

from tests import in_edges_ref
from tests import induced_ref as ref
from tests import link_ref, node2vec_ref
from tests.compare import same_arrays
from tests.test_gpu_labor import empty_rows, gap_rows, small_cases, small_rows
from tests.test_gpu_node_set import SENTINEL, P, build, stream_of

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = node2vec_ref.NODE_NUM
HUB = 6
COUNTS = [1, 63, 64, 65, 256, 257, 1023, 1024, 1025]
NAMES = ("dst", "src_local", "eid")
EIGHT = np.array([6, 0, 5, 100, 101, 102, 3, 4], dtype=np.int32)


def half_set():
    return np.random.RandomState(7).permutation(N)[:3000].astype(np.int32)


def table(indptr, col):
    """name -> (rows, nodes, M, K): the figures were computed on the CPU with a numpy restatement before the kernels existed; None: not pinned."""
    third = np.arange(0, N, 3, dtype=np.int32)
    everything = np.arange(N, dtype=np.int32)
    hub_row = col[indptr[HUB]:indptr[HUB + 1]]
    hubs = np.unique(np.concatenate([np.arange(12), hub_row[hub_row >= 0]])).astype(np.int32)
    half = half_set()
    repeats = np.concatenate([half[:1000], half[:500], [-1, N, N + 5]]).astype(np.int32)
    out = {"third": (third, third, 20560, 7956), "identity": (everything, everything, 53448, 53418), "hubs": (hubs, hubs, 39387, 29794),
           "shuffled": (half, half, 28647, 15475), "eight-of-all": (everything, EIGHT, 53448, 4934), "eight": (EIGHT, EIGHT, 4953, 26),
           "repeats": (everything, repeats, 53448, 8147), "wrap": (everything, ref.wrap_set()[0], 53448, None)}
    for n, K in zip(COUNTS, (2063, 23399, 21346, 23409, 104528, 104534, 422849, 420798, 422861)):
        out[f"rows-{n}"] = (node2vec_ref.seeds_for(n), half, None, K)
    return out


def reference(indptr, col, rows, nodes, m=None):
    """(offsets, M or m, kept mask, K, dst, src_local, eid) of the reference."""
    off = in_edges_ref.row_offsets(indptr, rows)
    m = int(off[-1]) if m is None else m
    kept = ref.slot_mask(indptr, col, rows, off, m, nodes)[0]
    K, dst, local, eid = ref.edges(indptr, col, rows, off, m, nodes)
    assert K == int(kept.sum()) and dst.shape == (K,) and np.all(np.diff(dst) >= 0) and (K == 0 or (local.min() >= 0 and local.max() < nodes.size))
    return off, m, kept, K, dst, local, eid


def conditions(name, indptr, col, rows, nodes, M, K):
    """What the case must hold for a wrong kernel to fail on it; returns reference()."""
    out = reference(indptr, col, rows, nodes)
    off, m, kept, k, dst, local, eid = out
    assert (M is None or m == M) and (K is None or k == K), (name, m, k)
    t, w = ref.tile_counts(kept), ref.wave_counts(kept)
    src = in_edges_ref.in_edges(indptr, col, rows, off, m)[1]
    differs = lambda wrong: not all(np.array_equal(a, b) for a, b in zip(ref.edges(indptr, col, rows, off, m, nodes, wrong=wrong)[1:], out[4:]))
    if name == "third":
        assert not np.array_equal(ref.lane_major(eid, kept), eid), "lane-major ranks differ"
        assert differs("global-src") and differs("member-of-dst"), "rows == set: dst's vertex is always a member, and keeps every live entry"
    if name == "identity":
        assert np.array_equal(kept, src >= 0) and (t == ref.TILE).sum() == 22 and (src < 0).sum() == 30 and np.array_equal(local, src[kept])
        assert differs("dead-matches-empty"), "a dead entry matched against the empty key is kept"
    if name == "hubs":
        assert nodes.size == 4102 and (t == ref.TILE).sum() == 3 and (w == 64).sum() == 64
    if name == "shuffled":
        assert np.all(local != src[kept]), "local != global everywhere"
        assert differs("global-src")
    if name == "eight-of-all":
        assert (t == 0).sum() == 2 and (w == 0).sum() == 71 and link_ref.table_slots(nodes.size) == 256
        assert differs("member-of-dst")
    if name == "eight":
        assert t.size == 5 and (t == 0).sum() == 3
    if name == "repeats":
        assert differs("last-position"), "the last position of a repeated node differs"
    if name == "wrap":
        members = ref.wrap_set()[1]
        assert members.size == 46 and members[:4].tolist() == [144, 288, 377, 521] and nodes.size == 100 and np.isin(members, src).all()
        for order in (np.arange(100), np.arange(100)[::-1]):
            _, longest, wraps = link_ref.probe_table(nodes, 100, order)
            assert wraps == 44 and 49 <= longest <= 58 and len(ref.lost_without_wrap(nodes, order)) == 44
            assert not np.array_equal(ref.edges(indptr, col, rows, off, m, nodes, wrong="no-wrap", order=order)[3], eid)
    if name.startswith("rows-") and rows.size >= 63:
        assert not np.array_equal(ref.lane_major(eid, kept), eid) and differs("member-of-dst") and differs("global-src")
        assert (rows == -1).sum() >= 1 and (rows == N).sum() >= 1 and np.unique(rows).size < rows.size, "repeats, -1 and N among the rows"
    return out


@pytest.fixture(scope="module")
def world(hip):
    from legion_amd import engine
    indptr, col, _ = node2vec_ref.sym_graph()
    graph = engine.GraphStorage(1, torch.from_numpy(indptr).to(DEV), torch.from_numpy(col).to(DEV))
    yield dict(graph=graph, indptr=indptr, col=col, L=hip, table=table(indptr, col))
    torch.cuda.synchronize()
    graph.close()


def abi(L, graph, rows, off, m, nodes, cap, with_eids=True, stream=None, scratch_fill=None, set_offset=0):
    """legion_node_set_build + legion_induced_count + legion_induced_edges over sentinel-filled buffers of cap + 8 entries and a scratch
    with 8 spare entries: (K as _count wrote it, dst, src_local, eid or None) of cap entries; the tails are checked untouched.
    scratch_fill: a value to fill the scratch with INSTEAD of calling _count (K is then None)."""
    n = rows.size
    d_rows = torch.from_numpy(np.ascontiguousarray(rows)).to(DEV) if n else torch.zeros(1, dtype=torch.int32, device=DEV)
    d_off = torch.from_numpy(np.ascontiguousarray(off)).to(DEV)
    s = stream_of(stream)
    tab, set_bytes, k, _, distinct = build(L, nodes, stream, offset=set_offset)
    nbytes = int(L.legion_induced_scratch_bytes(m))
    assert nbytes == ref.scratch_bytes(m) and nbytes % 8 == 0
    scratch = torch.full((nbytes // 8 + 8,), SENTINEL if scratch_fill is None else scratch_fill, dtype=torch.int64, device=DEV)
    count = torch.full((1 + 8,), SENTINEL, dtype=torch.int64, device=DEV)
    if scratch_fill is None:
        assert L.legion_induced_count(s, graph.handle, P(d_rows), n, P(d_off), m, P(tab), set_bytes, k, P(count), P(scratch), nbytes) == 0
    dst = torch.full((cap + 8,), SENTINEL, dtype=torch.int32, device=DEV)
    src = torch.full((cap + 8,), SENTINEL, dtype=torch.int32, device=DEV)
    eid = torch.full((cap + 8,), SENTINEL, dtype=torch.int64, device=DEV) if with_eids else None
    assert L.legion_induced_edges(s, graph.handle, P(d_rows), n, P(d_off), m, P(tab), set_bytes, k, P(scratch), nbytes, cap, P(dst), P(src),
                                  P(eid)) == 0
    torch.cuda.synchronize()
    fill = SENTINEL if scratch_fill is None else scratch_fill
    assert bool((scratch[nbytes // 8:] == fill).all()) and bool((count[1:] == SENTINEL).all()), "written past the scratch or the count"
    assert bool((tab[set_bytes // 4:] == SENTINEL).all()) and int(distinct[0].item()) == ref.distinct(nodes)
    K = None
    if scratch_fill is None:
        K = int(count[0].item())
        assert int(scratch[ref.labor_ref.tiles_of(m)].item()) == K, "the total in the scratch"
    out = [x.cpu().numpy() if x is not None else None for x in (dst, src, eid)]
    for x in out:
        assert x is None or np.all(x[cap:] == SENTINEL), "written past cap"
    return [K] + [x[:cap] if x is not None else None for x in out]


def same(got, want, what):
    got, want = zip(*[(g, w) for g, w in zip(got, want) if g is not None])
    same_arrays(list(got), list(want), what, names=NAMES)


CASES = sorted(["third", "identity", "hubs", "shuffled", "eight-of-all", "eight", "repeats", "wrap"] + [f"rows-{n}" for n in COUNTS])


# ---- the inputs -------------------------------------------------------------------------------------------------------------------
def test_the_inputs_hold_their_conditions_before_any_launch(world):
    indptr, col = world["indptr"], world["col"]
    assert col.size == 53448 and (col < 0).sum() == 30 and np.diff(indptr)[HUB] == 4097
    assert sorted(world["table"]) == CASES
    for name in ("third", "identity", "eight-of-all", "wrap", "rows-257"):
        conditions(name, indptr, col, *world["table"][name])
    off, M, kept = reference(indptr, col, gap_rows(), half_set())[:3]
    spans = in_edges_ref.tile_ranges(off, M)
    assert spans.max() > in_edges_ref.STAGE and (spans > in_edges_ref.STAGE).sum() >= 2 and 0 < kept.sum() < M, "both searches run"
    assert int(in_edges_ref.row_offsets(indptr, empty_rows())[-1]) == 0


# ---- bit for bit ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eids", [False, True], ids=["no-eids", "eids"])
@pytest.mark.parametrize("name", CASES)
def test_the_table_is_the_reference_bit_for_bit(world, name, eids):
    from legion_amd import engine
    indptr, col, g = world["indptr"], world["col"], world["graph"]
    rows, nodes, M, K = world["table"][name]
    off, M, kept, K, dst, local, eid = conditions(name, indptr, col, rows, nodes, M, K)
    k, *out = abi(world["L"], g, rows, off, M, nodes, K, eids)
    assert k == K, f"{name}: K {k} want {K}"
    same(out, (dst, local, eid), f"abi: {name}")
    given = nodes if eids else engine.NodeSet(torch.from_numpy(nodes).to(DEV))       # a list and a NodeSet
    got = g.induced_edges(torch.from_numpy(rows).to(DEV) if eids else rows, given, return_eids=eids)
    torch.cuda.synchronize()
    assert len(got) == (3 if eids else 2) and all(x.is_cuda for x in got)
    same(list(got) + [None] * (3 - len(got)), (dst, local, eid), name)


@pytest.mark.parametrize("name", ["third", "wrap", "repeats", "rows-257"])
def test_a_set_that_starts_behind_a_16_byte_boundary(world, name):
    """The kernels then probe key by key, not four keys a load: the same result."""
    indptr, col = world["indptr"], world["col"]
    rows, nodes, M, K = world["table"][name]
    off, M, kept, K, dst, local, eid = reference(indptr, col, rows, nodes)
    for offset in (1, 3):
        k, *out = abi(world["L"], world["graph"], rows, off, M, nodes, K, set_offset=offset)
        assert k == K
        same(out, (dst, local, eid), f"{name}, the set at {4 * offset} bytes")


@pytest.mark.parametrize("eids", [False, True], ids=["no-eids", "eids"])
def test_cap_is_a_capacity(world, eids):
    indptr, col = world["indptr"], world["col"]
    rows, nodes, M, K = world["table"]["third"]
    off = in_edges_ref.row_offsets(indptr, rows)
    assert K > ref.TILE
    for cap in (K, K - 1, K + 1000, 1):
        want = ref.edges(indptr, col, rows, off, M, nodes, cap=cap)
        assert cap <= K or all(np.all(w[K:] == -1) for w in want[1:])
        k, *out = abi(world["L"], world["graph"], rows, off, M, nodes, cap, eids)
        assert k == K, "the count does not depend on cap"
        same(out, want[1:], f"cap {cap}")


def prefix_case(indptr, col):
    """m below M, ending inside the second copy of the hub and inside a tile."""
    rows = node2vec_ref.seeds_for(257)
    off = in_edges_ref.row_offsets(indptr, rows)
    hub_at = int(np.nonzero(rows == HUB)[0][1])
    m = int(off[hub_at]) + 2000
    assert off[hub_at] < m < off[hub_at + 1] and m % ref.TILE != 0
    want = ref.edges(indptr, col, rows, off, m, half_set())
    assert 0 < want[0] < ref.count(indptr, col, rows, off, int(off[-1]), half_set())
    return rows, off, m, want


def test_m_below_M_ends_inside_the_hub(world):
    rows, off, m, want = prefix_case(world["indptr"], world["col"])
    k, *out = abi(world["L"], world["graph"], rows, off, m, half_set(), want[0] + 10)
    assert k == want[0]
    same(out, ref.edges(world["indptr"], world["col"], rows, off, m, half_set(), cap=want[0] + 10)[1:], "a prefix")


def test_runs_of_rows_without_entries_take_the_search_in_global_memory(world):
    indptr, col = world["indptr"], world["col"]
    rows = gap_rows()
    for nodes in (half_set(), np.arange(N, dtype=np.int32)):
        off, M, kept, K, dst, local, eid = reference(indptr, col, rows, nodes)
        assert in_edges_ref.tile_ranges(off, M).max() > in_edges_ref.STAGE and K > 0
        got = world["graph"].induced_edges(rows, nodes, return_eids=True)
        torch.cuda.synchronize()
        same(got, (dst, local, eid), f"gap, {nodes.size} nodes")
    assert set(np.unique(dst).tolist()) == set(np.nonzero(np.diff(off) > 0)[0].tolist()), "no row with entries is skipped"


def test_all_rows_empty_and_the_empty_set(world):
    g, L = world["graph"], world["L"]
    rows = empty_rows()
    got = g.induced_edges(rows, half_set(), return_eids=True)
    torch.cuda.synchronize()
    assert all(x.shape == (0,) for x in got) and [x.dtype for x in got] == [torch.int32, torch.int32, torch.int64]
    off = np.zeros(rows.size + 1, np.int64)
    for m, cap in ((0, 1500), (1500, 700)):                               # M = 0: a zero total, the fill only; slots that resolve to no row
        k, dst, src, eid = abi(L, g, rows, off, m, half_set(), cap)
        assert k == 0 and np.all(dst == -1) and np.all(src == -1) and np.all(eid == -1)
    k, dst, src, eid = abi(L, g, np.zeros(0, np.int32), np.zeros(1, np.int64), 0, EIGHT, 8)      # n == 0: the same
    assert k == 0 and np.all(dst == -1) and np.all(src == -1) and np.all(eid == -1)
    # k = 0: every slot is resolved, none is kept
    rows = node2vec_ref.seeds_for(257)
    off = in_edges_ref.row_offsets(world["indptr"], rows)
    none = np.zeros(0, np.int32)
    k, dst, src, eid = abi(L, g, rows, off, int(off[-1]), none, 300)
    assert k == 0 and np.all(dst == -1) and np.all(src == -1) and np.all(eid == -1)
    got = g.induced_edges(rows, none, return_eids=True)
    assert all(x.shape == (0,) for x in got)
    assert all(x.shape == (0,) for x in g.induced_edges(none, none))


@pytest.mark.parametrize("name", sorted(small_cases()))
def test_small_graphs(hip, name):
    from legion_amd import engine
    indptr, col = small_cases()[name]
    n = indptr.size - 1
    rows = small_rows(indptr)
    g = engine.GraphStorage(1, torch.from_numpy(indptr).to(DEV), torch.from_numpy(col).to(DEV))
    try:
        sets = {"all": np.arange(n), "backwards-with-strangers": np.concatenate([[n + 3, -1], np.arange(n)[::-1], [n]]), "even": np.arange(0, n, 2),
                "first-twice": np.array([0, 0]), "none": np.zeros(0)}
        for what, nodes in sets.items():
            nodes = nodes.astype(np.int32)
            want = ref.edges_full(indptr, col, rows, nodes)
            got = g.induced_edges(rows, nodes, return_eids=True)
            torch.cuda.synchronize()
            same(got, want, f"{name} {what}")
            if what == "all":
                assert want[0].size == 2 * int((col >= 0).sum()), "the identity keeps every live entry"
    finally:
        torch.cuda.synchronize()
        g.close()


@pytest.mark.parametrize("fill", [0, 2 ** 40, -1], ids=["zero", "2^40", "minus-one"])
def test_a_scratch_that_count_did_not_write(world, fill):
    """Only [0, cap) is written, whatever the scratch holds: the tails of abi() are checked.  The values are unspecified, but each is
    one the kernel writes: all bases 0 or -1 put every tile's triples over the fill of the whole buffer; all bases 2^40 drop every triple
    and clamp the fill to nothing."""
    indptr, col = world["indptr"], world["col"]
    rows, nodes, M, K = world["table"]["third"]
    off = in_edges_ref.row_offsets(indptr, rows)
    for cap in (K, 100):
        _, d, s, e = abi(world["L"], world["graph"], rows, off, M, nodes, cap, scratch_fill=fill)
        if fill == 2 ** 40:
            assert np.all(d == SENTINEL) and np.all(s == SENTINEL) and np.all(e == SENTINEL), "every triple dropped, the fill clamped to [cap, cap)"
        else:
            assert np.all((d == -1) | ((d >= 0) & (d < rows.size))) and np.all((e == -1) | ((e >= 0) & (e < col.size)))
            assert np.all((s == -1) | ((s >= 0) & (s < nodes.size)))


# ---- the row pointers ---------------------------------------------------------------------------------------------------------------
def dst_offsets(L, dst, cap, count, n, stream=None):
    """legion_dst_offsets over a sentinel-filled indptr of n + 1 + 8 entries; dst: cap entries at least."""
    d_dst = torch.from_numpy(np.ascontiguousarray(dst)).to(DEV) if dst.size else torch.zeros(1, dtype=torch.int32, device=DEV)
    d_count = torch.tensor([count], dtype=torch.int64, device=DEV)
    out = torch.full((n + 1 + 8,), SENTINEL, dtype=torch.int64, device=DEV)
    assert L.legion_dst_offsets(stream_of(stream), P(d_dst), cap, P(d_count), n, P(out)) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.all(got[n + 1:] == SENTINEL), "written past indptr_out"
    return got[:n + 1]


def offsets_cases(indptr, col):
    """(rows, nodes, off, M, K, dst, rows' kept counts) of the inputs of legion_dst_offsets: runs of rows that keep nothing in each."""
    for rows, nodes in ((half_set(),) * 2, (gap_rows(), half_set()), (node2vec_ref.seeds_for(1025), EIGHT)):
        off, M, kept, K, dst, local, eid = reference(indptr, col, rows, nodes)
        n = rows.size
        per_row = np.bincount(dst, minlength=n)
        assert (per_row == 0).sum() >= 3 and K > 10, "rows that keep nothing"
        assert not np.array_equal(ref.dst_offsets(dst, K, K, n, upper=True), ref.dst_offsets(dst, K, K, n)), "an upper bound differs"
        yield rows, nodes, off, M, K, dst, per_row


def test_dst_offsets(world):
    indptr, col, L = world["indptr"], world["col"], world["L"]
    for rows, nodes, off, M, K, dst, per_row in offsets_cases(indptr, col):
        n = rows.size
        for cap in (K - 7, K, K + 1000):
            buf = ref.edges(indptr, col, rows, off, M, nodes, cap=cap)[1]       # what legion_induced_edges leaves: -1 from K on
            want = ref.dst_offsets(buf, cap, K, n)
            assert want[-1] == min(K, cap) and want[0] == 0 and np.all(np.diff(want) >= 0)
            assert cap < K or np.array_equal(np.diff(want), per_row)
            same_arrays(dst_offsets(L, buf, cap, K, n), want, f"dst_offsets n {n} cap {cap}")
        for count in (-5, 0, 3, 2 ** 40):                                      # the count is clamped to [0, cap]
            same_arrays(dst_offsets(L, dst, K, count, n), ref.dst_offsets(dst, K, count, n), f"count {count}")
    same_arrays(dst_offsets(L, np.zeros(0, np.int32), 0, 0, 5), np.zeros(6, np.int64), "cap 0")
    same_arrays(dst_offsets(L, np.array([0, 0, 2], np.int32), 3, 3, 0), np.zeros(1, np.int64), "n 0")
    down = np.array([5, 1, 4, 0, 3, 3, 9, 2], dtype=np.int32)                  # not non-decreasing: some value in [0, L]
    got = dst_offsets(L, down, 8, 8, 10)
    assert np.all((got >= 0) & (got <= 8))


# ---- streams and graphs ---------------------------------------------------------------------------------------------------------------
def test_another_stream_and_one_captured_graph_of_count_edges_and_offsets(world):
    indptr, col, L, g = world["indptr"], world["col"], world["L"], world["graph"]
    rows, nodes = node2vec_ref.seeds_for(1025), half_set()
    off, M, kept, K, dst, local, eid = reference(indptr, col, rows, nodes)
    assert K == 422861
    d_rows = torch.from_numpy(rows).to(DEV)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    assert s != torch.cuda.current_stream()
    got = g.induced_edges(d_rows, nodes, return_eids=True, stream=s)
    s.synchronize()
    same(got, (dst, local, eid), "another stream")

    n, cap, k = rows.size, K + 500, nodes.size
    nbytes, set_bytes = int(L.legion_induced_scratch_bytes(M)), int(L.legion_node_set_bytes(k))
    scratch = torch.zeros(nbytes // 8, dtype=torch.int64, device=DEV)
    tab = torch.zeros(set_bytes // 4, dtype=torch.int32, device=DEV)
    d_nodes, d_off = torch.from_numpy(nodes).to(DEV), torch.from_numpy(off).to(DEV)
    distinct = torch.zeros(1, dtype=torch.int32, device=DEV)
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    o_dst, o_src = (torch.zeros(cap, dtype=torch.int32, device=DEV) for _ in range(2))
    o_eid = torch.zeros(cap, dtype=torch.int64, device=DEV)
    o_ptr = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cs = stream_of()
        rc = [L.legion_node_set_build(cs, P(d_nodes), k, P(tab), set_bytes, P(distinct)),
              L.legion_induced_count(cs, g.handle, P(d_rows), n, P(d_off), M, P(tab), set_bytes, k, P(count), P(scratch), nbytes),
              L.legion_induced_edges(cs, g.handle, P(d_rows), n, P(d_off), M, P(tab), set_bytes, k, P(scratch), nbytes, cap, P(o_dst), P(o_src),
                                     P(o_eid)),
              L.legion_dst_offsets(cs, P(o_dst), cap, P(count), n, P(o_ptr))]
    assert rc == [0, 0, 0, 0]
    capped = ref.edges(indptr, col, rows, off, M, nodes, cap=cap)[1:]
    want_ptr = ref.dst_offsets(capped[0], cap, K, n)
    for _ in range(2):
        for x in (tab, distinct, count, scratch, o_dst, o_src, o_eid, o_ptr):
            x.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        assert int(count.item()) == K and int(distinct.item()) == k
        same((o_dst, o_src, o_eid), capped, "captured")
        same_arrays(o_ptr, want_ptr, "captured offsets")


# ---- the C ABI's refusals -----------------------------------------------------------------------------------------------------------
def test_c_abi_refusals_leave_the_outputs_untouched(world):
    L, g = world["L"], world["graph"].handle
    n, m, cap, k = 8, 64, 64, 8
    rows = torch.from_numpy(node2vec_ref.seeds_for(n)).to(DEV)
    off = torch.full((n + 1,), SENTINEL, dtype=torch.int64, device=DEV)
    tab = torch.full((2048 // 4,), SENTINEL, dtype=torch.int32, device=DEV)
    scratch = torch.full((4,), SENTINEL, dtype=torch.int64, device=DEV)
    count = torch.full((2,), SENTINEL, dtype=torch.int64, device=DEV)
    dst, src = (torch.full((cap,), SENTINEL, dtype=torch.int32, device=DEV) for _ in range(2))
    eid = torch.full((cap,), SENTINEL, dtype=torch.int64, device=DEV)
    ptr = torch.full((n + 1,), SENTINEL, dtype=torch.int64, device=DEV)
    s = stream_of()
    assert L.legion_induced_scratch_bytes(m) == 24 == ref.scratch_bytes(m)
    for bad_m in (-1, 2 ** 30 + 1):
        assert L.legion_induced_scratch_bytes(bad_m) == -1 == ref.scratch_bytes(bad_m)
    ok = dict(graph=g, rows=P(rows), n=n, off=P(off), m=m, set=P(tab), set_b=2048, k=k, count=P(count), scratch=P(scratch), bytes=24)
    for change in (dict(graph=None), dict(rows=None), dict(off=None), dict(set=None), dict(count=None), dict(scratch=None), dict(n=-1),
                   dict(n=2 ** 20 + 1), dict(m=-1), dict(m=2 ** 30 + 1, bytes=1 << 40), dict(m=2 ** 40, bytes=1 << 40), dict(k=-1),
                   dict(k=2 ** 20 + 1, set_b=1 << 40), dict(k=129), dict(set_b=2047), dict(set_b=-1), dict(bytes=23), dict(bytes=0),
                   dict(bytes=-1), dict(m=1025)):
        a = dict(ok, **change)
        assert None in (a["graph"], a["rows"], a["off"], a["set"], a["count"], a["scratch"]) or \
            ref.refused("count", a["n"], a["m"], a["k"], a["set_b"], a["bytes"]), change
        assert L.legion_induced_count(s, a["graph"], a["rows"], a["n"], a["off"], a["m"], a["set"], a["set_b"], a["k"], a["count"], a["scratch"],
                                      a["bytes"]) == -1, change
    ok = dict(graph=g, rows=P(rows), n=n, off=P(off), m=m, set=P(tab), set_b=2048, k=k, scratch=P(scratch), bytes=24, cap=cap, dst=P(dst),
              src=P(src), eid=P(eid))
    for change in (dict(graph=None), dict(rows=None), dict(off=None), dict(set=None), dict(scratch=None), dict(dst=None), dict(src=None),
                   dict(n=-1), dict(n=2 ** 20 + 1), dict(m=-1), dict(m=2 ** 30 + 1, bytes=1 << 40), dict(k=-1), dict(k=2 ** 20 + 1, set_b=1 << 40),
                   dict(k=129), dict(set_b=2047), dict(cap=-1), dict(cap=2 ** 31), dict(cap=2 ** 40), dict(bytes=23), dict(bytes=-1)):
        a = dict(ok, **change)
        assert None in (a["graph"], a["rows"], a["off"], a["set"], a["scratch"], a["dst"], a["src"]) or \
            ref.refused("edges", a["n"], a["m"], a["k"], a["set_b"], a["bytes"], a["cap"]), change
        assert L.legion_induced_edges(s, a["graph"], a["rows"], a["n"], a["off"], a["m"], a["set"], a["set_b"], a["k"], a["scratch"], a["bytes"],
                                      a["cap"], a["dst"], a["src"], a["eid"]) == -1, change
    ok = dict(dst=P(dst), cap=cap, count=P(count), n=n, ptr=P(ptr))
    for change in (dict(dst=None), dict(count=None), dict(ptr=None), dict(cap=-1), dict(cap=2 ** 31), dict(n=-1), dict(n=2 ** 20 + 1)):
        a = dict(ok, **change)
        assert None in (a["dst"], a["count"], a["ptr"]) or ref.refused("dst_offsets", n=a["n"], cap=a["cap"]), change
        assert L.legion_dst_offsets(s, a["dst"], a["cap"], a["count"], a["n"], a["ptr"]) == -1, change
    assert L.legion_induced_edges(s, g, P(rows), n, P(off), m, P(tab), 2048, k, P(scratch), 24, 0, P(dst), P(src), P(eid)) == 0      # cap == 0
    torch.cuda.synchronize()
    for x in (off, tab, scratch, count, dst, src, eid, ptr):
        assert bool((x == SENTINEL).all()), "a refused call wrote"
    assert L.legion_induced_count(s, g, P(rows), n, P(off), 0, P(tab), 2048, k, P(count), P(scratch), 8) == 0      # m == 0: the two totals only
    torch.cuda.synchronize()
    assert count[0].item() == 0 and count[1].item() == SENTINEL and scratch[0].item() == 0 and bool((scratch[1:] == SENTINEL).all())
