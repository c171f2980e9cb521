"""GraphStorage.labor_edges and the C ABI's legion_labor_count / legion_labor_edges on the GPU, bit for bit against tests/labor_ref.py on
the symmetric graph of tests/node2vec_ref.py (6 000 vertices, 53 448 entries, 30 dead, 6 empty rows, a 4 097-entry hub), with and without
edge ids: every workgroup boundary in the number of rows and every row once, fan-outs 1, 5, 25 and the largest degree, salts 0, 1 and
-1; the hub tiles and the low-degree tiles give strips, waves and whole tiles that keep nothing, a fan-out of the hub's degree gives
tiles that keep all 1 024 slots; capacities at, below and above K; a run of 3 000 seeds without entries between two hubs (the search in
global memory); all seeds empty; the small graphs of link_ref; m below M, ending inside a hub, where the degree stays the row's whole
degree; a scratch that legion_labor_count did not write; another stream, a captured graph, and every refusal of the C ABI over
sentinel-filled buffers.  What makes a wrong kernel fail is asserted from the numpy reference alone before any launch; an input that
fails a condition is replaced, never the condition."""
import ctypes

import numpy as np
import pytest
import torch

from tests import in_edges_ref
from tests import labor_ref as ref
from tests import link_ref, node2vec_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
COUNTS = [1, 63, 64, 65, 256, 257, 1023, 1024, 1025]
MAX_DEGREE = 4097
FANOUTS = [1, 5, 25, MAX_DEGREE]
SALTS = [0, 1, -1]
FIGURES = {(1, 25, 0): 24, (63, 5, 0): 295, (257, 1, -1): 182, (257, 25, 1): 3166, (1025, 5, 0): 5248, (1025, MAX_DEGREE, 0): 839288}
SENTINEL = 0x5A5A5A5A
HUB = 6
N = node2vec_ref.NODE_NUM


def rows_for(n):
    return node2vec_ref.seeds_for(n) if n != "all" else np.arange(N, dtype=np.int32)


def gap_rows():
    """A hub, 3 000 seeds without entries (empty rows, -1, node_num), a hub, then plain rows."""
    none = np.resize(np.array(list(node2vec_ref.EMPTY) + [-1, N], dtype=np.int32), 3000)
    return np.concatenate([[HUB], none, [HUB, 100, 7, 101], none[:1500], [102, 1]]).astype(np.int32)


def empty_rows():
    return np.resize(np.array(list(node2vec_ref.EMPTY) + [-1, N, -5, N + 7], dtype=np.int32), 700)


def tile_counts(kept):
    return np.add.reduceat(kept.astype(np.int64), np.arange(0, kept.size, ref.TILE)) if kept.size else np.zeros(0, np.int64)


def strip_counts(kept):
    pad = np.concatenate([kept, np.zeros(-kept.size % 64, bool)])
    return pad.reshape(-1, 64).sum(axis=1)


def reference(indptr, col, rows, fanout, salt, m=None):
    """(offsets, M or m, kept mask, K, dst, src, eid) of the reference."""
    off = in_edges_ref.row_offsets(indptr, rows)
    m = int(off[-1]) if m is None else m
    kept = ref.slot_mask(indptr, col, rows, off, m, fanout, salt)[0]
    K, dst, src, eid = ref.edges(indptr, col, rows, off, m, fanout, salt)
    assert K == int(kept.sum()) and dst.shape == (K,) and np.all(np.diff(dst) >= 0) and (K == 0 or src.min() >= 0)
    return off, m, kept, K, dst, src, eid


def conditions(indptr, col, rows, fanout, salt):
    """What the rows must hold for a wrong kernel to fail on them; returns reference()."""
    out = reference(indptr, col, rows, fanout, salt)
    off, M, kept, K = out[:4]
    if rows.size >= 63:
        t, s = tile_counts(kept), strip_counts(kept)
        assert (s == 0).sum() >= 1 or fanout == MAX_DEGREE, "a wave that keeps nothing"
        if fanout == 1:
            assert (t == 0).sum() >= 1, "a tile that keeps nothing"
        if fanout == MAX_DEGREE:
            assert (t == ref.TILE).sum() >= 1 and K == int(((out[5] >= 0)).sum()), "a tile that keeps all 1 024 slots"
            live = in_edges_ref.in_edges(indptr, col, rows, off, M)[1] >= 0
            assert np.array_equal(kept, live), "the identity: every live entry"
        else:
            assert 0 < K < M
            wrong = ref.lane_major(out[6], kept)
            assert not np.array_equal(wrong, out[6]), "lane-major ranks differ"
    return out


@pytest.fixture(scope="module")
def world(hip):
    from legion_amd import engine
    indptr, col, _ = node2vec_ref.sym_graph()
    graph = engine.GraphStorage(1, torch.from_numpy(indptr).to(DEV), torch.from_numpy(col).to(DEV))
    yield dict(graph=graph, indptr=indptr, col=col, L=hip)
    torch.cuda.synchronize()
    graph.close()


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def abi(L, graph, rows, off, m, fanout, salt, cap, with_eids=True, stream=None, scratch_fill=None):
    """legion_labor_count + legion_labor_edges over sentinel-filled buffers of cap + 8 entries and a scratch with 8 spare entries: (K
    as _count wrote it, dst, src, eid or None) of cap entries; the tails are checked untouched.  scratch_fill: a value to fill the
    scratch with INSTEAD of calling _count (K is then None)."""
    n = rows.size
    d_rows = torch.from_numpy(np.ascontiguousarray(rows)).to(DEV) if n else torch.zeros(1, dtype=torch.int32, device=DEV)
    d_off = torch.from_numpy(np.ascontiguousarray(off)).to(DEV)
    s = ctypes.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    nbytes = int(L.legion_labor_scratch_bytes(m))
    assert nbytes == ref.scratch_bytes(m) and nbytes % 8 == 0
    scratch = torch.full((nbytes // 8 + 8,), SENTINEL if scratch_fill is None else scratch_fill, dtype=torch.int64, device=DEV)
    count = torch.full((1 + 8,), SENTINEL, dtype=torch.int64, device=DEV)
    if scratch_fill is None:
        assert L.legion_labor_count(s, graph.handle, P(d_rows), n, P(d_off), m, fanout, salt, P(count), P(scratch), nbytes) == 0
    dst = torch.full((cap + 8,), SENTINEL, dtype=torch.int32, device=DEV)
    src = torch.full((cap + 8,), SENTINEL, dtype=torch.int32, device=DEV)
    eid = torch.full((cap + 8,), SENTINEL, dtype=torch.int64, device=DEV) if with_eids else None
    assert L.legion_labor_edges(s, graph.handle, P(d_rows), n, P(d_off), m, fanout, salt, P(scratch), nbytes, cap, P(dst), P(src), P(eid)) == 0
    torch.cuda.synchronize()
    fill = SENTINEL if scratch_fill is None else scratch_fill
    assert bool((scratch[nbytes // 8:] == fill).all()) and bool((count[1:] == SENTINEL).all()), "written past the scratch or the count"
    K = None
    if scratch_fill is None:
        K = int(count[0].item())
        assert int(scratch[ref.tiles_of(m)].item()) == K, "the total in the scratch"
    out = [x.cpu().numpy() if x is not None else None for x in (dst, src, eid)]
    for x in out:
        assert x is None or np.all(x[cap:] == SENTINEL), "written past cap"
    return [K] + [x[:cap] if x is not None else None for x in out]


def same(got, want, what):
    for name, g, w in zip(("dst", "src", "eid"), got, want):
        if g is None:
            continue
        g = g.cpu().numpy() if isinstance(g, torch.Tensor) else g
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, f"{what}: {bad.size} entries of {name} differ, first at {bad[0]}: got {g[bad[0]]} want {w[bad[0]]}"


# ---- the inputs -------------------------------------------------------------------------------------------------------------------
def test_the_inputs_hold_their_conditions_before_any_launch(world):
    indptr, col = world["indptr"], world["col"]
    assert col.size == 53448 and (col < 0).sum() == 30 and np.diff(indptr).max() == MAX_DEGREE == np.diff(indptr)[HUB]
    for (n, fanout, salt), K in FIGURES.items():
        assert conditions(indptr, col, rows_for(n), fanout, salt)[3] == K, (n, fanout, salt)
    for n in (63, 257, "all"):
        for fanout in FANOUTS:
            conditions(indptr, col, rows_for(n), fanout, 0)
    off, M, kept = reference(indptr, col, gap_rows(), 5, 0)[:3]
    spans = in_edges_ref.tile_ranges(off, M)
    assert spans.max() > in_edges_ref.STAGE and (spans > in_edges_ref.STAGE).sum() >= 2 and 0 < kept.sum() < M, "both searches run"
    assert int(in_edges_ref.row_offsets(indptr, empty_rows())[-1]) == 0


# ---- bit for bit ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eids", [False, True], ids=["no-eids", "eids"])
@pytest.mark.parametrize("n", COUNTS + ["all"])
def test_labor_edges_is_the_reference_bit_for_bit(world, n, eids):
    indptr, col, g = world["indptr"], world["col"], world["graph"]
    rows = rows_for(n)
    d_rows = torch.from_numpy(rows).to(DEV)
    for fanout in FANOUTS:
        for salt in SALTS:
            off, M, kept, K, dst, src, eid = conditions(indptr, col, rows, fanout, salt) if salt == 0 else reference(indptr, col, rows, fanout, salt)
            got = g.labor_edges(d_rows if salt else rows, fanout, salt=salt, return_eids=eids)       # rows from the device and the host
            torch.cuda.synchronize()
            assert len(got) == (3 if eids else 2) and all(x.is_cuda for x in got)
            same(got, (dst, src, eid), f"n {n} fanout {fanout} salt {salt}")
            if salt == 0:
                k, *out = abi(world["L"], g, rows, off, M, fanout, salt, K, eids)
                assert k == K
                same(out, (dst, src, eid), f"abi: n {n} fanout {fanout}")


@pytest.mark.parametrize("eids", [False, True], ids=["no-eids", "eids"])
def test_cap_is_a_capacity(world, eids):
    indptr, col = world["indptr"], world["col"]
    rows = rows_for(257)
    off, M, kept, K = conditions(indptr, col, rows, 25, 1)[:4]
    assert K == FIGURES[(257, 25, 1)] > ref.TILE
    for cap in (K, K - 1, K + 1000, 1):
        want = ref.edges(indptr, col, rows, off, M, 25, 1, cap=cap)
        assert cap <= K or all(np.all(w[K:] == -1) for w in want[1:])
        k, *out = abi(world["L"], world["graph"], rows, off, M, 25, 1, cap, eids)
        assert k == K, "the count does not depend on cap"
        same(out, want[1:], f"cap {cap}")


def test_a_run_of_seeds_without_entries_takes_the_search_in_global_memory(world):
    indptr, col = world["indptr"], world["col"]
    rows = gap_rows()
    for fanout in (5, MAX_DEGREE):
        off, M, kept, K, dst, src, eid = reference(indptr, col, rows, fanout, 0)
        assert in_edges_ref.tile_ranges(off, M).max() > in_edges_ref.STAGE and K > 0
        got = world["graph"].labor_edges(rows, fanout, return_eids=True)
        torch.cuda.synchronize()
        same(got, (dst, src, eid), f"gap, fanout {fanout}")
    assert set(np.unique(dst).tolist()) == set(np.nonzero(np.diff(off) > 0)[0].tolist()), "no seed with entries is skipped"


def test_all_seeds_empty(world):
    rows = empty_rows()
    got = world["graph"].labor_edges(rows, 5, return_eids=True)
    torch.cuda.synchronize()
    assert all(x.shape == (0,) for x in got) and [x.dtype for x in got] == [torch.int32, torch.int32, torch.int64]
    off = np.zeros(rows.size + 1, np.int64)
    k, dst, src, eid = abi(world["L"], world["graph"], rows, off, 0, 5, 0, 1500)          # M = 0: a zero total, the fill only
    assert k == 0 and np.all(dst == -1) and np.all(src == -1) and np.all(eid == -1)
    k, dst, src, eid = abi(world["L"], world["graph"], rows, off, 1500, 5, 0, 700)        # slots that resolve to no row
    assert k == 0 and np.all(dst == -1) and np.all(src == -1) and np.all(eid == -1)
    k, dst, src, eid = abi(world["L"], world["graph"], np.zeros(0, np.int32), np.zeros(1, np.int64), 0, 5, 0, 8)      # n == 0: the same
    assert k == 0 and np.all(dst == -1) and np.all(src == -1) and np.all(eid == -1)
    none = world["graph"].labor_edges(np.zeros(0, np.int32), 3, return_eids=True)
    assert all(x.shape == (0,) for x in none)


def small_cases():
    g = dict(link_ref.small_graphs())
    g["complete"] = link_ref.complete_graph(8)
    g["ring"] = link_ref.ring_graph(8)
    return g


def small_rows(indptr):
    """Every row from -1 to N, then every row again backwards."""
    n = indptr.size - 1
    return np.concatenate([np.arange(-1, n + 1), np.arange(n)[::-1]]).astype(np.int32)


@pytest.mark.parametrize("name", sorted(small_cases()))
def test_small_graphs(hip, name):
    from legion_amd import engine
    indptr, col = small_cases()[name]
    rows = small_rows(indptr)
    g = engine.GraphStorage(1, torch.from_numpy(indptr).to(DEV), torch.from_numpy(col).to(DEV))
    try:
        for fanout in (1, 2, 3, 40):
            for salt in (0, 7):
                want = ref.edges_full(indptr, col, rows, fanout, salt)
                got = g.labor_edges(rows, fanout, salt=salt, return_eids=True)
                torch.cuda.synchronize()
                same(got, want, f"{name} fanout {fanout} salt {salt}")
        assert want[0].size == 2 * int((col >= 0).sum()), "fanout 40, the largest degree among these graphs, keeps every live entry"
    finally:
        torch.cuda.synchronize()
        g.close()


def prefix_case(indptr, col):
    """m below M, ending inside the second copy of the hub and inside a tile; fan-out 2 000: with the hub's whole degree near half of
    the slots are kept, with the slots below m as the degree all of them."""
    rows = rows_for(257)
    off = in_edges_ref.row_offsets(indptr, rows)
    hub_at = int(np.nonzero(rows == HUB)[0][1])
    m = int(off[hub_at]) + 2000
    assert off[hub_at] < m < off[hub_at + 1] and m % ref.TILE != 0
    want = ref.edges(indptr, col, rows, off, m, 2000, 3)
    wrong = ref.edges(indptr, col, rows, off, m, 2000, 3, **ref.WRONG["degree-below-m"])
    assert wrong[0] >= want[0] + 500, "d as the slots below m keeps the whole prefix of the hub"
    return rows, off, m, want


def test_m_below_M_keeps_the_rows_whole_degree(world):
    rows, off, m, want = prefix_case(world["indptr"], world["col"])
    k, *out = abi(world["L"], world["graph"], rows, off, m, 2000, 3, want[0] + 10)
    assert k == want[0]
    same(out, ref.edges(world["indptr"], world["col"], rows, off, m, 2000, 3, cap=want[0] + 10)[1:], "a prefix")


@pytest.mark.parametrize("fill", [0, 2 ** 40, -1], ids=["zero", "2^40", "minus-one"])
def test_a_scratch_that_count_did_not_write(world, fill):
    """Only [0, cap) is written, whatever the scratch holds: the tails of abi() are checked.  The values are unspecified, but each is
    one the kernel writes: all bases 0 or -1 put every tile's triples over the fill of the whole buffer; all bases 2^40 drop every triple
    and clamp the fill to nothing."""
    indptr, col = world["indptr"], world["col"]
    rows = rows_for(257)
    off, M, kept, K, dst, src, eid = reference(indptr, col, rows, 25, 1)
    for cap in (K, 100):
        _, d, s, e = abi(world["L"], world["graph"], rows, off, M, 25, 1, cap, scratch_fill=fill)
        if fill == 2 ** 40:
            assert np.all(d == SENTINEL) and np.all(s == SENTINEL) and np.all(e == SENTINEL), "every triple dropped, the fill clamped to [cap, cap)"
        else:
            assert np.all((d == -1) | ((d >= 0) & (d < rows.size))) and np.all((e == -1) | ((e >= 0) & (e < col.size)))
            assert np.all((s == -1) | ((s >= 0) & (s < N)))


# ---- streams and graphs ---------------------------------------------------------------------------------------------------------------
def test_another_stream_and_a_captured_graph(world):
    indptr, col, L, g = world["indptr"], world["col"], world["L"], world["graph"]
    rows = rows_for(1025)
    off, M, kept, K, dst, src, eid = reference(indptr, col, rows, 5, 0)
    assert K == FIGURES[(1025, 5, 0)]
    d_rows = torch.from_numpy(rows).to(DEV)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    assert s != torch.cuda.current_stream()
    got = g.labor_edges(d_rows, 5, return_eids=True, stream=s)
    s.synchronize()
    same(got, (dst, src, eid), "another stream")

    n, cap = rows.size, K + 500
    nbytes = int(L.legion_labor_scratch_bytes(M))
    scratch = torch.zeros(nbytes // 8, dtype=torch.int64, device=DEV)
    d_off = torch.from_numpy(off).to(DEV)
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    o_dst, o_src = (torch.zeros(cap, dtype=torch.int32, device=DEV) for _ in range(2))
    o_eid = torch.zeros(cap, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cs = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = [L.legion_labor_count(cs, g.handle, P(d_rows), n, P(d_off), M, 5, 0, P(count), P(scratch), nbytes),
              L.legion_labor_edges(cs, g.handle, P(d_rows), n, P(d_off), M, 5, 0, P(scratch), nbytes, cap, P(o_dst), P(o_src), P(o_eid))]
    assert rc == [0, 0]
    capped = ref.edges(indptr, col, rows, off, M, 5, 0, cap=cap)[1:]
    for _ in range(2):
        for x in (count, scratch, o_dst, o_src, o_eid):
            x.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        assert int(count.item()) == K
        same((o_dst, o_src, o_eid), capped, "captured")


# ---- the C ABI's refusals -----------------------------------------------------------------------------------------------------------
def test_c_abi_refusals_leave_the_outputs_untouched(world):
    L, g = world["L"], world["graph"].handle
    n, m, cap = 8, 64, 64
    rows = torch.from_numpy(rows_for(n)).to(DEV)
    off = torch.full((n + 1,), SENTINEL, dtype=torch.int64, device=DEV)
    scratch = torch.full((4,), SENTINEL, dtype=torch.int64, device=DEV)
    count = torch.full((2,), SENTINEL, dtype=torch.int64, device=DEV)
    dst, src = (torch.full((cap,), SENTINEL, dtype=torch.int32, device=DEV) for _ in range(2))
    eid = torch.full((cap,), SENTINEL, dtype=torch.int64, device=DEV)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.legion_labor_scratch_bytes(m) == 24 == ref.scratch_bytes(m)
    for bad_m in (-1, 2 ** 30 + 1):
        assert L.legion_labor_scratch_bytes(bad_m) == -1 == ref.scratch_bytes(bad_m)
    ok = dict(graph=g, rows=P(rows), n=n, off=P(off), m=m, fanout=5, salt=0, count=P(count), scratch=P(scratch), bytes=24)
    for change in (dict(graph=None), dict(rows=None), dict(off=None), dict(count=None), dict(scratch=None), dict(n=-1), dict(n=2 ** 20 + 1),
                   dict(m=-1), dict(m=2 ** 30 + 1, bytes=1 << 40), dict(m=2 ** 40, bytes=1 << 40), dict(fanout=0), dict(fanout=-3),
                   dict(bytes=23), dict(bytes=0), dict(bytes=-1), dict(m=1025)):
        a = dict(ok, **change)
        assert None in (a["graph"], a["rows"], a["off"], a["count"], a["scratch"]) or \
            ref.refused("count", a["n"], a["m"], a["fanout"], scratch=a["bytes"]), change
        assert L.legion_labor_count(s, a["graph"], a["rows"], a["n"], a["off"], a["m"], a["fanout"], a["salt"], a["count"], a["scratch"],
                                    a["bytes"]) == -1, change
    ok = dict(graph=g, rows=P(rows), n=n, off=P(off), m=m, fanout=5, salt=0, scratch=P(scratch), bytes=24, cap=cap, dst=P(dst), src=P(src),
              eid=P(eid))
    for change in (dict(graph=None), dict(rows=None), dict(off=None), dict(scratch=None), dict(dst=None), dict(src=None), dict(n=-1),
                   dict(n=2 ** 20 + 1), dict(m=-1), dict(m=2 ** 30 + 1, bytes=1 << 40), dict(fanout=0), dict(cap=-1), dict(cap=2 ** 31),
                   dict(cap=2 ** 40), dict(bytes=23), dict(bytes=-1)):
        a = dict(ok, **change)
        assert None in (a["graph"], a["rows"], a["off"], a["scratch"], a["dst"], a["src"]) or \
            ref.refused("edges", a["n"], a["m"], a["fanout"], scratch=a["bytes"], cap=a["cap"]), change
        assert L.legion_labor_edges(s, a["graph"], a["rows"], a["n"], a["off"], a["m"], a["fanout"], a["salt"], a["scratch"], a["bytes"],
                                    a["cap"], a["dst"], a["src"], a["eid"]) == -1, change
    assert L.legion_labor_edges(s, g, P(rows), n, P(off), m, 5, 0, P(scratch), 24, 0, P(dst), P(src), P(eid)) == 0      # cap == 0: nothing runs
    torch.cuda.synchronize()
    for x in (off, scratch, count, dst, src, eid):
        assert bool((x == SENTINEL).all()), "a refused call wrote"
    assert L.legion_labor_count(s, g, P(rows), n, P(off), 0, 5, 0, P(count), P(scratch), 8) == 0          # m == 0: the two totals only
    torch.cuda.synchronize()
    assert count[0].item() == 0 and count[1].item() == SENTINEL and scratch[0].item() == 0 and bool((scratch[1:] == SENTINEL).all())
