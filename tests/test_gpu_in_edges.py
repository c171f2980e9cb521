"""GraphStorage.row_offsets / in_edges and the C ABI's legion_row_offsets / legion_in_edges on the GPU, bit for bit against
tests/in_edges_ref.py on the symmetric graph of tests/node2vec_ref.py (6 000 vertices, 53 448 entries, 30 dead, 6 empty rows, a
4 097-entry hub), with and without edge ids: every workgroup boundary in the number of rows, every row once, capacities at, below and
above M and a prefix that ends inside the hub, a run of 3 000 seeds without entries between two hubs (the tile's range exceeds the LDS
staging: the search in global memory runs), all seeds empty, the small graphs of link_ref, offsets that are wrong on purpose (the guards
of rule 4 are plain comparisons: nothing is read outside the arrays whatever offsets holds), another stream, a captured graph, and every
refusal of the C ABI over sentinel-filled buffers.  What makes a wrong kernel fail is asserted from the numpy reference alone before any
launch; an input that fails a condition is replaced, never the condition."""
import ctypes

import numpy as np
import pytest
import torch

from tests import in_edges_ref as ref
from tests import link_ref, node2vec_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
COUNTS = [1, 63, 64, 65, 256, 257, 1023, 1024, 1025]
FIGURES = {1: 4097, 63: 46432, 64: 42351, 65: 46448, 257: 207475}      # n -> M of seeds_for(n)
SENTINEL = 0x5A5A5A5A
HUB = 6
N = node2vec_ref.NODE_NUM


def rows_for(n):
    return node2vec_ref.seeds_for(n) if n != "all" else np.arange(N, dtype=np.int32)


def conditions(indptr, col, rows):
    """What the rows must hold for a wrong kernel to fail on them; returns the reference (offsets, dst, src, eid)."""
    want = ref.in_edges_full(indptr, col, rows)
    M = int(want[0][-1])
    deg = ref.degrees(indptr, rows)
    if rows.size >= 63:
        inside = (rows >= 0) & (rows < N)
        assert (~inside).sum() == 2 or rows.size == N, "a -1 and a node_num"
        assert ((deg == 0) & inside).sum() >= 1 and (rows == HUB).sum() >= 1, "an empty row and the hub"
        wrong = ref.in_edges_lower_bound(indptr, col, rows, want[0], M)
        assert (wrong[0] != want[1]).sum() >= 1, "a lower bound names an empty row somewhere"
        assert (want[2] < 0).sum() >= 1, "a dead entry"
    return want


def gap_rows():
    """A hub, 3 000 seeds without entries (empty rows, -1, node_num), a hub, then plain rows."""
    none = np.resize(np.array(list(node2vec_ref.EMPTY) + [-1, N], dtype=np.int32), 3000)
    return np.concatenate([[HUB], none, [HUB, 100, 7, 101], none[:1500], [102, 1]]).astype(np.int32)


def empty_rows():
    return np.resize(np.array(list(node2vec_ref.EMPTY) + [-1, N, -5, N + 7], dtype=np.int32), 700)


def bad_offsets(indptr, rows):
    """name -> (offsets, exact): offsets that are wrong on purpose.  exact: non-decreasing, or such that every probe of a binary search
    answers alike, so the reference applies as it stands; else only rule 4's either-or is specified."""
    good = ref.row_offsets(indptr, rows)
    n = rows.size
    over = good.copy()
    k = int(np.nonzero(np.diff(good) > 0)[0][3])                      # the fourth row with entries: its span one longer
    over[k + 1:] += 1
    return {"all-zero": (np.zeros(n + 1, np.int64), True), "all-2^40": (np.full(n + 1, 2 ** 40, np.int64), True),
            "span-overstated": (over, True), "decreasing-high": (2 ** 40 - np.arange(n + 1, dtype=np.int64), True),
            "decreasing-negative": (-1 - np.arange(n + 1, dtype=np.int64), True),
            "reversed": (good[::-1].copy(), False), "shuffled": (np.random.RandomState(3).permutation(good), False),
            "extremes": (np.where(np.arange(n + 1) % 2 == 0, np.int64(-2 ** 63), np.int64(2 ** 63 - 1)), False)}


def want_bad(indptr, col, rows, offsets, m):
    """The reference for offsets marked exact: a binary search over them finds what counting finds."""
    p = np.arange(m, dtype=np.int64)
    i = (offsets[None, :] <= p[:, None]).sum(axis=1) - 1 if not np.all(np.diff(offsets) >= 0) else \
        np.searchsorted(offsets, p, side="right") - 1
    return ref._expand(indptr, col, rows, offsets, m, i)


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


def abi(L, graph, rows, offsets, m, with_eids=True, stream=None):
    """legion_in_edges over buffers of m + 8 entries filled with a sentinel: (dst, src, eid or None) of m entries; the tail is checked
    untouched.  offsets: a numpy array, or None for legion_row_offsets' own (returned too)."""
    n = rows.size
    d_rows = torch.from_numpy(np.ascontiguousarray(rows)).to(DEV) if n else torch.zeros(1, dtype=torch.int32, device=DEV)
    s = ctypes.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    if offsets is None:
        d_off = torch.full((n + 1,), SENTINEL, dtype=torch.int64, device=DEV)
        nbytes = int(L.legion_row_offsets_scratch_bytes(n))
        scratch = torch.zeros(nbytes // 8 + 1, dtype=torch.int64, device=DEV)
        assert L.legion_row_offsets(s, graph.handle, P(d_rows), n, P(d_off), P(scratch), nbytes) == 0
    else:
        d_off = torch.from_numpy(np.ascontiguousarray(offsets)).to(DEV)
    dst = torch.full((m + 8,), SENTINEL, dtype=torch.int32, device=DEV)
    src = torch.full((m + 8,), SENTINEL, dtype=torch.int32, device=DEV)
    eid = torch.full((m + 8,), SENTINEL, dtype=torch.int64, device=DEV) if with_eids else None
    assert L.legion_in_edges(s, graph.handle, P(d_rows), n, P(d_off), m, P(dst), P(src), P(eid)) == 0
    torch.cuda.synchronize()
    out = [x.cpu().numpy() if x is not None else None for x in (dst, src, eid)]
    for x in out:
        assert x is None or np.all(x[m:] == SENTINEL), "written past m"
    return [x[:m] if x is not None else None for x in out] + [d_off.cpu().numpy()]


def same(got, want, what):
    for name, g, w in zip(("dst", "src", "eid"), got, want):
        if g is None:
            continue
        g = g.cpu().numpy() if isinstance(g, torch.Tensor) else g
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, f"{what}: {bad.size} slots of {name} differ, first at {bad[0]}: got {g[bad[0]]} want {w[bad[0]]}"


# ---- the inputs -------------------------------------------------------------------------------------------------------------------
def test_the_inputs_hold_their_conditions_before_any_launch(world):
    indptr, col = world["indptr"], world["col"]
    assert col.size == 53448 and (col < 0).sum() == 30 and (np.diff(indptr) == 0).sum() == 6 and np.diff(indptr)[HUB] == 4097
    for n in COUNTS + ["all"]:
        want = conditions(indptr, col, rows_for(n))
        if n in FIGURES:
            assert int(want[0][-1]) == FIGURES[n], (n, int(want[0][-1]))
    assert int(conditions(indptr, col, rows_for("all"))[0][-1]) == 53448
    rows = gap_rows()
    off = ref.row_offsets(indptr, rows)
    spans = ref.tile_ranges(off, int(off[-1]))
    assert spans.max() > ref.STAGE and spans.min() <= ref.STAGE and (spans > ref.STAGE).sum() >= 2, "both searches run"
    assert int(ref.row_offsets(indptr, empty_rows())[-1]) == 0
    for name, (offsets, exact) in bad_offsets(indptr, rows_for(257)).items():
        assert offsets.size == 258 and (exact or np.any(np.diff(offsets) < 0)), name


# ---- bit for bit ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eids", [False, True], ids=["no-eids", "eids"])
@pytest.mark.parametrize("n", COUNTS + ["all"])
def test_in_edges_is_the_reference_bit_for_bit(world, n, eids):
    rows = rows_for(n)
    want = conditions(world["indptr"], world["col"], rows)
    got = world["graph"].in_edges(torch.from_numpy(rows).to(DEV), return_eids=eids)
    host = world["graph"].in_edges(rows, return_eids=eids)             # rows from the host
    alone = world["graph"].row_offsets(rows)
    torch.cuda.synchronize()
    assert len(got) == (4 if eids else 3) and got[0].dtype == torch.int64 and got[0].shape == (rows.size + 1,)
    for o in (got[0], host[0], alone):
        assert np.array_equal(o.cpu().numpy(), want[0]), f"n {n}: offsets"
    same(got[1:], want[1:], f"n {n}")
    same(host[1:], want[1:], f"n {n}, rows from the host")


@pytest.mark.parametrize("eids", [False, True], ids=["no-eids", "eids"])
def test_m_is_a_capacity(world, eids):
    indptr, col = world["indptr"], world["col"]
    rows = rows_for(257)
    off = ref.row_offsets(indptr, rows)
    M = int(off[-1])
    hub_at = int(np.nonzero(rows == HUB)[0][1])
    inside = int(off[hub_at]) + 2000
    assert off[hub_at] < inside < off[hub_at + 1] and inside % ref.TILE != 0
    for m in (M, M - 1, M + 1000, 1, inside):
        want = ref.in_edges(indptr, col, rows, off, m)
        assert m <= M or (np.all(want[0][M:] == -1) and np.all(want[2][M:] == -1))
        got = abi(world["L"], world["graph"], rows, None, m, eids)
        assert np.array_equal(got[3], off)
        same(got[:3], want, f"m {m}")


def test_a_run_of_seeds_without_entries_takes_the_search_in_global_memory(world):
    indptr, col = world["indptr"], world["col"]
    rows = gap_rows()
    want = ref.in_edges_full(indptr, col, rows)
    assert ref.tile_ranges(want[0], int(want[0][-1])).max() > ref.STAGE
    got = world["graph"].in_edges(rows, return_eids=True)
    torch.cuda.synchronize()
    assert np.array_equal(got[0].cpu().numpy(), want[0])
    same(got[1:], want[1:], "gap")
    assert set(np.unique(want[1]).tolist()) == set(np.nonzero(np.diff(want[0]) > 0)[0].tolist()), "no seed with entries is skipped"


def test_all_seeds_empty(world):
    rows = empty_rows()
    got = world["graph"].in_edges(rows, return_eids=True)
    torch.cuda.synchronize()
    assert np.all(got[0].cpu().numpy() == 0) and all(x.shape == (0,) for x in got[1:])
    dst, src, eid, off = abi(world["L"], world["graph"], rows, None, 1500)
    assert np.all(off == 0) and np.all(dst == -1) and np.all(src == -1) and np.all(eid == -1)
    none = world["graph"].in_edges(np.zeros(0, np.int32), return_eids=True)
    assert none[0].cpu().tolist() == [0] and all(x.shape == (0,) for x in none[1:])
    assert world["graph"].row_offsets(np.zeros(0, np.int32)).cpu().tolist() == [0]


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
    want = ref.in_edges_full(indptr, col, rows)
    assert int(want[0][-1]) == 2 * col.size and (name != "loop" or indptr.size == 2)
    g = engine.GraphStorage(1, torch.from_numpy(indptr).to(DEV), torch.from_numpy(col).to(DEV))
    try:
        got = g.in_edges(rows, return_eids=True)
        torch.cuda.synchronize()
        assert np.array_equal(got[0].cpu().numpy(), want[0])
        same(got[1:], want[1:], name)
    finally:
        torch.cuda.synchronize()
        g.close()


# ---- offsets that are wrong on purpose ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["all-zero", "all-2^40", "span-overstated", "decreasing-high", "decreasing-negative", "reversed",
                                  "shuffled", "extremes"])
def test_wrong_offsets_are_guarded_by_rule_4(world, name):
    indptr, col = world["indptr"], world["col"]
    rows = rows_for(257)
    offsets, exact = bad_offsets(indptr, rows)[name]
    m = FIGURES[257] + 100
    dst, src, eid, _ = abi(world["L"], world["graph"], rows, offsets, m)
    assert ref.consistent(indptr, col, rows, offsets, dst, src, eid), name
    if exact:
        want = want_bad(indptr, col, rows, offsets, m) if name.startswith("decreasing") else ref.in_edges(indptr, col, rows, offsets, m)
        same((dst, src, eid), want, name)
        if name == "span-overstated":
            good = ref.in_edges(indptr, col, rows, ref.row_offsets(indptr, rows), m)
            assert (want[2] != good[2]).sum() >= 1000 and (want[0][:m - 100] == -1).sum() == 1, "one slot past a row's end, the rest shifted"
    else:
        print(f"{name}: {(dst >= 0).sum()} of {m} slots name an entry")


# ---- streams and graphs ---------------------------------------------------------------------------------------------------------------
def test_another_stream_and_a_captured_graph(world):
    indptr, col, L, g = world["indptr"], world["col"], world["L"], world["graph"]
    rows = rows_for(1025)
    want = ref.in_edges_full(indptr, col, rows)
    M = int(want[0][-1])
    d_rows = torch.from_numpy(rows).to(DEV)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    assert s != torch.cuda.current_stream()
    off = g.row_offsets(d_rows, stream=s)
    got = g.in_edges(d_rows, return_eids=True, stream=s)
    s.synchronize()
    assert np.array_equal(off.cpu().numpy(), want[0]) and np.array_equal(got[0].cpu().numpy(), want[0])
    same(got[1:], want[1:], "another stream")

    n, m = rows.size, M + 500
    nbytes = int(L.legion_row_offsets_scratch_bytes(n))
    scratch = torch.zeros(nbytes // 8, dtype=torch.int64, device=DEV)
    d_off = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    dst, src = (torch.zeros(m, dtype=torch.int32, device=DEV) for _ in range(2))
    eid = torch.zeros(m, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cs = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = [L.legion_row_offsets(cs, g.handle, P(d_rows), n, P(d_off), P(scratch), nbytes),
              L.legion_in_edges(cs, g.handle, P(d_rows), n, P(d_off), m, P(dst), P(src), P(eid))]
    assert rc == [0, 0]
    capped = ref.in_edges(indptr, col, rows, want[0], m)
    for _ in range(2):
        for x in (d_off, dst, src, eid):
            x.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(d_off.cpu().numpy(), want[0])
        same((dst, src, eid), capped, "captured")


# ---- the C ABI's refusals -----------------------------------------------------------------------------------------------------------
def test_c_abi_refusals_leave_the_outputs_untouched(world):
    L, g = world["L"], world["graph"].handle
    n, m = 8, 64
    rows = torch.from_numpy(rows_for(n)).to(DEV)
    off = torch.full((n + 1,), SENTINEL, dtype=torch.int64, device=DEV)
    scratch = torch.full((4,), SENTINEL, dtype=torch.int64, device=DEV)
    dst, src = (torch.full((m,), SENTINEL, dtype=torch.int32, device=DEV) for _ in range(2))
    eid = torch.full((m,), SENTINEL, dtype=torch.int64, device=DEV)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.legion_row_offsets_scratch_bytes(n) == 8 == ref.scratch_bytes(n)
    ok = dict(graph=g, rows=P(rows), n=n, off=P(off), scratch=P(scratch), bytes=8)
    for change in (dict(graph=None), dict(rows=None), dict(off=None), dict(scratch=None), dict(n=-1), dict(n=2 ** 20 + 1, bytes=1 << 40),
                   dict(bytes=7), dict(bytes=0), dict(bytes=-1)):
        a = dict(ok, **change)
        assert None in (a["graph"], a["rows"], a["off"], a["scratch"]) or ref.refused("row_offsets", a["n"], scratch=a["bytes"]), change
        assert L.legion_row_offsets(s, a["graph"], a["rows"], a["n"], a["off"], a["scratch"], a["bytes"]) == -1, change
    ok = dict(graph=g, rows=P(rows), n=n, off=P(off), m=m, dst=P(dst), src=P(src), eid=P(eid))
    for change in (dict(graph=None), dict(rows=None), dict(off=None), dict(dst=None), dict(src=None), dict(n=-1), dict(n=2 ** 20 + 1),
                   dict(m=-1), dict(m=2 ** 31), dict(m=2 ** 40)):
        a = dict(ok, **change)
        assert None in (a["graph"], a["rows"], a["off"], a["dst"], a["src"]) or ref.refused("in_edges", a["n"], m=a["m"]), change
        assert L.legion_in_edges(s, a["graph"], a["rows"], a["n"], a["off"], a["m"], a["dst"], a["src"], a["eid"]) == -1, change
    assert L.legion_in_edges(s, g, P(rows), n, P(off), 0, P(dst), P(src), P(eid)) == 0      # no slots: nothing runs
    torch.cuda.synchronize()
    for x in (off, scratch, dst, src, eid):
        assert bool((x == SENTINEL).all()), "a refused call wrote"
    assert L.legion_row_offsets(s, g, P(rows), 0, P(off), P(scratch), 0) == 0               # no rows: offsets[0] = 0 only
    torch.cuda.synchronize()
    assert off[0].item() == 0 and bool((off[1:] == SENTINEL).all()) and bool((scratch == SENTINEL).all())
