"""Temporal neighbour sampling on the GPU (legion_graph_set_edge_times, legion_temporal_sample_count, legion_temporal_sample_edges and
the Python ops over them), bit for bit against tests/temporal_ref.py, on one hand-made graph: row degrees around a wave, around 4 096 and
a hub of 70 001 (three rounds of the 64-ary search); times that step by 3 000 000 001 from negative values to far above 2^32, so that a
compare of the low words alone fails, with a run of three equal stamps in every sixteen entries; a row of INT64_MIN and INT64_MAX - 1.
A row is listed once per CUT, the number of candidates its bound leaves.  Three graphs: `sorted`; `forced`, the same arrays with one
swapped pair of times in a row that is never sampled, which sends the sorted graph through the scan kernels; `scan`, col and time
permuted together inside every row.  What makes a wrong kernel fail is asserted from the reference before any launch."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import far_rows
from tests import temporal_ref as ref
from tests.compare import same_arrays

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 0x5A5A5A5A
MIN64, MAX64 = -2 ** 63, 2 ** 63 - 1
STEP = 3_000_000_001
DEGREES = [0, 1, 2, 63, 64, 65, 4095, 4096, 4097, 70001, 2, 2]
EXTREME, SPARE, HUB, N = 10, 11, 9, len(DEGREES)                    # the row of INT64_MIN and INT64_MAX - 1; the row no test samples
# row -> the cuts its bounds are chosen for: 0 and D; a first-round probe (5 * 64, 3 * 65, 3 * 1094) and either side of it; 63, 64, 65;
# 16 m + 9 and 16 m + 12, either end of a run of equal times; C - f in {-1, 0, 1} for f in {1, 5, 64} on the row of 65
CUTS = {0: [0], 1: [0, 1], 2: [0, 1, 2], 3: [0, 25, 28, 62, 63], 4: [0, 63, 64], 5: [0, 1, 2, 4, 5, 6, 63, 64, 65], 6: [0, 319, 320, 321, 4094, 4095],
        7: [319, 320, 321, 63, 64, 65, 169, 172, 4096], 8: [0, 194, 195, 196, 4097], HUB: [0, 3281, 3282, 3283, 16009, 16012, 35000, 69999, 70001]}
NAMES = ("dst", "src", "eid", "time")
FANOUTS = (1, 5, 64, -1)
CASES = ([(g, ref.UNIFORM, f, rep) for g in ("sorted", "forced", "scan") for f in FANOUTS for rep in (0, 1)]
         + [("sorted", ref.LAST, f, 0) for f in FANOUTS])


def stamp(d, p):
    """The time of position p of a row of d entries: positions 16 m + 9 .. 16 m + 11 share one stamp."""
    p = np.asarray(p, dtype=np.int64)
    return (np.where((p % 16 == 10) | (p % 16 == 11), p - p % 16 + 9, p) - d // 2) * STEP


@functools.lru_cache(maxsize=None)
def hand_graph(which="sorted"):
    rng = np.random.RandomState(11)
    indptr = np.concatenate([[0], np.cumsum(DEGREES)]).astype(np.int64)
    col = rng.randint(0, N, int(indptr[-1])).astype(np.int32)
    col[rng.rand(col.size) < 0.03] = -1
    time = np.concatenate([stamp(d, np.arange(d)) for d in DEGREES]).astype(np.int64)
    time[indptr[EXTREME]:indptr[EXTREME + 1]] = [MIN64, MAX64 - 1]
    time[indptr[SPARE]:indptr[SPARE + 1]] = [5, 9]
    if which == "forced":
        time[indptr[SPARE]:indptr[SPARE + 1]] = [9, 5]
    if which == "scan":
        order = np.concatenate([indptr[r] + rng.permutation(d) for r, d in enumerate(DEGREES)])
        col, time = col[order], time[order]
    return indptr, col, time


@functools.lru_cache(maxsize=None)
def row_list():
    """(rows, bounds, cuts): a row per cut, the extreme bounds, rows outside the graph, and one (row, bound) pair twice."""
    rows, bounds = [], []
    for r, cuts in CUTS.items():
        d = DEGREES[r]
        for c in cuts:
            rows.append(r)
            bounds.append(int(stamp(d, c)) if c < d else int(stamp(d, d - 1)) + 1 if d else 5)
    rows += [EXTREME, EXTREME, EXTREME, 4, 4, 7, 7, -1, N, HUB]
    bounds += [MIN64, 0, MAX64, MIN64, MAX64, int(stamp(4096, 169)) + 1, int(stamp(4096, 169)), 7, 7, int(stamp(70001, 3282))]
    cuts = sum(CUTS.values(), []) + [0, 1, 2, 0, 64, 172, 169, 0, 0, 3282]
    return np.array(rows, dtype=np.int32), np.array(bounds, dtype=np.int64), np.array(cuts, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def want(which, strategy, fanout, replace):
    """The forced graph's reference is the sorted graph's: one rule for both classes."""
    rows, bounds, _ = row_list()
    return ref.sample(*hand_graph("scan" if which == "scan" else "sorted"), rows, bounds, fanout, strategy, replace, 3)


@pytest.fixture(scope="module")
def world(hip):
    from legion_amd import engine
    out = dict(L=hip)
    for which in ("sorted", "forced", "scan"):
        indptr, col, time = (torch.from_numpy(x).to(DEV) for x in hand_graph(which))
        out[which] = engine.GraphStorage(1, indptr, col)
        out[which].set_edge_times(time)
    yield out
    torch.cuda.synchronize()
    for which in ("sorted", "forced", "scan"):
        out[which].close()


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def abi(world, which, rows, bounds, fanout, strategy, replace, salt, w, cap, ids=True, stream=None):
    """count, then edges over sentinel-filled buffers with 8 spare entries, against the reference's w: cand and the offsets; [0, min(M,
    cap)) the picks; [M, cap) -1; nothing past cap, cand, the offsets and the scratch."""
    L, g, n = world["L"], world[which], rows.size
    d_rows = torch.from_numpy(rows).to(DEV) if n else torch.zeros(1, dtype=torch.int32, device=DEV)
    d_bounds = torch.from_numpy(bounds).to(DEV) if n else torch.zeros(1, dtype=torch.int64, device=DEV)
    s = ctypes.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    nbytes = int(L.legion_temporal_sample_scratch_bytes(n))
    assert nbytes == 8 * ((n + 255) // 256)
    full = lambda size, dtype: torch.full((size + 8,), SENTINEL, dtype=dtype, device=DEV)
    scratch, cand, offsets = full(nbytes // 8, torch.int64), full(n, torch.int64), full(n + 1, torch.int64)
    out = [full(cap, torch.int32), full(cap, torch.int32), full(cap, torch.int64) if ids else None, full(cap, torch.int64) if ids else None]
    head = (s, g.handle, P(d_rows), P(d_bounds), n, fanout, strategy, replace)
    assert L.legion_temporal_sample_count(*head, P(cand), P(offsets), P(scratch), nbytes) == 0
    assert L.legion_temporal_sample_edges(*head, salt, P(cand), P(offsets), cap, *[P(x) for x in out]) == 0
    torch.cuda.synchronize()
    M = w[2].size
    pad = np.full(8, SENTINEL)
    same_arrays([cand, offsets], [np.concatenate([w[0], pad]), np.concatenate([w[1], pad])], which, names=["cand", "offsets"])
    assert bool((scratch[nbytes // 8:] == SENTINEL).all()), "written past the scratch"
    for name, x, ref_x in zip(NAMES, out, w[2:]):
        if x is not None:
            tail = np.concatenate([np.full(max(cap - M, 0), -1), pad]).astype(ref_x.dtype)
            same_arrays(x, np.concatenate([ref_x[:cap], tail]), f"{which} cap {cap} of {M}", names=[name])


def test_the_inputs_hold_their_conditions_before_any_launch():
    rows, bounds, cuts = row_list()
    for which in ("sorted", "forced", "scan"):
        indptr, col, time = hand_graph(which)
        inside = np.ones(time.size - 1, dtype=bool)
        inside[indptr[1:-1][(np.diff(indptr)[1:] > 0) & (indptr[1:-1] > 0)] - 1] = False      # pairs across a row's first entry
        descents = int(((time[1:] < time[:-1]) & inside).sum())
        assert (descents == 0) == (which == "sorted") and (which != "forced" or descents == 1)
    indptr, col, time = hand_graph()
    assert SPARE not in rows and np.array_equal(ref.degrees(indptr, time, rows, bounds), cuts), "every bound cuts where it is meant to"
    assert time.min() == MIN64 and time.max() == MAX64 - 1 and (time[:-4] < 0).any() and (time[:-4] > 2 ** 32).any()
    low = time[indptr[7]:indptr[8]] & 0xFFFFFFFF
    assert (np.diff(low) < 0).any(), "the low words alone are not sorted"
    runs = np.diff(time[indptr[HUB]:indptr[HUB + 1]]) == 0
    assert runs[16009] and runs[16010] and not runs[16008] and not runs[16011], "runs of three equal stamps"
    assert 320 % (4096 // 64) == 0 and 195 % -(-4097 // 64) == 0 and 3282 % -(-70001 // 64) == 0 and 70001 > 64 * 64 * 4, "probes; three rounds"
    assert {(f, int(c) - f) for f in (1, 5, 64) for c in cuts} >= {(f, d) for f in (1, 5, 64) for d in (-1, 0, 1)}
    seen_dead = set()
    for which, strategy, fanout, replace in CASES:
        _, _, dst, src, eid, _ = want(which, strategy, fanout, replace)
        assert np.array_equal(eid[dst == list(rows).index(HUB) + 2], eid[dst == rows.size - 1]), "a (row, bound) pair listed twice gets the same picks"
        seen_dead.add(bool((src < 0).any()))
    assert True in seen_dead, "dead entries are picked"
    a, b = want("sorted", ref.UNIFORM, 5, 0), want("scan", ref.UNIFORM, 5, 0)
    assert np.array_equal(a[0], b[0]) and not np.array_equal(a[4], b[4]), "the permuted graph has the same counts at other positions"


def test_set_edge_times_and_the_class_it_selects(world):
    L, g = world["L"], world["sorted"]
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert [world[k].edge_times_sorted for k in ("sorted", "forced", "scan")] == [True, False, False]
    assert all(world[k].has_edge_times for k in ("sorted", "forced", "scan"))
    good = torch.from_numpy(hand_graph()[2]).to(DEV)
    assert L.legion_graph_set_edge_times(None, s, P(good)) == -1 and L.legion_graph_edge_times_sorted(None) == -1
    for bad in (good.int(), good[:-1], good.cpu(), good.cpu().numpy(), good.reshape(1, -1), None):
        g.set_edge_times(good)
        with pytest.raises(ValueError):
            g.set_edge_times(bad)
        assert not g.has_edge_times and not g.edge_times_sorted and L.legion_graph_edge_times_sorted(g.handle) == -1
        for call in (lambda: g.temporal_degrees([0], [0]), lambda: g.sample_temporal_neighbors([0], [0], 1), lambda: g.sample_temporal_layers([0], [0], [1])):
            with pytest.raises(ValueError, match="no edge times"):
                call()
    g.set_edge_times(torch.from_numpy(hand_graph("forced")[2]).to(DEV))     # a second call replaces the times, and the class
    assert g.has_edge_times and not g.edge_times_sorted
    g.set_edge_times(good)
    assert g.edge_times_sorted


@pytest.mark.parametrize("which, strategy, fanout, replace", CASES)
def test_the_edges_are_the_references_bit_for_bit(world, which, strategy, fanout, replace):
    rows, bounds, _ = row_list()
    w = want(which, strategy, fanout, replace)
    M = w[2].size
    for cap, ids in ((M, True), (M + 5, False), (M // 2, True)):
        abi(world, which, rows, bounds, fanout, strategy, replace, 3, w, cap, ids)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 3 * 2048 * 4 + 37])
def test_row_counts_around_a_wave_and_past_the_capped_grid(world, n):
    """The grid is capped at 2 048 workgroups of four rows: the last n is three trips and a remainder.  Rows of at most 65 entries."""
    rows = ((np.arange(n) * 7 + 3) % 6).astype(np.int32)
    bounds = np.array([stamp(DEGREES[r], min(i % 9, DEGREES[r])) for i, r in enumerate(rows)], dtype=np.int64).reshape(n)
    for which in ("sorted", "scan"):
        w = ref.sample(*hand_graph(which), rows, bounds, 5, ref.UNIFORM, 0, -1)
        assert (w[2].size > 0) == (n > 1)
        abi(world, which, rows, bounds, 5, ref.UNIFORM, 0, -1, w, w[2].size + 5)


def test_another_stream_and_a_captured_graph(world):
    L = world["L"]
    rows, bounds, _ = row_list()
    n = rows.size
    torch.cuda.synchronize()
    abi(world, "scan", rows, bounds, 5, ref.UNIFORM, 0, 3, want("scan", ref.UNIFORM, 5, 0), want("scan", ref.UNIFORM, 5, 0)[2].size + 3, stream=torch.cuda.Stream())
    abi(world, "sorted", rows, bounds, 5, ref.LAST, 0, 3, want("sorted", ref.LAST, 5, 0), want("sorted", ref.LAST, 5, 0)[2].size + 3, stream=torch.cuda.Stream())
    for which in ("sorted", "scan"):
        w = want(which, ref.UNIFORM, 5, 0)
        cap = w[2].size + 3
        d_rows, d_bounds = torch.from_numpy(rows).to(DEV), torch.from_numpy(bounds).to(DEV)
        scratch, cand, offsets = (torch.zeros(k, dtype=torch.int64, device=DEV) for k in (1, n, n + 1))
        out = [torch.zeros(cap, dtype=dt, device=DEV) for dt in (torch.int32, torch.int32, torch.int64, torch.int64)]
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            head = (ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), world[which].handle, P(d_rows), P(d_bounds), n, 5, ref.UNIFORM, 0)
            rc = L.legion_temporal_sample_count(*head, P(cand), P(offsets), P(scratch), 8)
            rc |= L.legion_temporal_sample_edges(*head, 3, P(cand), P(offsets), cap, *[P(x) for x in out])
        assert rc == 0
        for _ in range(2):
            for x in [scratch, cand, offsets] + out:
                x.fill_(7)
            graph.replay()
            torch.cuda.synchronize()
            same_arrays([cand, offsets] + out, list(w[:2]) + [np.concatenate([x, np.full(3, -1, dtype=x.dtype)]) for x in w[2:]], "captured " + which,
                        names=("cand", "offsets") + NAMES)


def test_c_abi_refusals_leave_the_outputs_untouched(world):
    from legion_amd import engine
    L = world["L"]
    n, cap = 8, 16
    rows = torch.arange(n, dtype=torch.int32, device=DEV)
    bounds, cand, offsets, scratch, dst, src = [torch.full((cap,), SENTINEL, dtype=torch.int64, device=DEV) for _ in range(6)]
    untimed = engine.GraphStorage(1, *(torch.from_numpy(x).to(DEV) for x in hand_graph()[:2]))
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ok = dict(graph=world["sorted"].handle, rows=P(rows), bounds=P(bounds), n=n, fan=5, strategy=0, replace=0, cand=P(cand), offsets=P(offsets),
              cap=cap, dst=P(dst), src=P(src), scratch=P(scratch), bytes=8)
    both = [dict(n=-1), dict(n=2 ** 20 + 1, bytes=1 << 40), dict(graph=untimed.handle), dict(graph=None), dict(fan=0), dict(fan=65), dict(fan=-2),
            dict(strategy=2), dict(strategy=-1), dict(replace=2), dict(replace=-1), dict(strategy=1, replace=1),
            dict(strategy=1, graph=world["scan"].handle), dict(strategy=1, graph=world["forced"].handle), dict(rows=None), dict(bounds=None),
            dict(cand=None), dict(offsets=None)]
    for change in both + [dict(cap=-1), dict(cap=2 ** 31), dict(dst=None), dict(src=None), dict(scratch=None), dict(bytes=7), dict(bytes=-1)]:
        a = dict(ok, **change)
        head = (s, a["graph"], a["rows"], a["bounds"], a["n"], a["fan"], a["strategy"], a["replace"])
        if change in both or not {"scratch", "bytes"} & set(change):
            assert L.legion_temporal_sample_edges(*head, 0, a["cand"], a["offsets"], a["cap"], a["dst"], a["src"], None, None) == -1, change
        if change in both or {"scratch", "bytes"} & set(change):
            assert L.legion_temporal_sample_count(*head, a["cand"], a["offsets"], a["scratch"], a["bytes"]) == -1, change
    assert [L.legion_temporal_sample_scratch_bytes(x) for x in (0, 256, 257, 2 ** 20, 2 ** 20 + 1, -1)] == [0, 8, 16, 32768, -1, -1]
    assert L.legion_temporal_sample_edges(s, ok["graph"], P(rows), P(bounds), n, 5, 0, 0, 0, P(cand), P(offsets), 0, P(dst), P(src), None, None) == 0   # cap == 0
    torch.cuda.synchronize()
    untimed.close()
    assert all(bool((x == SENTINEL).all()) for x in (bounds, cand, offsets, scratch, dst, src)), "a refused call wrote"


def test_the_python_ops_their_value_errors_and_two_hops(world):
    rows, bounds, cuts = row_list()
    g = world["sorted"]
    for kw in (dict(fanout=0), dict(fanout=65), dict(fanout=-2), dict(fanout=1.5), dict(strategy="first"), dict(strategy=1), dict(replace=1),
               dict(strategy="last", replace=True), dict(salt=2 ** 63), dict(return_eids=1), dict(return_times=0), dict(row_times=[1]),
               dict(row_times=torch.zeros(2, dtype=torch.int32)), dict(rows=torch.zeros(2, dtype=torch.int64))):
        a = dict(dict(rows=[0, 1], row_times=[1, 2], fanout=5), **kw)
        r, t, f = a.pop("rows"), a.pop("row_times"), a.pop("fanout")
        with pytest.raises(ValueError):
            g.sample_temporal_neighbors(r, t, f, **a)
        with pytest.raises(ValueError):
            g.sample_temporal_layers(r, t, [5, f], **a)
    for which in ("scan", "forced"):
        with pytest.raises(ValueError, match="sorted by time"):
            world[which].sample_temporal_neighbors([0], [0], 1, strategy="last")
    with pytest.raises(ValueError):
        g.sample_temporal_layers([0], [0], [])
    with pytest.raises(ValueError):
        g.temporal_degrees([0, 1], [0])
    for which in ("sorted", "forced", "scan"):
        same_arrays(world[which].temporal_degrees(rows, bounds), cuts, "temporal_degrees " + which)
        got = world[which].sample_temporal_neighbors(rows, torch.from_numpy(bounds), 5, salt=3, return_eids=True, return_times=True)
        same_arrays(got, want(which, ref.UNIFORM, 5, 0)[2:], "sample_temporal_neighbors " + which, names=NAMES)
    assert [x.numel() for x in g.sample_temporal_neighbors([], [], 5, return_times=True)] == [0, 0, 0] and g.temporal_degrees([], []).numel() == 0
    same_arrays(g.sample_temporal_neighbors(rows, bounds, 64, strategy="last"), want("sorted", ref.LAST, 64, 0)[2:4], "last", names=NAMES)
    # two hops: the second samples the first's sources, dead ones (-1, rows outside the graph) included, under their rows' bounds
    for which, strategy, name in (("sorted", ref.LAST, "last"), ("scan", ref.UNIFORM, "uniform")):
        graph = hand_graph(which)
        h0 = ref.sample(*graph, rows, bounds, 5, strategy, 0, 9)[2:]
        h1 = ref.sample(*graph, h0[1], bounds[h0[0]], 64, strategy, 0, 9)[2:]
        assert (h0[1] < 0).any() and h1[0].size > 64
        got = world[which].sample_temporal_layers(rows, bounds, [5, 64], strategy=name, salt=9, return_eids=True, return_times=True)
        same_arrays(got[0] + got[1], h0 + h1, "two hops " + which, names=NAMES + NAMES)


def test_a_timed_hub_astride_the_far_edge_offset_2_31(hip):
    """tests/far_rows.py's layout at the 2^31 boundary with times: 0 on the ballast, the position inside the row on a live row (the
    sorted class), then the same positions counted from the row's end (every live row decreases: the scan class), in place.  A row's
    bound leaves three quarters of it, so the straddling hub has candidates, and true edge ids, on both sides of the boundary.  The
    2^32 boundary is left out: the int64 time array alone would be 34 GB on a shared card."""
    with far_rows.device_world(hip, "2^31") as w:
        g, graph = w["g"], w["graph"]
        deg = np.diff(g.indptr_ref)
        pos = np.arange(g.live_E, dtype=np.int64) - np.repeat(g.indptr_ref[:-1], deg)
        rows = g.seeds(300)
        inside = (rows >= 0) & (rows < g.node_num)
        bounds = np.where(inside, np.diff(g.indptr)[np.where(inside, rows, 0)] * 3 // 4 + 1, 0).astype(np.int64)
        time = torch.zeros(g.E, dtype=torch.int64, device=DEV)
        for sorted_class, live in ((True, pos), (False, np.repeat(deg, deg) - 1 - pos)):
            time[g.offset:] = torch.from_numpy(live).to(DEV)
            graph.set_edge_times(time)
            assert graph.edge_times_sorted == sorted_class
            same_arrays(graph.temporal_degrees(rows, bounds), ref.degrees(g.indptr_ref, live, rows, bounds), "degrees" + w["why"])
            for strategy, name, replace in ((ref.UNIFORM, "uniform", False), (ref.UNIFORM, "uniform", True), (ref.LAST, "last", False))[:3 if sorted_class else 2]:
                want_ = ref.sample(g.indptr_ref, g.col_ref, live, rows, bounds, 64, strategy, replace, 9, add=g.offset)[2:]
                if strategy == ref.UNIFORM:
                    g.assert_straddles(rows[want_[0]].astype(np.int64), want_[2], f"temporal sorted {sorted_class} replace {replace}")
                got = graph.sample_temporal_neighbors(rows, bounds, 64, strategy=name, replace=replace, salt=9, return_eids=True, return_times=True)
                same_arrays(got, want_, f"sorted {sorted_class} {name} replace {replace}" + w["why"], names=NAMES)
        del time
