"""Typed edges and per-edge-type fan-outs on the GPU (legion_graph_set_edge_types, legion_etype_degrees, legion_etype_sample_count,
legion_etype_sample_edges and the Python ops over them), bit for bit against tests/etype_ref.py, on one hand-made graph: row degrees
around a wave, around 4 096 and a hub of 70 001; T in {1, 2, 63, 64}; a row's first T - 1 segment boundaries from CUTS (a row's ends: a
missing first or last type and single-type rows; entries 64 and 65; sample positions of the 64-way step; one-entry segments at either
end of a long row; runs of 63, 64, 65 and 4, 5, 6 entries; repeats: missing middle types); dead entries.  What makes a wrong kernel
fail is asserted from the reference before any launch."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import etype_ref as ref
from tests import far_rows
from tests.compare import same_arrays
from tests.gpu_harness import GpuSide
from tests.helpers import Workload

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 0x5A5A5A5A
DEGREES = [0, 1, 2, 4, 5, 6, 63, 64, 65, 128, 4095, 4096, 4097, 70001, 300, 200]
CUTS = [[], [0], [1], [4], [0], [5], [63, 4, 9], [1, 63], [64], [64, 65, 65, 100], [1, 4094, 2000], [320, 383, 447, 512, 1000],
        [195, 199, 204, 210, 3000], [10940, 10941, 70000, 30000], [300], [0] * 63]      # then evenly spread from the last one to the row's end
HUB, N = 13, len(DEGREES)
ROWS = np.concatenate([np.arange(N), [-1, N, HUB, 3], np.arange(N - 3)[::-1]]).astype(np.int32)      # every row; outside ones; repeats
NAMES = ("dst", "src", "eid", "etype")
FANOUTS = {1: [[1], [5], [64], [-1]], 2: [[5, -1], [64, 5], [0, 64], [-1, 0], [1, 1]],
           63: [([5, -1, 0, 1, 64, 5, 64, 1] * 9)[s:s + 63] for s in (0, 3)], 64: [([5, -1, 0, 1, 64, 5, 64, 1] * 9)[s:s + 64] for s in (0, 3)]}
CASES = [(T, shift, replace) for T in FANOUTS for shift in range(len(FANOUTS[T])) for replace in (0, 1)]


@functools.lru_cache(maxsize=None)
def hand_graph():
    rng = np.random.RandomState(7)
    indptr = np.concatenate([[0], np.cumsum(DEGREES)]).astype(np.int64)
    col = rng.randint(0, N, int(indptr[-1])).astype(np.int32)
    col[rng.rand(col.size) < 0.03] = -1
    return indptr, col


@functools.lru_cache(maxsize=None)
def types(T):
    indptr, col = hand_graph()
    etype = np.zeros(col.size, dtype=np.uint8)
    for r, d in enumerate(DEGREES):
        start = CUTS[r][-1] if CUTS[r] else 0
        cuts = np.sort((CUTS[r] + [start + (d - start + 1) * j // 67 for j in range(1, 64)])[:T - 1])
        etype[indptr[r]:indptr[r + 1]] = np.searchsorted(cuts, np.arange(d), side="right")
    return etype


@functools.lru_cache(maxsize=None)
def want(T, shift, replace):
    return ref.sample(*hand_graph(), types(T), T, ROWS, FANOUTS[T][shift], replace, 3)


@pytest.fixture(scope="module")
def world(hip):
    from legion_amd import engine
    indptr, col = hand_graph()
    graph = engine.GraphStorage(1, torch.from_numpy(indptr).to(DEV), torch.from_numpy(col).to(DEV))
    yield dict(graph=graph, L=hip)
    torch.cuda.synchronize()
    graph.close()


def typed(world, T):
    world["graph"].set_edge_types(types(T), T)
    return world["graph"]


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def abi(world, rows, fan, replace, salt, w, cap, ids=True, stream=None):
    """count, then edges over sentinel-filled buffers with 8 spare entries, against the reference's w: the offsets; [0, min(M, cap)) the
    picks; [M, cap) -1 (255 in etype); nothing past cap, the offsets and the scratch."""
    L, g, n = world["L"], world["graph"], rows.size
    d_rows = torch.from_numpy(rows).to(DEV) if n else torch.zeros(1, dtype=torch.int32, device=DEV)
    s = ctypes.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    fan = (ctypes.c_int32 * len(fan))(*fan)
    nbytes = int(L.legion_etype_sample_scratch_bytes(n))
    assert nbytes == 8 * ((n + 255) // 256)
    full = lambda size, dtype: torch.full((size + 8,), 0x5A if dtype == torch.uint8 else SENTINEL, dtype=dtype, device=DEV)
    scratch, offsets = full(nbytes // 8, torch.int64), full(n + 1, torch.int64)
    out = [full(cap, torch.int32), full(cap, torch.int32), full(cap, torch.int64) if ids else None, full(cap, torch.uint8) if ids else None]
    assert L.legion_etype_sample_count(s, g.handle, P(d_rows), n, fan, replace, P(offsets), P(scratch), nbytes) == 0
    assert L.legion_etype_sample_edges(s, g.handle, P(d_rows), n, fan, replace, salt, P(offsets), cap, *[P(x) for x in out]) == 0
    torch.cuda.synchronize()
    M = w[1].size
    same_arrays(offsets, np.concatenate([w[0], np.full(8, SENTINEL)]), "offsets")
    assert bool((scratch[nbytes // 8:] == SENTINEL).all()), "written past the scratch"
    for name, x, ref_x in zip(NAMES, out, w[1:]):
        if x is not None:
            fill, past = (255, 0x5A) if name == "etype" else (-1, SENTINEL)
            tail = np.concatenate([np.full(max(cap - M, 0), fill), np.full(8, past)]).astype(ref_x.dtype)
            same_arrays(x, np.concatenate([ref_x[:cap], tail]), f"cap {cap} of {M}", names=[name])


def test_the_inputs_hold_their_conditions_before_any_launch():
    indptr, col = hand_graph()
    seen, dead = set(), set()             # (fan-out, segment length - fan-out); is a dead pick's pair taken whole?
    for T, shift, replace in CASES:
        D = ref.degrees(indptr, types(T), np.arange(N), T)
        fan = FANOUTS[T][shift]
        seen |= {(f, int(d) - f) for row in D for f, d in zip(fan, row) if abs(int(d) - f) <= 1}
        _, dst, src, eid, ety = want(T, shift, replace)
        dead |= {bool(ref.slots(int(D[ROWS[i], t]), fan[t], replace) == D[ROWS[i], t]) for i, t in zip(dst[src < 0], ety[src < 0])}
        assert np.array_equal(eid[dst == HUB], eid[dst == N + 2]), "a row listed twice gets the same picks"
    assert {(f, d) for f in (1, 5, 64) for d in (-1, 0, 1)} <= seen and dead == {False, True}
    for T in (2, 63, 64):
        D = ref.degrees(indptr, types(T), np.arange(N), T)
        b = lambda r: (ref.segments(indptr, types(T), r, T) - indptr[r]).tolist()
        assert D[1, 0] == 0 and D[6, T - 1] == 0 and not D[14, 1:].any() and not D[15, :-1].any(), "missing first / last type, single-type rows"
        assert 64 in b(8) and 64 in b(9) and 1 in b(10) and 320 in b(11) and 195 in b(12) and 10940 in b(HUB), "boundaries at 64 and on samples"
        assert 320 % (4096 // 64) == 0 and 195 % -(-4097 // 64) == 0 and 10940 % -(-70001 // 64) == 0
        if T > 2:
            assert 65 in b(9) and D[9, 2] == 0 and D[10, 0] == 1 and D[10, T - 1] == 1 and D[HUB, 1] == 1, "a missing middle type, one-entry segments"
            assert {63, 64, 65} <= set(D[11].tolist()) and {4, 5, 6} <= set(D[12].tolist())


def test_set_edge_types_refuses_and_leaves_the_graph_untyped(world):
    indptr, col = hand_graph()
    L, g = world["L"], world["graph"]
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = torch.from_numpy(types(63)).to(DEV)
    swapped = good.clone()                                             # one swapped pair, in the last row
    swapped[-50], swapped[-49] = 62, 61
    rows, buf = torch.zeros(4, dtype=torch.int32, device=DEV), torch.full((64,), SENTINEL, dtype=torch.int64, device=DEV)
    fan = (ctypes.c_int32 * 64)(*[1] * 64)
    for et, T, code in ((swapped, 63, -5), (good, 62, -4), (good, 0, -3), (good, 65, -3), (None, 63, -2)):
        assert L.legion_graph_set_edge_types(g.handle, s, P(good), 64) == 0 and g.num_edge_types == 64      # typed just before
        assert L.legion_graph_set_edge_types(g.handle, s, P(et), T) == code and g.num_edge_types == 0, code
        # the untyped graph is refused by every op, before anything is enqueued
        assert L.legion_etype_degrees(s, g.handle, P(rows), 4, P(buf)) == -1
        assert L.legion_etype_sample_count(s, g.handle, P(rows), 4, fan, 0, P(buf), P(buf), 512) == -1
        assert L.legion_etype_sample_edges(s, g.handle, P(rows), 4, fan, 0, 0, P(buf), 16, P(buf), P(buf), None, None) == -1
    assert L.legion_graph_set_edge_types(None, s, P(good), 4) == -1
    for bad, T in ((swapped, 63), (good, 62), (good, 0), (good, 65), (good.int(), 63), (good[:-1], 63), (good, 2.0)):
        g.set_edge_types(good, 63)
        with pytest.raises(ValueError):
            g.set_edge_types(bad, T)
        assert g.num_edge_types == 0
    for call in (lambda: g.etype_degrees([0]), lambda: g.sample_etype_neighbors([0], [1]), lambda: g.sample_etype_block([0], [1])):
        with pytest.raises(ValueError, match="no edge types"):
            call()
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all()), "a refused call wrote"


@pytest.mark.parametrize("T, shift, replace", CASES)
def test_the_edges_are_the_references_bit_for_bit(world, T, shift, replace):
    same_arrays(typed(world, T).etype_degrees(ROWS), ref.degrees(hand_graph()[0], types(T), ROWS, T), "etype_degrees")
    w = want(T, shift, replace)
    M = w[1].size
    for cap, ids in ((M, True), (M + 5, False), (M // 2, True)):
        abi(world, ROWS, FANOUTS[T][shift], replace, 3, w, cap, ids)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 3 * 2048 * 4 + 37])
def test_row_counts_around_a_wave_and_past_the_capped_grid(world, n):
    """The grid is capped at 2 048 workgroups of four rows: the last n is three trips and a remainder.  Rows of at most 128 entries."""
    typed(world, 2)
    rows = ((np.arange(n) * 7 + 3) % 10).astype(np.int32)
    w = ref.sample(*hand_graph(), types(2), 2, rows, [5, 64], 0, -1)
    assert (w[1].size > 0) == (n > 0)
    abi(world, rows, [5, 64], 0, -1, w, w[1].size + 5)


def test_another_stream_and_a_captured_graph(world):
    L, g = world["L"], typed(world, 64)
    fan, w = FANOUTS[64][1], want(64, 1, 0)
    n, cap = ROWS.size, w[1].size + 3
    torch.cuda.synchronize()
    abi(world, ROWS, fan, 0, 3, w, cap, stream=torch.cuda.Stream())
    d_rows, c_fan = torch.from_numpy(ROWS).to(DEV), (ctypes.c_int32 * 64)(*fan)
    scratch, offsets = torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    out = [torch.zeros(cap, dtype=dt, device=DEV) for dt in (torch.int32, torch.int32, torch.int64, torch.uint8)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cs = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = L.legion_etype_sample_count(cs, g.handle, P(d_rows), n, c_fan, 0, P(offsets), P(scratch), 8)
        rc |= L.legion_etype_sample_edges(cs, g.handle, P(d_rows), n, c_fan, 0, 3, P(offsets), cap, *[P(x) for x in out])
    assert rc == 0
    for _ in range(2):
        for x in [scratch, offsets] + out:
            x.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        tails = [np.full(3, 255 if name == "etype" else -1).astype(x.dtype) for name, x in zip(NAMES, w[1:])]
        same_arrays([offsets] + out, [w[0]] + [np.concatenate([x, t]) for x, t in zip(w[1:], tails)], "captured", names=("offsets",) + NAMES)


def test_c_abi_refusals_leave_the_outputs_untouched(world):
    L, g = world["L"], typed(world, 2).handle
    n, cap = 8, 16
    rows = torch.arange(n, dtype=torch.int32, device=DEV)
    offsets, scratch, dst, src = [torch.full((cap,), SENTINEL, dtype=torch.int64, device=DEV) for _ in range(4)]
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ok = dict(graph=g, rows=P(rows), n=n, fan=[5, -1], replace=0, offsets=P(offsets), cap=cap, dst=P(dst), src=P(src), scratch=P(scratch), bytes=8)
    both = [dict(n=-1), dict(n=2 ** 20 + 1, bytes=1 << 40), dict(fan=[5, -2]), dict(fan=[65, 0]), dict(replace=2), dict(replace=-1), dict(graph=None),
            dict(rows=None), dict(fan=None), dict(offsets=None)]
    for change in both + [dict(cap=-1), dict(cap=2 ** 31), dict(dst=None), dict(src=None), dict(scratch=None), dict(bytes=7), dict(bytes=-1)]:
        a = dict(ok, **change)
        fan = None if a["fan"] is None else (ctypes.c_int32 * 2)(*a["fan"])
        if change in both or not {"scratch", "bytes"} & set(change):
            assert L.legion_etype_sample_edges(s, a["graph"], a["rows"], a["n"], fan, a["replace"], 0, a["offsets"], a["cap"], a["dst"], a["src"], None, None) == -1, change
        if change in both or {"scratch", "bytes"} & set(change):
            assert L.legion_etype_sample_count(s, a["graph"], a["rows"], a["n"], fan, a["replace"], a["offsets"], a["scratch"], a["bytes"]) == -1, change
    for args in ((g, P(rows), -1, P(dst)), (g, P(rows), 2 ** 20 + 1, P(dst)), (None, P(rows), n, P(dst)), (g, None, n, P(dst)), (g, P(rows), n, None)):
        assert L.legion_etype_degrees(s, *args) == -1, args
    assert [L.legion_etype_sample_scratch_bytes(x) for x in (0, 256, 257, 2 ** 20, 2 ** 20 + 1, -1)] == [0, 8, 16, 32768, -1, -1]
    assert L.legion_etype_sample_edges(s, g, P(rows), n, (ctypes.c_int32 * 2)(5, -1), 0, 0, P(offsets), 0, P(dst), P(src), None, None) == 0      # cap == 0
    torch.cuda.synchronize()
    assert all(bool((x == SENTINEL).all()) for x in (offsets, scratch, dst, src)), "a refused call wrote"


def test_the_python_ops_their_value_errors_and_the_block_through_set_ids(world):
    from legion_amd import engine
    indptr, col = hand_graph()
    g = typed(world, 2)
    for kw in (dict(fanouts=[5]), dict(fanouts=[5, 65]), dict(fanouts=[-2, 5]), dict(fanouts=[5, 1.5]), dict(fanouts=5), dict(replace=1),
               dict(salt=2 ** 63), dict(return_eids=1), dict(exclude_eids=[1, 2]), dict(seeds=[3, 3]), dict(seeds=[N]), dict(seeds=[-1])):
        a = dict(dict(seeds=[0, 1], fanouts=[5, 5]), **kw)
        seeds, fan = a.pop("seeds"), a.pop("fanouts")
        with pytest.raises(ValueError):
            g.sample_etype_block(seeds, fan, **a)
        if not {"seeds", "exclude_eids"} & set(kw):
            with pytest.raises(ValueError):
                g.sample_etype_neighbors(seeds, fan, **a)
    fan = FANOUTS[2][0]
    same_arrays(g.sample_etype_neighbors(ROWS, fan, salt=3, return_eids=True), want(2, 0, 0)[1:], "sample_etype_neighbors", names=NAMES)
    assert [x.numel() for x in g.sample_etype_neighbors([], fan, return_etypes=False)] == [0, 0]
    # the block: the seeds first, dead picks masked out, the types riding along; then without a third of its edges
    seeds = np.array([9, 12, 3, 7, 10], dtype=np.int32)
    _, dst, src, eid, ety = ref.sample(indptr, col, types(2), 2, seeds, fan, 0, 5)
    live = src >= 0
    assert 0 < live.sum() < live.size
    for excl, keep in ((None, live), (engine.EdgeIdSet(eid[live][::3], device=DEV), live & ~np.isin(eid, eid[live][::3]))):
        nodes, d_local, s_local, b_ety, b_eid = g.sample_etype_block(seeds, fan, salt=5, return_eids=True, exclude_eids=excl)
        ids = nodes.cpu().numpy()
        assert np.array_equal(ids[:seeds.size], seeds) and np.unique(ids).size == ids.size and np.array_equal(ids[s_local.cpu().numpy()], src[keep])
        same_arrays([d_local, b_ety, b_eid], [dst[keep], ety[keep], eid[keep]], "block", names=["dst_local", "etypes", "eids"])
    # input_nodes through the host to FeatureStorage.set_ids: a batch over them samples for exactly these rows, in order
    wl = Workload(dim=4, indptr=indptr, col=col, n_seeds=64, n_valid=8, n_test=8)
    wl.sets[(0, 0)] = (np.ascontiguousarray(ids), np.ascontiguousarray(wl.labels_all[ids]))
    gpu = GpuSide(wl, ids.size, [2], edge_ids=True)
    try:
        assert np.array_equal(gpu.run(0, 0, 0)["sampled_ids"][:ids.size], ids), "the batch's first rows are the block's input nodes, in order"
    finally:
        torch.cuda.synchronize()
        gpu.close()


@pytest.mark.parametrize("boundary", ["2^31", "2^32"])
def test_a_typed_hub_astride_a_far_edge_offset(hip, boundary):
    """tests/far_rows.py's layout, typed: the ballast is of type 0, a live row's entries are split evenly over four types.  The straddling
    hub is taken whole in one type and sampled in the others, with true edge ids on both sides of the boundary."""
    T, fan = 4, [5, -1, 64, 1]
    with far_rows.device_world(hip, boundary) as w:
        g = w["g"]
        deg = np.diff(g.indptr_ref)
        live = ((np.arange(g.live_E) - np.repeat(g.indptr_ref[:-1], deg)) * T // np.repeat(deg, deg)).astype(np.uint8)
        rows = g.seeds(300)
        etype = torch.zeros(g.E, dtype=torch.uint8, device=DEV)
        etype[g.offset:] = torch.from_numpy(live).to(DEV)
        w["graph"].set_edge_types(etype, T)
        same_arrays(w["graph"].etype_degrees(rows), ref.degrees(g.indptr_ref, live, rows, T), "degrees" + w["why"])
        for replace in (False, True):
            _, dst, src, eid, ety = ref.sample(g.indptr_ref, g.col_ref, live, T, rows, fan, replace, 9, add=g.offset)
            g.assert_straddles(rows[dst].astype(np.int64), eid, f"etype sample replace {replace}")
            hub = rows[dst] == g.hub
            assert ((ety == 1) & hub & (eid < g.boundary)).any() and ((ety == 2) & hub & (eid >= g.boundary)).any(), "a type on either side"
            got = w["graph"].sample_etype_neighbors(rows, fan, replace=replace, salt=9, return_eids=True)
            same_arrays(got, [dst, src, eid, ety], f"replace {replace}" + w["why"], names=NAMES)
