"""Metapath walks and PinSAGE over a metapath on the GPU (legion_metapath_walk, legion_pinsage_metapath_neighbors and the Python ops over
them), bit for bit against tests/metapath_ref.py on its hand-made typed graph: rows of 0 .. 17 and 63 .. 65 entries around the short
class's threshold (16), a row of 4 097 and a hub of 70 001; T in {1, 2, 64}; walk counts around a tile of 256 and past it; periods and
lengths around a chunk of 16 (8 with edge ids) and a period of 64.  What makes a wrong kernel fail is asserted from the reference before
any launch (metapath_ref.assert_hand_graph)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import far_rows
from tests import metapath_ref as ref
from tests.compare import same_arrays

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 0x5A5A5A5A
SHAPES = [(1, 1), (2, 2), (3, 16), (3, 17), (64, 64), (2, 100)]      # (L, length)
PINSAGE = [(4, 3, 5, 2), (10, 5, 10, 3), (16, 16, 20, 1), (64, 16, 1024, 2)]      # (R, Q, k, L): VPAD 32, 64, 256, 1024


@functools.lru_cache(maxsize=None)
def want(T, L, length, restart):
    indptr, col, _ = ref.hand_graph()
    return ref.walk(indptr, col, ref.keys(T), ref.seeds(), ref.metapath(T, L), length, restart, base=7)


@pytest.fixture(scope="module")
def world(hip):
    from legion_amd import engine
    ref.assert_hand_graph()
    indptr, col, _ = ref.hand_graph()
    graph = engine.GraphStorage(1, torch.from_numpy(indptr.copy()).to(DEV), torch.from_numpy(col.copy()).to(DEV))
    yield dict(graph=graph, L=hip)
    torch.cuda.synchronize()
    graph.close()


def typed(world, T, offset=0):
    """The graph with ref.types(T), the tensor a view `offset` bytes into a larger one."""
    room = torch.zeros(ref.types(T).size + 32, dtype=torch.uint8, device=DEV)
    view = room[offset:offset + ref.types(T).size]
    view.copy_(torch.from_numpy(ref.types(T).copy()))
    world["graph"].set_edge_types(view, T)
    return world["graph"]


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


@pytest.mark.parametrize("restart", [0.0, 0.3])
@pytest.mark.parametrize("L, length", SHAPES)
@pytest.mark.parametrize("T", [1, 2, 64])
def test_the_walks_are_the_references_bit_for_bit(world, T, L, length, restart):
    g, seeds = typed(world, T), ref.seeds()
    traces, eids = want(T, L, length, restart)
    for n in (1, 255, 256, 257, 5000):
        got = g.metapath_random_walk(seeds[:n].copy(), ref.metapath(T, L), repeats=length // L, restart_prob=restart, return_eids=True, base=7) \
            if length % L == 0 else None
        if got is not None:
            same_arrays(got, [traces[:n], eids[:n]], f"T {T} L {L} length {length} n {n}", names=["traces", "eids"])
        # the C call: any length over the period, with and without edge ids, nothing written past either buffer
        path, d_seeds = (ctypes.c_uint8 * L)(*ref.metapath(T, L)), torch.from_numpy(seeds[:n].copy()).to(DEV)
        for with_ids in (True, False):
            out = torch.full((n * (length + 1) + 8,), SENTINEL, dtype=torch.int32, device=DEV)
            ids = torch.full((n * length + 8,), SENTINEL, dtype=torch.int64, device=DEV)
            s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            assert world["L"].legion_metapath_walk(s, g.handle, P(d_seeds), n, path, L, length, restart, 7, P(out), P(ids) if with_ids else None) == 0
            tail = np.full(8, SENTINEL)
            same_arrays([out, ids], [np.concatenate([traces[:n].ravel(), tail]).astype(np.int32),
                                     np.concatenate([eids[:n].ravel(), tail]) if with_ids else np.full(n * length + 8, SENTINEL)],
                        f"abi T {T} L {L} length {length} n {n} ids {with_ids}", names=["traces", "eids"])


@pytest.mark.parametrize("restart", [0.0, 0.3])
def test_one_type_is_random_walk_and_pinsage_neighbors_bit_for_bit(world, restart):
    g, seeds = typed(world, 1), torch.from_numpy(ref.seeds().copy()).to(DEV)
    for length in (1, 17, 100):
        ours = g.metapath_random_walk(seeds, [0], repeats=length, restart_prob=restart, return_eids=True, base=3)
        theirs = g.random_walk(seeds, length, restart_prob=restart, return_eids=True, base=3)
        same_arrays(ours, [x.cpu().numpy() for x in theirs], f"length {length}", names=["traces", "eids"])
    for R, Q, k, _ in PINSAGE:
        ours = g.pinsage_metapath_neighbors(seeds[:300], [0], R, Q, k, termination_prob=restart, base=3)
        theirs = g.pinsage_neighbors(seeds[:300], R, Q, k, termination_prob=restart, base=3)
        same_arrays(ours, [x.cpu().numpy() for x in theirs], f"R {R} Q {Q} k {k}", names=["neighbors", "counts"])


@pytest.mark.parametrize("offset", [1, 15])
def test_a_type_array_that_starts_off_a_word(world, offset):
    """The short class reads aligned words where they lie inside the array and bytes at its ends: the first rows and the last ones."""
    g = typed(world, 64, offset)
    last = np.arange(ref.NODE_NUM - 40, ref.NODE_NUM, dtype=np.int32)
    seeds = np.concatenate([ref.seeds()[:300], last]).astype(np.int32)
    indptr, col, _ = ref.hand_graph()
    w = ref.walk(indptr, col, ref.keys(64), seeds, ref.metapath(64, 3), 17, 0.0, base=0)
    assert (w[0][-40:, 1] >= 0).sum() >= 20 and (w[0][:9, 1] >= 0).sum() >= 5, "steps are taken from the array's first and last rows"
    same_arrays(g.metapath_random_walk(seeds, (ref.metapath(64, 3) * 6)[:17], return_eids=True), w, f"offset {offset}", names=["traces", "eids"])


@pytest.mark.parametrize("n", [1, 63, 65, 300])
@pytest.mark.parametrize("R, Q, k, L", PINSAGE)
def test_pinsage_over_a_metapath_is_the_references(world, R, Q, k, L, n):
    indptr, col, _ = ref.hand_graph()
    for T, term in ((64, 0.5), (2, 0.0)):
        g, seeds = typed(world, T), ref.seeds()[11 - min(n, 11):][:n].copy()   # (n == 1: the hub alone)
        w = ref.neighbors(indptr, col, ref.keys(T), seeds, ref.metapath(T, L), R, Q, k, term, base=5)
        assert n < 63 or ((w[1] > 1).any() and (w[0] < 0).any()), "repeated visits, and rows with fewer than k neighbours"
        same_arrays(g.pinsage_metapath_neighbors(seeds, ref.metapath(T, L), R, Q, k, termination_prob=term, base=5), w,
                    f"T {T} R {R} Q {Q} k {k} L {L} n {n}", names=["neighbors", "counts"])


def test_another_stream_and_a_captured_graph(world):
    L, g = world["L"], typed(world, 64)
    n, length = 5000, 17
    traces, eids = want(64, 3, length, 0.3)
    d_seeds, path = torch.from_numpy(ref.seeds().copy()).to(DEV), (ctypes.c_uint8 * 3)(*ref.metapath(64, 3))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    got = g.metapath_random_walk(d_seeds, (ref.metapath(64, 3) * 6)[:17], restart_prob=0.3, return_eids=True, base=7, stream=side)
    side.synchronize()
    same_arrays(got, [traces, eids], "another stream", names=["traces", "eids"])
    seeds300 = ref.seeds()[:300].copy()
    indptr, col, _ = ref.hand_graph()
    w = ref.neighbors(indptr, col, ref.keys(64), seeds300, ref.metapath(64, 3), 10, 5, 10, 0.5, base=5)
    out, ids = torch.zeros(n * (length + 1), dtype=torch.int32, device=DEV), torch.zeros(n * length, dtype=torch.int64, device=DEV)
    nb, ct = torch.zeros(300 * 10, dtype=torch.int32, device=DEV), torch.zeros(300 * 10, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cs = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = L.legion_metapath_walk(cs, g.handle, P(d_seeds), n, path, 3, length, 0.3, 7, P(out), P(ids))
        rc |= L.legion_pinsage_metapath_neighbors(cs, g.handle, P(d_seeds), 300, path, 3, 10, 5, 10, 0.5, 5, P(nb), P(ct))
    assert rc == 0
    for _ in range(2):
        for x in (out, ids, nb, ct):
            x.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        same_arrays([out, ids, nb, ct], [traces.ravel(), eids.ravel(), w[0].ravel(), w[1].ravel()], "captured", names=["traces", "eids", "neighbors", "counts"])


def test_c_abi_refusals_leave_the_outputs_untouched_and_the_value_errors(world):
    L, g = world["L"], typed(world, 2)
    seeds = torch.arange(8, dtype=torch.int32, device=DEV)
    a_buf, b_buf = [torch.full((4096,), SENTINEL, dtype=torch.int64, device=DEV) for _ in range(2)]
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ok = dict(graph=g.handle, seeds=P(seeds), n=8, path=[0, 1], L=2, length=4, R=4, Q=3, k=10, prob=0.5, base=0, a=P(a_buf), b=P(b_buf))
    both = [dict(n=-1), dict(base=-1), dict(L=0), dict(L=65), dict(base=2 ** 31), dict(graph=None), dict(path=[0, 2]), dict(prob=1.5),
            dict(prob=float("nan")), dict(seeds=None), dict(a=None), dict(path=None)]
    for change in both + [dict(length=0), dict(R=0), dict(Q=0), dict(k=0), dict(R=1025, Q=1), dict(k=1025), dict(b=None), dict(untyped=True)]:
        c = dict(ok, **change)
        if c.get("untyped"):
            L.legion_graph_set_edge_types(g.handle, s, None, 0)
        path = None if c["path"] is None else (ctypes.c_uint8 * 64)(*c["path"])
        if change in both or set(change) & {"length", "untyped"}:
            assert L.legion_metapath_walk(s, c["graph"], c["seeds"], c["n"], path, c["L"], c["length"], c["prob"], c["base"], c["a"], c["b"]) == -1, change
        if change in both or set(change) & {"R", "Q", "k", "b", "untyped"}:
            assert L.legion_pinsage_metapath_neighbors(s, c["graph"], c["seeds"], c["n"], path, c["L"], c["R"], c["Q"], c["k"], c["prob"], c["base"],
                                                       c["a"], c["b"]) == -1, change
    with pytest.raises(ValueError, match="no edge types"):
        g.metapath_random_walk([0], [0])
    g = typed(world, 2)
    path = (ctypes.c_uint8 * 2)(0, 1)
    assert L.legion_metapath_walk(s, g.handle, P(seeds), 0, path, 2, 4, 0.5, 0, P(a_buf), None) == 0      # no walks: nothing enqueued
    assert L.legion_pinsage_metapath_neighbors(s, g.handle, P(seeds), 0, path, 2, 4, 3, 10, 0.5, 0, P(a_buf), P(b_buf)) == 0
    torch.cuda.synchronize()
    assert bool((a_buf == SENTINEL).all()) and bool((b_buf == SENTINEL).all()), "a refused call wrote"
    for kw in (dict(metapath=[]), dict(metapath=[0] * 65), dict(metapath=[0, 2]), dict(metapath=[-1]), dict(metapath=[0.5]), dict(metapath=3),
               dict(repeats=0), dict(repeats=1.5), dict(restart_prob=1.5), dict(return_eids=1), dict(base=-1), dict(base=2 ** 31)):
        c = dict(dict(metapath=[0, 1]), **kw)
        with pytest.raises(ValueError):
            g.metapath_random_walk([0, 1], c.pop("metapath"), **c)
    for kw in (dict(metapath=[0, 2]), dict(R=0), dict(Q=0), dict(k=0), dict(R=1025), dict(k=1025), dict(termination_prob=-0.1), dict(base=2 ** 31 - 20)):
        c = dict(dict(metapath=[0, 1], R=4, Q=3, k=10), **kw)
        with pytest.raises(ValueError):
            g.pinsage_metapath_neighbors([0, 1], c.pop("metapath"), c.pop("R"), c.pop("Q"), c.pop("k"), **c)
    assert g.metapath_random_walk([], [0, 1]).shape == (0, 3) and [x.shape for x in g.pinsage_metapath_neighbors([], [0, 1], 4, 3, 10)] == [(0, 10)] * 2


def test_a_typed_hub_astride_edge_offset_2_31(hip):
    """tests/far_rows.py's layout, typed as tests/test_gpu_etype.py types it: the ballast of type 0, a live row's entries split evenly
    over four types.  Walks leave the straddling hub to both sides of the boundary, with true edge ids."""
    T, path = 4, [1, 2, 0, 3, 2]
    with far_rows.device_world(hip, "2^31") as w:
        g = w["g"]
        deg = np.diff(g.indptr_ref)
        live = ((np.arange(g.live_E) - np.repeat(g.indptr_ref[:-1], deg)) * T // np.repeat(deg, deg)).astype(np.uint8)
        etype = torch.zeros(g.E, dtype=torch.uint8, device=DEV)
        etype[g.offset:] = torch.from_numpy(live).to(DEV)
        w["graph"].set_edge_types(etype, T)
        seeds = g.seeds(5000)
        traces, eids = ref.walk(g.indptr_ref, g.col_ref, ref.row_keys(g.indptr_ref, live), seeds, path, 15)
        eids = g.true_eids(eids, g.offset)
        g.assert_straddles(traces[:, :-1], eids, "metapath walk")
        same_arrays(w["graph"].metapath_random_walk(seeds, path, repeats=3, return_eids=True), [traces, eids], "far rows" + w["why"], names=["traces", "eids"])
        want_nb = ref.neighbors(g.indptr_ref, g.col_ref, ref.row_keys(g.indptr_ref, live), seeds[:300], path[:2], 10, 5, 10)
        same_arrays(w["graph"].pinsage_metapath_neighbors(seeds[:300], path[:2], 10, 5, 10), want_nb, "far rows pinsage" + w["why"], names=["neighbors", "counts"])
