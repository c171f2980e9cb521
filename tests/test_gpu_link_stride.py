"""One stride of the grid and a bit for the link seed ops: every kernel of kernels_link.hip caps its grid at 2 048 workgroups
(LG_WALK_MAX_WG) and strides over tiles, so only a call of more than 2 048 tiles sends a workgroup through its loop a second time --
find_edges past 2 048 x 1 024 edge ids, negative_sample past 524 288 slots, the kernels of unique_ids past 524 288 ids (and its
one-workgroup scan changes shape at 256 tiles: a thread takes a run of tiles from 257 on, and the last run is short at 2 050).  Whole
arrays bit for bit against tests/link_ref.py, unique_ids twice.

Before the GPU runs, each test checks from the reference alone that a wrong second trip could not pass (tests/test_link_cpu.py checks
the same without a GPU, and that a second trip which repeats the tile 2 048 earlier fails every case here):
  find_edges       the expected (row, col) of a second-trip index differs from that of the index 2 097 152 earlier at 99 % of the
                   positions at least, and the ids placed by hand behind the stride give what they are named for;
  negative_sample  counted over the rows that lie wholly in the second trip: with the edge exclusion at least 20 rejections by a search
                   hit; with the edge exclusion and max_tries = 3 at least 20 exhausted slots; the two rows outside the graph give -1;
                   every second-trip tile expects other values than the tile 2 048 earlier.  The third shape excludes the row itself
                   only, at max_tries = 2: a slot is exhausted there by two self-draws in a row, 1 in 36 000 000 on 6 000 vertices, so
                   20 exhausted slots cannot be had and are not asked for; instead 60 of its second-trip rows are made the candidate of
                   their slot's try 0, and at least 20 rejections of the row itself are counted;
  unique_ids       `mix`: every second-trip tile of at least 64 ids holds a first touch, a repeat of an id first seen in the first
                   trip and a -1, and every second-trip tile expects another `local` than the tile 2 048 earlier.  A tile of one id
                   (m = 524 289, 524 545) can hold one of the three: there the last id is a first touch and a repeat in turn.  `batch`,
                   the concatenation a batch makes over the 6 000-vertex graph, has seen every vertex long before index 524 288 and
                   its -1s are few (the negatives of a dead edge): its second trip is repeats of first-trip ids, with a -1 in some tiles of the
                   largest count, and that is what is asserted of it."""
import functools

import numpy as np
import pytest
import torch

from tests import link_ref as ref
from tests import node2vec_ref, walk_ref
from tests.test_gpu_link_unique import _check, ids_of

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MAX_WG = 2048                                                      # LG_WALK_MAX_WG
M31 = 2 ** 31 - 1
N = node2vec_ref.NODE_NUM


@functools.lru_cache(maxsize=None)
def graph():
    indptr, col, _ = node2vec_ref.sym_graph()
    return indptr, col


def stale_second_trip(want, stride):
    """What a kernel gives whose second trip repeats its first: entry i >= stride is entry i - stride (flat, row-major)."""
    out = np.array(want).reshape(-1).copy()
    out[stride:] = out[:out.size - stride]
    return out.reshape(np.shape(want))


# ---- find_edges -------------------------------------------------------------------------------------------------------------------
FIND_STRIDE = MAX_WG * 1024                                        # 2 048 tiles of 256 lanes x 4 edge ids
FIND_N = FIND_STRIDE + 1024 + 1                                    # tile 2 049 has one live id


def find_case():
    """(eids, reference, {name: (index, expected row, expected col)} of the ids placed by hand), the conditions checked."""
    indptr, col = graph()
    E = col.size
    eids = np.arange(FIND_N, dtype=np.int64) * 2654435761 % E
    hub = max(node2vec_ref.HUBS, key=node2vec_ref.HUBS.get)
    dead = int(np.nonzero(col < 0)[0][7])
    assert node2vec_ref.HUBS[hub] == 4097 and indptr[40] == indptr[41] == indptr[42] < indptr[43] and col[indptr[42]] >= 0
    s, e = int(indptr[hub]), int(indptr[hub + 1]) - 1
    placed = {"-1": (-1, -1, -1), "E": (E, -1, -1), "E + 5": (E + 5, -1, -1), "first of the hub": (s, hub, col[s]), "last of the hub": (e, hub, col[e]),
              "dead entry": (dead, -1, -1), "after two empty rows": (int(indptr[42]), 42, col[indptr[42]])}
    assert col[s] >= 0 and col[e] >= 0
    named = {}
    for j, (name, (eid, row, c)) in enumerate(placed.items()):
        eids[FIND_STRIDE + 1 + 3 * j] = eid                        # three apart: other lanes, the same tile
        named[name] = (FIND_STRIDE + 1 + 3 * j, row, int(c))
    reads = {}
    want = ref.find_edges(indptr, col, eids, reads=reads)
    walk_ref.assert_reads_in_bounds(reads, N, E)
    for name, (i, row, c) in named.items():
        assert (want[0][i], want[1][i]) == (row, c), name
    late = np.arange(FIND_STRIDE, FIND_N)
    same = (want[0][late] == want[0][late - FIND_STRIDE]) & (want[1][late] == want[1][late - FIND_STRIDE])
    assert late.size == 1025 and same.sum() * 100 <= late.size, f"{int(same.sum())} of {late.size} second-trip answers are those of the first trip"
    assert (FIND_N + 1023) // 1024 == MAX_WG + 2 and FIND_N % 1024 == 1
    return eids, want, named


def test_find_edges_over_one_grid_stride_and_a_bit(hip):
    from legion_amd import engine
    indptr, col = graph()
    eids, want, _ = find_case()
    g = engine.GraphStorage(1, torch.from_numpy(indptr).to(DEV), torch.from_numpy(col).to(DEV))
    try:
        got = g.find_edges(torch.from_numpy(eids).to(DEV))
        torch.cuda.synchronize()
        for name, x, w in zip(("row", "col"), got, want):
            x = x.cpu().numpy()
            assert x.dtype == np.int32 and x.shape == w.shape
            bad = np.nonzero(x != w)[0]
            assert bad.size == 0, (f"{bad.size} entries of {name} differ, {int((bad >= FIND_STRIDE).sum())} of them on a second trip; first at {bad[0]} "
                                   f"(tile {bad[0] // 1024}, eid {eids[bad[0]]}): got {x[bad[0]]} want {w[bad[0]]}")
    finally:
        torch.cuda.synchronize()
        g.close()


# ---- negative_sample --------------------------------------------------------------------------------------------------------------
NEG_STRIDE = MAX_WG * 256
NEG_SHAPES = [dict(n=8200, k=64, exclude=3, tries=3, base=0), dict(n=104909, k=5, exclude=2, tries=256, base=M31 - 104909 * 5),
              dict(n=524545, k=1, exclude=1, tries=2, base=1234567890)]
NEG_PLACED = [-1, N, 3, 4, 5, 6, 6, 6]                             # the first rows that lie wholly in the second trip
SELF_ROWS = 60                                                     # exclude 1: rows made their slot's first candidate


def negative_case(shape):
    """(rows, reference, the counters of the rows wholly in the second trip), the conditions checked."""
    indptr, col = graph()
    n, k, exclude, tries, base = (shape[x] for x in ("n", "k", "exclude", "tries", "base"))
    assert n * k > NEG_STRIDE and (n * k + 255) // 256 == MAX_WG + 2 and base + n * k <= M31
    rows = node2vec_ref.seeds_for(n).copy()
    r0 = -(-NEG_STRIDE // k)                                       # the first row with every slot in the second trip
    assert n - r0 >= len(NEG_PLACED)
    rows[r0:r0 + len(NEG_PLACED)] = NEG_PLACED
    if exclude == 1:                                               # the candidate of try 0 is what no exclusion gives
        at = np.arange(r0 + 20, r0 + 20 + SELF_ROWS)
        rows[at] = ref.negative_sample(indptr, col, np.zeros(n, dtype=np.int32), k, 0, 1, base)[at, 0]
    reads, stats = {}, ref.new_stats(N)
    want = ref.negative_sample(indptr, col, rows, k, exclude, tries, base, reads=reads)
    walk_ref.assert_reads_in_bounds(reads, N, col.size)
    late = ref.negative_sample(indptr, col, rows[r0:], k, exclude, tries, base + r0 * k, stats=stats)
    assert np.array_equal(late, want[r0:])
    if exclude & ref.EDGES:
        assert stats["hit"] >= 20 and stats["hits_of_row"][6] >= 1, stats["hit"]
        if tries <= 3:
            assert stats["exhausted"] >= 20, stats["exhausted"]
    if exclude == ref.SELF:
        assert stats["self"] >= 20 and tries == 2, stats["self"]
    assert np.all(want[r0] == -1) and np.all(want[r0 + 1] == -1) and rows[r0] == -1 and rows[r0 + 1] == N
    flat = want.reshape(-1)
    for t0 in range(NEG_STRIDE, n * k, 256):
        live = min(256, n * k - t0)
        old = t0 - NEG_STRIDE
        assert not np.array_equal(flat[t0:t0 + live], flat[old:old + live]), f"tile {t0 // 256} expects what tile {t0 // 256 - MAX_WG} does"
    return rows, want, stats


@pytest.mark.parametrize("shape", NEG_SHAPES, ids=lambda s: f"{s['n']}x{s['k']}-exclude{s['exclude']}-tries{s['tries']}")
def test_negatives_over_one_grid_stride_and_a_bit(hip, shape):
    from legion_amd import engine
    indptr, col = graph()
    rows, want, _ = negative_case(shape)
    g = engine.GraphStorage(1, torch.from_numpy(indptr).to(DEV), torch.from_numpy(col).to(DEV))
    try:
        got = g.negative_sample(torch.from_numpy(rows).to(DEV), shape["k"], exclude_self=bool(shape["exclude"] & 1),
                                exclude_edges=bool(shape["exclude"] & 2), max_tries=shape["tries"], base=shape["base"])
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        assert got.dtype == np.int32 and got.shape == want.shape
        bad = np.nonzero(got.reshape(-1) != want.reshape(-1))[0]
        assert bad.size == 0, (f"{shape}: {bad.size} negatives differ, {int((bad >= NEG_STRIDE).sum())} of them on a second trip; first at slot {bad[0]} "
                               f"(tile {bad[0] // 256}): got {got.reshape(-1)[bad[0]]} want {want.reshape(-1)[bad[0]]}")
    finally:
        torch.cuda.synchronize()
        g.close()


# ---- unique_ids -------------------------------------------------------------------------------------------------------------------
UNIQUE_STRIDE = MAX_WG * 256
UNIQUE_COUNTS = [65536, 65537, 524289, 524545, 2 ** 20 - 1]        # 256 and 257 tiles (the scan's per = 1, 2); 2 049, 2 050, 4 096 tiles
UNIQUE_KINDS = ["mix", "distinct", "batch"]
MIX_VALUES = 300000


def stride_ids(kind, m):
    if kind != "mix":
        return ids_of(kind, m)
    ids = np.random.RandomState(m % 1000 + 7).randint(0, MIX_VALUES, m).astype(np.int32)      # about 300 000 values
    ids[2::5] = -1                                                 # a fifth -1
    if m % 256 == 1:                                               # the last tile is one id: a first touch, or a repeat of the first trip's
        ids[-1] = MIX_VALUES + 1 if m % 512 == 1 else ids[5]
    return ids


def first_touches(ids):
    flag = np.zeros(ids.size, dtype=bool)
    live = np.nonzero(ids >= 0)[0]
    flag[live[np.unique(ids[live], return_index=True)[1]]] = True
    return flag


def unique_conditions(kind, ids):
    """The conditions of the module's docstring on one input; returns (first touches, repeats of first-trip ids) behind the stride."""
    m = ids.size
    want = ref.unique_ids(ids)
    if m <= UNIQUE_STRIDE:
        assert (m + 255) // 256 in (256, 257)
        return want, 0, 0
    first = first_touches(ids)
    repeat = np.zeros(m, dtype=bool)                               # behind the stride: an id the first trip has seen
    repeat[UNIQUE_STRIDE:] = (ids[UNIQUE_STRIDE:] >= 0) & np.isin(ids[UNIQUE_STRIDE:], ids[:UNIQUE_STRIDE])
    for t0 in range(UNIQUE_STRIDE, m, 256):
        sl = slice(t0, min(t0 + 256, m))
        old = slice(t0 - UNIQUE_STRIDE, sl.stop - UNIQUE_STRIDE)
        assert not np.array_equal(want[1][sl], want[1][old]), f"{kind} {m}: tile {t0 // 256} expects the local of tile {t0 // 256 - MAX_WG}"
        if kind == "mix" and sl.stop - t0 >= 64:
            assert first[sl].any() and repeat[sl].any() and (ids[sl] == -1).any(), f"mix {m}: tile {t0 // 256}"
        if kind == "batch":
            assert repeat[sl].any() and np.all(repeat[sl] | (ids[sl] == -1)), f"batch {m}: tile {t0 // 256}"
        if kind == "distinct":
            assert first[sl].all()
    if kind == "mix" and m % 256 == 1:
        assert first[-1] if m % 512 == 1 else (repeat[-1] and not first[-1])
    return want, int(first[UNIQUE_STRIDE:].sum()), int(repeat[UNIQUE_STRIDE:].sum())


@pytest.mark.parametrize("kind", UNIQUE_KINDS)
@pytest.mark.parametrize("m", UNIQUE_COUNTS)
def test_unique_ids_over_one_grid_stride_and_a_bit(hip, m, kind):
    ids = stride_ids(kind, m)
    unique_conditions(kind, ids)
    _check(ids, f"{kind} {m}")
