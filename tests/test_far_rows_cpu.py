"""The stand-in trick of tests/far_rows.py is the reference: at boundary 5000, where the host holds the whole graph, every reference run
on the whole arrays (ballast included) gives what it gives on the reference view -- traces, neighbours, counts and batches equal, edge ids
equal after adding `offset` -- and no read touches a ballast row.  The conditions every GPU test repeats (edge ids on both sides of the
boundary, the straddling row left to both sides, a node2vec row search beyond it, a PinSAGE seed whose walks cross it) are asserted
inside far_rows' want_* functions, here at every boundary: they need the view alone, so none needs a GPU."""
import numpy as np
import pytest

from tests import far_rows, node2vec_ref, weighted_ref
from tests.helpers import KEYS_EXACT


@pytest.fixture(scope="module")
def g():
    return far_rows.layout("5000")


def _pair(fn, case, with_reads=True):
    """fn(*case) on the view and on the whole graph, with their reads."""
    g = fn.__self__
    reads_view, reads_whole = {}, {}
    a = fn(*case, reads=reads_view) if with_reads else fn(*case)
    b = fn(*case, reads=reads_whole, whole=True) if with_reads else fn(*case, whole=True)
    if with_reads:
        assert reads_view and reads_whole
        g.assert_no_ballast_read(reads_view, view=True)
        g.assert_no_ballast_read(reads_whole)
    return a, b


def test_the_layout(g):
    """The ballast is what the docstring says, at every boundary; the whole graph at 5000 is a sorted CSR whose tail is the view's."""
    for name, (boundary, L) in far_rows.BOUNDARIES.items():
        f = far_rows.layout(name)
        assert f.boundary == boundary and f.L == L and f.indptr.size == f.node_num + 1 and f.E > boundary
        assert f.indptr[f.hub] < boundary < f.indptr[f.hub + 1] and f.deg[f.hub] == far_rows.LIVE_HUBS[far_rows.STRADDLER]
        assert np.array_equal(f.indptr[f.B:] - f.offset, f.indptr_ref[f.B:]) and not f.indptr_ref[:f.B + 1].any()
    assert far_rows.layout("2^32").B == 4096 and far_rows.layout("2^31").B == 2048
    indptr, col, w = g.full()
    assert col.size == w.size == g.E and not col[:g.offset].any() and np.all(w[:g.offset] == 1)
    assert node2vec_ref.rows_sorted(indptr, col) and node2vec_ref.rows_sorted(g.indptr_ref, g.col_ref)
    table = weighted_ref.cdf(indptr, w)
    assert np.array_equal(table[g.offset:].view(np.uint32), g.table_ref.view(np.uint32))
    first = np.arange(1, g.L + 1, dtype=np.float32)                                 # a full ballast row's table is 1 .. L
    assert np.array_equal(table[:g.L], first) and np.array_equal(table[(g.B - 2) * g.L:(g.B - 1) * g.L], first)
    live = g.col_ref
    assert (live == -1).sum() >= 3 and (np.diff(g.indptr_ref[g.B:]) == 0).sum() >= 3                      # dead entries, empty rows
    zero = g.vertex(node2vec_ref.ZERO_ROW)
    assert g.deg[zero] > 0 and not g.table_ref[g.indptr_ref[zero]:g.indptr_ref[zero + 1]].any()      # an all-zero-weight row
    assert np.array_equal(g.w_ref * 8, np.round(g.w_ref * 8))                                        # eighths: the table is unique


def test_seeds_are_live(g):
    for n in (257, 5000):
        s = g.seeds(n)
        assert (s == -1).sum() == 1 and (s == g.node_num).sum() == 1 and (s == g.hub).sum() >= n // 6
    ids, labels = g.train_ids()
    assert np.array_equal(np.sort(ids), np.arange(g.B, g.node_num)) and g.hub in ids[:far_rows.SAMPLER_BATCH]


@pytest.mark.parametrize("case", far_rows.WALK_CASES, ids=str)
def test_walk(g, case):
    (ta, ea), (tb, eb) = _pair(g.want_walk, case)
    assert np.array_equal(ta, tb) and np.array_equal(ea, eb)


@pytest.mark.parametrize("case", far_rows.NODE2VEC_CASES, ids=str)
def test_node2vec(g, case):
    (ta, ea), (tb, eb) = _pair(g.want_node2vec, case)
    assert np.array_equal(ta, tb) and np.array_equal(ea, eb)


@pytest.mark.parametrize("case", far_rows.PINSAGE_CASES, ids=str)
def test_pinsage(g, case):
    (na, ca), (nb, cb) = _pair(g.want_pinsage, case)
    assert np.array_equal(na, nb) and np.array_equal(ca, cb) and (ca > 0).any()


def test_weighted_picks(g):
    a, b = _pair(g.want_picks, (), with_reads=False)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("fanout", far_rows.SAMPLER_SHAPES, ids=str)
@pytest.mark.parametrize("mode", far_rows.SAMPLER_MODES)
def test_sampler_batches(g, mode, fanout):
    """The first, second and last (clamped) batch; the view's and the whole graph's agree on every key, edge ids included."""
    n_batches = -(-g.n // far_rows.SAMPLER_BATCH)
    for it in (0, 1, n_batches - 1):
        a, b = _pair(g.want_batch, (mode, it, far_rows.SAMPLER_BATCH, fanout), with_reads=False)
        for key in KEYS_EXACT + ["agg_edge_ids"]:
            assert np.array_equal(a[key], b[key]), (it, key)
        dst = a["agg_dst_ids"].astype(np.int64)
        assert dst.min() >= g.B                                                                      # no ballast row is sampled for


@pytest.mark.parametrize("name", ["2^31", "2^32"])
def test_the_conditions_hold_at_the_large_boundaries(name):
    """What the GPU tests assert before they launch, from the view alone (the live graph is the same; the vertex ids move with B)."""
    f = far_rows.layout(name)
    for case in far_rows.WALK_CASES[:4]:
        traces, eids = f.want_walk(*case)
        assert eids.max() >= f.boundary > eids[eids >= 0].min() >= f.offset
    f.want_node2vec(*far_rows.NODE2VEC_CASES[0])
    f.want_pinsage(*far_rows.PINSAGE_CASES[-1])
    f.want_picks()
    for mode in far_rows.SAMPLER_MODES:
        f.want_batch(mode, 0, far_rows.SAMPLER_BATCH, [25, 10])
