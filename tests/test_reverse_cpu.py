"""The reverse CSR without a GPU: the entry points in the header, the ctypes table and the library, the methods and the arguments they
refuse before they touch a device, the numpy restatement (tests/reverse_ref.py) against brute-force loops, the round-trip identities,
the figures the GPU files rely on, and the numpy models of wrong kernels differing from the reference on the GPU files' own inputs."""
import os
import re
import subprocess

import numpy as np
import pytest

from legion_amd import engine, lib
from tests import far_rows, link_ref, node2vec_ref
from tests import reverse_ref as ref
# the inputs of the GPU files come from their own builders: what is proven here is what they launch
from tests import test_gpu_reverse as gpu_main
from tests import test_gpu_reverse_far_rows as gpu_far
from tests import test_gpu_reverse_fuzz as gpu_fuzz
from tests import test_gpu_reverse_stride as gpu_stride

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "legion_hip.h")
LIB = os.path.join(ROOT, "legion_amd", "liblegion_hip.so")
NAMES = ["legion_graph_build_reverse", "legion_graph_reverse_csr"]


# ---- the entry points -----------------------------------------------------------------------------------------------------------
def test_symbols_in_header_ctypes_table_and_library():
    text = open(HEADER).read()
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NAMES:
        assert re.search(r"\bint(32|64)_t\s+" + name + r"\s*\(", text), name
    assert re.search(r"#define\s+LEGION_REVERSE_MAX_NODES\s+\(1 << 28\)", text)
    assert set(NAMES) <= exported
    c_p, c_i32, c_i64 = lib.c_p, lib.c_i32, lib.c_i64
    assert lib.SIGNATURES["legion_graph_build_reverse"][0] == c_i32 and lib.SIGNATURES["legion_graph_build_reverse"][1] == [c_p, c_p]
    assert lib.SIGNATURES["legion_graph_reverse_csr"][0] == c_i64 and len(lib.SIGNATURES["legion_graph_reverse_csr"][1]) == 4


def test_the_python_side_has_the_methods():
    for name in ("reverse", "out_degrees", "out_edges"):
        assert callable(getattr(engine.GraphStorage, name, None)), name
    assert engine.GraphStorage.REVERSE_MAX_NODES == ref.MAX_NODES == 2 ** 28


def test_a_null_graph_is_refused_without_a_device():
    L = lib.load()
    assert L.legion_graph_build_reverse(None, None) == -1
    assert L.legion_graph_reverse_csr(None, None, None, None) == -1
    assert ref.refused(False, 0) and ref.refused(True, 2 ** 28 + 1) and not ref.refused(True, 2 ** 28) and not ref.refused(True, 0)


def test_the_header_states_the_rule_and_what_is_not_offered():
    text = open(HEADER).read()
    for phrase in ("rindptr[u] = #{ live e : col[e] < u }", "ASCENDING", "rcol[p] = row(reid[p])", "must not be captured",
                   "synchronises that stream", "freed by legion_graph_destroy", "a second call returns 0 without work",
                   "N > LEGION_REVERSE_MAX_NODES", "Any\n * out-pointer may be null", "to_bidirected", "seed-edge exclusion",
                   "the reverse of a cached topology or of a partition", "heterogeneous graphs"):
        assert phrase in text, phrase


# ---- ValueErrors, without a device ----------------------------------------------------------------------------------------------
def _bare_graph(node_num=10):
    g = engine.GraphStorage.__new__(engine.GraphStorage)      # (no handle: the checks come before the library call)
    g.node_num, g.edge_num = node_num, 20
    return g


def test_argument_errors_are_value_errors_before_any_device():
    import torch
    g = _bare_graph()
    ok = np.array([1, 2, 3], dtype=np.int32)
    for method in (g.out_degrees, g.out_edges):
        with pytest.raises(ValueError, match="int32"):
            method(torch.tensor([1, 2], dtype=torch.int64))
        with pytest.raises(ValueError, match="one-dimensional"):
            method(np.zeros((2, 2), dtype=np.int32))
        with pytest.raises(ValueError, match="at most"):
            method(np.zeros(2 ** 20 + 1, dtype=np.int32))
    for flag in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="return_eids"):
            g.out_edges(ok, return_eids=flag)
    big = _bare_graph(2 ** 28 + 1)
    for call in (big.reverse, lambda: big.out_degrees(ok), lambda: big.out_edges(ok)):
        with pytest.raises(ValueError, match="at most 268435456"):
            call()


# ---- the reference against brute force ------------------------------------------------------------------------------------------
def _loop(indptr, col):
    """The definition: for every vertex the live entries that name it, in order of their positions, each with its row."""
    N = indptr.size - 1
    rindptr, rcol, reid = [0], [], []
    row = np.full(col.size, -1, dtype=np.int64)
    for v in range(N):
        row[int(indptr[v]):int(indptr[v + 1])] = v
    by = [[] for _ in range(N)]
    for e, u in enumerate(col.tolist()):
        if 0 <= u < N:
            by[u].append(e)
    for u in range(N):
        for e in by[u]:
            reid.append(e)
            rcol.append(int(row[e]))
        rindptr.append(len(reid))
    return np.array(rindptr, dtype=np.int64), np.array(rcol, dtype=np.int32), np.array(reid, dtype=np.int64)


def _against_the_loop(indptr, col, what):
    got, want = ref.reverse(indptr, col), _loop(indptr, col)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), what
    N = indptr.size - 1
    nodes = np.concatenate([np.arange(-1, N + 1), [0, 0, N - 1]]).astype(np.int32)
    src, dst, eid = ref.out_edges(indptr, col, nodes)
    k = 0
    for i, u in enumerate(nodes.tolist()):
        mine = [e for e in range(col.size) if col[e] == u] if 0 <= u < N else []
        assert eid[k:k + len(mine)].tolist() == mine and np.all(src[k:k + len(mine)] == i), (what, i)
        k += len(mine)
    assert k == eid.size and np.array_equal(dst, ref.rows_of(indptr, eid))
    assert np.array_equal(ref.out_degrees(indptr, col, nodes), np.bincount(src, minlength=nodes.size))


def test_the_reference_is_the_loop():
    for name, (indptr, col) in link_ref.small_graphs().items():
        _against_the_loop(indptr, col, name)
    _against_the_loop(*link_ref.complete_graph(), "complete")
    _against_the_loop(*link_ref.ring_graph(), "ring")
    _against_the_loop(*gpu_main.all_dead(), "all-dead")
    _against_the_loop(*ref.class_graph([0, 1, 2, 5, 9, 0, 3], 4, dead=5, outside=4), "a small class graph")
    indptr, col, _ = node2vec_ref.sym_graph()
    got, want = ref.reverse(indptr, col), _loop(indptr, col)
    for g, w in zip(got, want):
        assert np.array_equal(g, w), "sym"


# ---- the round trip ---------------------------------------------------------------------------------------------------------------
def test_the_reverse_of_the_reverse_is_the_graph():
    """On sym_graph() after dropping its 30 dead entries: N = 6 000, E = 53 418, 603 parallel pairs, reverse rows of 0 .. 4 083."""
    indptr, col, _ = node2vec_ref.sym_graph()
    assert indptr.size - 1 == 6000 and col.size == 53448 and (col < 0).sum() == 30
    indptr, col = ref.live_graph(indptr, col)
    assert col.size == 53418 and node2vec_ref.rows_sorted(indptr, col)
    rindptr, rcol, reid = ref.reverse(indptr, col)
    lengths = np.diff(rindptr)
    assert lengths.min() == 0 and lengths.max() == 4083
    pairs = rcol.astype(np.int64) * 6000 + np.repeat(np.arange(6000), lengths)
    assert pairs.size - np.unique(pairs).size == 603
    assert node2vec_ref.rows_sorted(rindptr, rcol), "every reverse row is sorted by vertex id"
    back = ref.reverse(rindptr, rcol)
    assert np.array_equal(back[0], indptr) and np.array_equal(back[1], col)
    assert np.array_equal(reid[back[2]], np.arange(col.size))
    for name in ("complete", "ring"):
        ip, c = getattr(link_ref, name + "_graph")()
        r = ref.reverse(ip, c)
        b = ref.reverse(r[0], r[1])
        assert np.array_equal(b[0], ip) and np.array_equal(b[1], c) and np.array_equal(r[2][b[2]], np.arange(c.size)), name


def test_the_live_graph_drops_what_the_reverse_drops():
    indptr, col = ref.class_graph([3, 0, 4, 1], 2, dead=6, outside=5)
    ip, c = ref.live_graph(indptr, col)
    assert c.size == 8 and ip[-1] == 8 and np.all((c >= 0) & (c < 4))
    assert np.array_equal(ref.reverse(ip, c)[0], ref.reverse(indptr, col)[0])
    assert np.array_equal(ref.reverse(ip, c)[1], ref.reverse(indptr, col)[1])


# ---- the classes ------------------------------------------------------------------------------------------------------------------
def test_the_classes_and_passes():
    T = ref.TILE
    want = {0: "none", 1: "none", 2: "wave", 64: "wave", 65: "tile", T: "tile", T + 1: "long"}
    assert {k: ref.sort_class(k) for k in want} == want
    assert [ref.runs(x) for x in (T + 1, 2 * T, 2 * T + 1, 3 * T + 5, 5 * T - 1)] == [2, 2, 3, 4, 5]
    assert [ref.passes(x) for x in (T, T + 1, 2 * T, 2 * T + 1, 3 * T + 5, 5 * T - 1, 10 ** 6)] == [0, 1, 1, 2, 2, 3, 8]
    assert [ref.scan_levels(n) for n in (0, 1, 2 ** 20, 2 ** 20 + 1, 2 ** 28)] == [0, 1, 1, 2, 2]
    assert engine.GraphStorage.IN_EDGES_MAX_ROWS == 2 ** 20


# ---- the figures the GPU files rely on ---------------------------------------------------------------------------------------------
def test_the_figures_of_the_main_file():
    made = gpu_main.graphs()
    assert set(gpu_main.FIGURES) <= set(made)
    for name, (indptr, col) in made.items():
        want = gpu_main.conditions(name, indptr, col)
        for n in (0, 1, 5, 257):
            nodes = gpu_main.seeds_for(indptr, col, n)
            assert nodes.size == n and nodes.dtype == np.int32
            if n >= 5 and name in ("classes", "sym"):
                N = indptr.size - 1
                assert (nodes == -1).sum() >= 1 and (nodes == N).sum() >= 1 and np.unique(nodes).size < n
                deg = ref.out_degrees(indptr, col, nodes)
                assert deg.max() == np.diff(want[0]).max() and (deg == 0).sum() >= 2
    indptr, col = ref.live_graph(*made["sym"])
    assert node2vec_ref.rows_sorted(indptr, col)


def test_the_figures_of_the_stride_file():
    indptr, col, want = gpu_stride.stride_case()
    print("stride: N", indptr.size - 1, "E", col.size, "live", want[2].size)
    assert want[2].size == int(gpu_stride.stride_lengths().sum())
    for N in gpu_stride.SCAN_NODES:
        indptr, col, want = gpu_stride.scan_case(N)
        print("scan", N, "live", want[2].size, "longest", int(np.diff(want[0]).max()))
    assert gpu_stride.SCAN_NODES == [2 ** 20 - 1, 2 ** 20, 2 ** 20 + 257]


def test_the_figures_of_the_far_row_file():
    for boundary in ("5000", "2^31", "2^32"):
        g = far_rows.layout(boundary)
        rindptr, rcol, reid = gpu_far.want_reverse(g)
        print(boundary, "live", reid.size, "below", int((reid < g.boundary).sum()))
        assert reid.min() >= g.offset and reid.max() < g.E
    g = far_rows.layout("5000")
    whole = np.concatenate([np.full(g.offset, -1, np.int32), g.col_ref])
    for a, b in zip(gpu_far.want_reverse(g), ref.reverse(g.indptr, whole)):
        assert np.array_equal(a, b), "the view is the whole graph"
    zeros = np.concatenate([np.zeros(g.offset, np.int32), g.col_ref])
    assert np.diff(ref.reverse(g.indptr, zeros)[0])[0] == g.offset, "a ballast of zeros makes vertex 0 a hub of every ballast entry"


def test_the_fuzz_seed_set_holds_its_conditions():
    made = {}
    gpu_fuzz.seed_set_conditions(lambda seed: made.setdefault(seed, gpu_fuzz.reverse_shape(seed)))
    assert len(made) == 24


# ---- the wrong kernels differ -------------------------------------------------------------------------------------------------------
def test_the_models_of_wrong_kernels_are_the_reference_where_they_should_be():
    indptr, col = link_ref.ring_graph()
    want = ref.reverse(indptr, col)
    for got in (ref.merge_off_by_one(indptr, col), ref.dead_kept(indptr, col), ref.e32(*want), ref.stale_second_trip(indptr, col)):
        for a, b in zip(got, want):
            assert np.array_equal(a, b), "no long row, no dead entry, no far entry, one trip: the model is the reference"
    assert np.array_equal(ref.counts_int32(want[0]), want[0])
    assert not np.array_equal(ref.counts_int32(np.array([0, 2 ** 31 + 5])), np.array([0, 2 ** 31 + 5]))
