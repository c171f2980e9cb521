"""The full-neighbour ops without a GPU: the entry points in the header, the ctypes table and the library, the arguments the Python
methods refuse before they touch a device, the numpy restatement (tests/in_edges_ref.py) against brute-force loops, the figures the GPU
files rely on, and the numpy models of wrong kernels differing from the reference on the GPU files' own inputs."""
import os
import re
import subprocess

import numpy as np
import pytest

from legion_amd import engine, lib
from tests import in_edges_ref as ref
from tests import link_ref, node2vec_ref, walk_ref
# the inputs of the GPU files come from their own builders: what is proven here is what they launch
from tests import test_gpu_in_edges as gpu_main
from tests import test_gpu_in_edges_block as gpu_block
from tests import test_gpu_in_edges_fuzz as gpu_fuzz
from tests import test_gpu_in_edges_stride as gpu_stride

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "legion_hip.h")
LIB = os.path.join(ROOT, "legion_amd", "liblegion_hip.so")
NAMES = ["legion_row_offsets_scratch_bytes", "legion_row_offsets", "legion_in_edges"]


@pytest.fixture(scope="module")
def world():
    indptr, col, _ = node2vec_ref.sym_graph()
    return {"indptr": indptr, "col": col}


# ---- the entry points -----------------------------------------------------------------------------------------------------------
def test_symbols_in_header_ctypes_table_and_library():
    text = open(HEADER).read()
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NAMES:
        assert re.search(r"\bint(32|64)_t\s+" + name + r"\s*\(", text), name
    assert re.search(r"#define\s+LEGION_IN_EDGES_MAX_ROWS\s+1048576\b", text)
    assert set(NAMES) <= exported
    c_p, c_i32, c_i64 = lib.c_p, lib.c_i32, lib.c_i64
    assert lib.SIGNATURES["legion_row_offsets_scratch_bytes"] == (c_i64, [c_i32])
    assert lib.SIGNATURES["legion_row_offsets"] == (c_i32, [c_p, c_p, c_p, c_i32, c_p, c_p, c_i64])
    assert lib.SIGNATURES["legion_in_edges"] == (c_i32, [c_p, c_p, c_p, c_i32, c_p, c_i64, c_p, c_p, c_p])


def test_the_python_side_has_the_methods():
    for name in ("row_offsets", "in_edges", "full_neighbor_block"):
        assert callable(getattr(engine.GraphStorage, name, None)), name
    assert engine.GraphStorage.IN_EDGES_MAX_ROWS == ref.MAX_ROWS


def test_null_pointers_and_illegal_counts_are_refused_without_a_device():
    L = lib.load()
    assert L.legion_row_offsets(None, None, None, 1, None, None, 8) == -1
    assert L.legion_in_edges(None, None, None, 1, None, 1, None, None, None) == -1
    for n in (-1, 0, 1, 255, 256, 257, 65537, 2 ** 20, 2 ** 20 + 1):
        assert L.legion_row_offsets_scratch_bytes(n) == ref.scratch_bytes(n), n
    assert ref.scratch_bytes(2 ** 20) == 8 * 4096 and ref.scratch_bytes(0) == 0


def test_the_header_states_the_rule_and_what_is_not_offered():
    text = open(HEADER).read()
    for phrase in ("offsets[v] <= p", "a lower bound would name the first of a run of empty rows", "memory safety does not rest on the caller's offsets",
                   "m is a capacity", "out-edges (there is no reverse CSR)", "dropping dead entries", "heterogeneous graphs"):
        assert phrase in text, phrase


# ---- ValueErrors, without a device ----------------------------------------------------------------------------------------------
def _bare_graph():
    g = engine.GraphStorage.__new__(engine.GraphStorage)      # (no handle: the checks come before the library call)
    g.node_num, g.edge_num = 10, 20
    return g


def test_argument_errors_are_value_errors_before_any_device():
    import torch
    g = _bare_graph()
    ok = np.array([1, 2, 3], dtype=np.int32)
    for method in (g.row_offsets, g.in_edges, g.full_neighbor_block):
        with pytest.raises(ValueError, match="int32"):
            method(torch.tensor([1, 2], dtype=torch.int64))
        with pytest.raises(ValueError, match="one-dimensional"):
            method(np.zeros((2, 2), dtype=np.int32))
        with pytest.raises(ValueError, match="at most"):
            method(np.zeros(2 ** 20 + 1, dtype=np.int32))
    for method in (g.in_edges, g.full_neighbor_block):
        for flag in (1, 0, None, "yes"):
            with pytest.raises(ValueError, match="return_eids"):
                method(ok, return_eids=flag)


def test_the_predicates():
    assert ref.refused("row_offsets", -1) and ref.refused("row_offsets", 2 ** 20 + 1) and not ref.refused("row_offsets", 2 ** 20)
    assert ref.refused("row_offsets", 257, scratch=15) and not ref.refused("row_offsets", 257, scratch=16) and not ref.refused("row_offsets", 0, scratch=0)
    assert ref.refused("in_edges", 5, m=-1) and ref.refused("in_edges", 5, m=2 ** 31) and not ref.refused("in_edges", 5, m=2 ** 31 - 1)
    assert ref.refused("in_edges", -1, m=5) and ref.refused("in_edges", 2 ** 20 + 1, m=5) and not ref.refused("in_edges", 0, m=0)


# ---- the reference against brute force ------------------------------------------------------------------------------------------
def _loop(indptr, col, rows, m=None):
    """The definition: the rows' entries one after another."""
    N = indptr.size - 1
    offsets, dst, src, eid = [0], [], [], []
    for i, r in enumerate(np.asarray(rows).tolist()):
        if 0 <= r < N:
            for e in range(int(indptr[r]), int(indptr[r + 1])):
                dst.append(i)
                src.append(int(col[e]))
                eid.append(e)
        offsets.append(len(dst))
    M = len(dst)
    m = M if m is None else m
    pad = lambda x: np.array((x + [-1] * max(m - M, 0))[:m])
    return np.array(offsets), pad(dst), pad(src), pad(eid)


def _against_the_loop(indptr, col, rows, what):
    reads = {}
    off = ref.row_offsets(indptr, rows, reads=reads)
    M = int(off[-1])
    for m in (M, max(M - 3, 0), M + 5):
        got = ref.in_edges(indptr, col, rows, off, m, reads=reads)
        want = _loop(indptr, col, rows, m)
        assert np.array_equal(off, want[0]), what
        for g, w in zip(got, want[1:]):
            assert np.array_equal(g, w), (what, m)
        assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[2].dtype == np.int64
    walk_ref.assert_reads_in_bounds(reads, indptr.size - 1, col.size)


def test_the_reference_is_the_loop(world):
    indptr, col = world["indptr"], world["col"]
    for n in (1, 63, 257):
        _against_the_loop(indptr, col, node2vec_ref.seeds_for(n), f"sym {n}")
    _against_the_loop(indptr, col, gpu_main.gap_rows(), "gap")
    _against_the_loop(indptr, col, gpu_main.empty_rows(), "empty")
    for name, (ip, c) in gpu_main.small_cases().items():
        _against_the_loop(ip, c, gpu_main.small_rows(ip), name)


def test_the_block_reference_is_the_loop(world):
    for name, (indptr, col, seeds) in gpu_block.graphs().items():
        b = gpu_block.block_conditions(indptr, col, seeds)
        seen = {int(v): i for i, v in enumerate(seeds.tolist())}
        for v in b["src"].tolist():
            if v >= 0 and v not in seen:
                seen[v] = len(seen)
        assert b["input_nodes"].tolist() == list(seen), name
        assert b["src_local"].tolist() == [seen.get(int(v), -1) if v >= 0 else -1 for v in b["src"].tolist()], name
    with pytest.raises(AssertionError):
        ref.full_neighbor_block(indptr, col, np.array([5, 5], dtype=np.int32))


# ---- the figures the GPU files rely on ---------------------------------------------------------------------------------------------
def test_the_figures_of_the_main_file(world):
    indptr, col = world["indptr"], world["col"]
    assert col.size == 53448 and (col < 0).sum() == 30 and (np.diff(indptr) == 0).sum() == 6 and np.diff(indptr)[6] == 4097
    for n, M in gpu_main.FIGURES.items():
        rows = gpu_main.rows_for(n)
        want = gpu_main.conditions(indptr, col, rows)
        assert int(want[0][-1]) == M, (n, int(want[0][-1]))
        if n >= 63:
            deg = ref.degrees(indptr, rows)
            inside = (rows >= 0) & (rows < node2vec_ref.NODE_NUM)
            assert (~inside).sum() == 2 and ((deg == 0) & inside).sum() >= 1 and 10 <= (rows == 6).sum() <= 50, n
    for n in gpu_main.COUNTS + ["all"]:
        gpu_main.conditions(indptr, col, gpu_main.rows_for(n))
    assert {256, 1023, 1024, 1025} <= set(gpu_main.COUNTS)
    off = ref.row_offsets(indptr, gpu_main.gap_rows())
    spans = ref.tile_ranges(off, int(off[-1]))
    print("gap: tiles", spans.size, "ranges", spans.tolist())
    assert spans.max() > 3000 > ref.STAGE and (spans <= ref.STAGE).sum() >= 2


def test_the_figures_of_the_stride_file(world):
    gpu_stride.slot_case(world["indptr"], world["col"])
    for n in gpu_stride.ROW_COUNTS:
        rows, off = gpu_stride.row_case(world["indptr"], n)
        print(n, "rows:", int(off[-1]), "slots")


def test_the_fuzz_seed_set_holds_its_conditions():
    made = {}
    gpu_fuzz.seed_set_conditions(lambda seed: made.setdefault(seed, gpu_fuzz.in_edges_shape(seed)))
    assert len(made) == 24


# ---- the wrong kernels differ -------------------------------------------------------------------------------------------------------
def test_a_lower_bound_differs(world):
    indptr, col = world["indptr"], world["col"]
    for n in (63, 257, "all"):
        rows = gpu_main.rows_for(n)
        want = ref.in_edges_full(indptr, col, rows)
        wrong = ref.in_edges_lower_bound(indptr, col, rows, want[0], int(want[0][-1]))
        bad = np.nonzero(wrong[0] != want[1])[0]
        assert bad.size >= 1 and np.all(wrong[0][bad] == -1), "the first slot of a row behind empty rows is lost"
        empty_before = np.diff(want[0])[want[1][bad] - 1] == 0
        assert np.all(empty_before)
    ip, c = link_ref.small_graphs()["ends-empty"]
    rows = gpu_main.small_rows(ip)
    want = ref.in_edges_full(ip, c, rows)
    assert not np.array_equal(ref.in_edges_lower_bound(ip, c, rows, want[0], int(want[0][-1]))[0], want[1])


def test_e_in_32_bits_and_int32_tile_sums_differ():
    """On a layout small enough for the host whose offsets are what the far-row file's are: two rows of 2^30 + 5 entries in front."""
    big = 2 ** 30 + 5
    indptr = np.array([0, big, 2 * big, 2 * big + 3, 2 * big + 3, 2 * big + 7], dtype=np.int64)

    class FarCol:                                                  # col without its 2^31 entries: zeros, the tail live
        size = int(indptr[-1])

        def __getitem__(self, e):
            return np.where(np.asarray(e) >= 2 * big, 7, 0).astype(np.int32)

    rows = np.array([2, 4, 3, 2], dtype=np.int32)
    off = ref.row_offsets(indptr, rows)
    i = np.searchsorted(off, np.arange(int(off[-1])), side="right") - 1
    want = ref._expand(indptr, FarCol(), rows, off, int(off[-1]), i)
    wrong = ref._expand(indptr, FarCol(), rows, off, int(off[-1]), i, e32=True)
    assert want[2].min() >= 2 ** 31 and np.all(want[1] == 7) and np.all(wrong[0] == -1)
    every = np.arange(5, dtype=np.int32)
    assert np.array_equal(ref.row_offsets(indptr, every), indptr)
    assert not np.array_equal(ref.row_offsets_int32_tiles(indptr, every), indptr)
    small = node2vec_ref.seeds_for(700)
    ip = node2vec_ref.sym_graph()[0]
    assert np.array_equal(ref.row_offsets_int32_tiles(ip, small), ref.row_offsets(ip, small)), "the model is the reference while sums fit"


def test_a_stale_second_trip_differs(world):
    rows, want = gpu_stride.slot_case(world["indptr"], world["col"])
    for w in want[1:]:
        stale = ref.stale_second_trip(w, ref.STRIDE)
        assert np.array_equal(stale[:ref.STRIDE], w[:ref.STRIDE]) and (stale != w).sum() >= 10 ** 6
