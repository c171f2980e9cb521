"""Seed-edge exclusion without a GPU: the entry points in the header, the ctypes table and the library, the methods and the arguments
they refuse before they touch a device, the numpy restatement (tests/exclude_ref.py) against brute-force loops, the figures the GPU
files rely on, and the numpy models of wrong kernels differing from the reference on the GPU files' own inputs."""
import os
import re
import subprocess

import numpy as np
import pytest

from legion_amd import engine, lib
from tests import exclude_ref as ref
from tests import far_rows, link_ref, node2vec_ref, reverse_ref
# the inputs of the GPU files come from their own builders: what is proven here is what they launch
from tests import test_gpu_exclude_blocks as gpu_blocks
from tests import test_gpu_exclude_far_rows as gpu_far
from tests import test_gpu_exclude_filter as gpu_filter
from tests import test_gpu_exclude_fuzz as gpu_fuzz
from tests import test_gpu_exclude_reverse_ids as gpu_ids
from tests import test_gpu_exclude_set as gpu_set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "legion_hip.h")
LIB = os.path.join(ROOT, "legion_amd", "liblegion_hip.so")
NAMES = ["legion_reverse_edge_ids", "legion_edge_set_bytes", "legion_edge_set_build", "legion_edge_set_contains",
         "legion_edge_filter_scratch_bytes", "legion_edge_filter_count", "legion_edge_filter_edges"]


# ---- the entry points -----------------------------------------------------------------------------------------------------------
def test_symbols_in_header_ctypes_table_and_library():
    text = open(HEADER).read()
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NAMES:
        assert re.search(r"\bint(32|64)_t\s+" + name + r"\s*\(", text), name
        assert name in lib.SIGNATURES, name
    assert re.search(r"#define\s+LEGION_EDGE_SET_MAX_IDS\s+2097152\b", text) and re.search(r"#define\s+LEGION_EDGE_FILTER_MAX_EDGES\s+1073741824\b", text)
    assert set(NAMES) <= exported
    c_p, c_i32, c_i64 = lib.c_p, lib.c_i32, lib.c_i64
    assert lib.SIGNATURES["legion_reverse_edge_ids"] == (c_i32, [c_p, c_p, c_p, c_i64, c_i32, c_p])
    assert lib.SIGNATURES["legion_edge_set_bytes"] == (c_i64, [c_i32]) and lib.SIGNATURES["legion_edge_filter_scratch_bytes"] == (c_i64, [c_i64])
    assert len(lib.SIGNATURES["legion_edge_filter_count"][1]) == 11 and len(lib.SIGNATURES["legion_edge_filter_edges"][1]) == 14


def test_the_python_side_has_the_methods():
    for name in ("reverse_edge_ids", "seed_edge_exclusion"):
        assert callable(getattr(engine.GraphStorage, name, None)), name
    assert callable(engine.exclude_edges) and callable(engine.EdgeIdSet.contains)
    assert engine.EDGE_SET_MAX_IDS == ref.SET_MAX_IDS == 2 ** 21 and engine.EDGE_FILTER_MAX_EDGES == ref.FILTER_MAX_EDGES == 2 ** 30
    import inspect
    for name in ("full_neighbor_block", "labor_block", "sample_distinct_block"):
        p = inspect.signature(getattr(engine.GraphStorage, name)).parameters["exclude_eids"]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY, name


def test_nulls_sizes_and_limits_are_refused_without_a_device():
    L = lib.load()
    assert L.legion_reverse_edge_ids(None, None, None, 5, 0, None) == -1
    assert L.legion_edge_set_build(None, None, 5, None, 1 << 20) == -1
    assert L.legion_edge_set_contains(None, None, 1 << 20, 5, None, 5, None) == -1
    assert L.legion_edge_filter_count(None, None, None, None, 5, None, 1 << 20, 5, None, None, 1 << 20) == -1
    assert L.legion_edge_filter_edges(None, None, None, None, 5, None, 1 << 20, 5, None, 1 << 20, 5, None, None, None) == -1
    for k in (0, 1, 128, 129, 2 ** 21, 2 ** 21 + 1, -1):
        assert L.legion_edge_set_bytes(k) == ref.set_bytes(k), k
    for m, want in ((0, 8), (1, 24), (1025, 32), (2 ** 30, 8 * (2 ** 20 + 1 + 4096)), (2 ** 30 + 1, -1), (-1, -1)):
        assert L.legion_edge_filter_scratch_bytes(m) == want, m
        assert ref.filter_refused(m, 1, 2048, want - 1) and (want < 0 or not ref.filter_refused(m, 1, 2048, want))


def test_the_header_states_the_rules_and_what_is_not_offered():
    text = open(HEADER).read()
    for phrase in ("the LEAST e' in row u", "PARALLEL EDGES ALL\n * MAP TO THE FIRST REVERSE EDGE", "via == 0", "via == 1", "bit-identical from\n * run to run",
                   "0x9E3779B97F4A7C15", "never inserted and never members", "64-bit compare-and-swap", "dst[p] >= 0 and eid[p] is not a member",
                   "an output that overlaps an input", "rank-matched pairing of parallel edges", "exclusion by vertex pair",
                   "exclude=\"reverse_types\"", "the filter inside the pool's hops or the launch group", "a whole-graph reverse-id map",
                   # the sentences earlier tests pin stay, with a note beside them
                   "a consumer masks by agg_edge_ids", "pairing an edge with its reverse edge\n * id (seed-edge exclusion)",
                   "The exclusion exists since", "The pairing exists since"):
        assert phrase in text, phrase


# ---- ValueErrors, without a device ----------------------------------------------------------------------------------------------
def _bare_graph(node_num=10):
    g = engine.GraphStorage.__new__(engine.GraphStorage)      # (no handle: the checks come before the library call)
    g.node_num, g.edge_num = node_num, 20
    return g


def test_argument_errors_are_value_errors_before_any_device():
    import torch
    g = _bare_graph()
    with pytest.raises(ValueError, match="int64"):
        g.reverse_edge_ids(torch.tensor([1, 2], dtype=torch.int32))
    with pytest.raises(ValueError, match="one-dimensional"):
        g.reverse_edge_ids(np.zeros((2, 2), dtype=np.int64))
    for bad in ("reverse", "both", "", None, 0, True, b"self", "reverse_types"):
        with pytest.raises(ValueError, match='exclude must be "self" or "reverse_id"'):
            g.seed_edge_exclusion(np.array([1, 2], dtype=np.int64), exclude=bad)
    with pytest.raises(ValueError, match="int64"):
        g.seed_edge_exclusion(torch.tensor([1, 2], dtype=torch.int32))
    with pytest.raises(ValueError, match="at most 2097152"):
        g.seed_edge_exclusion(np.zeros(2 ** 20 + 1, dtype=np.int64), exclude="reverse_id")
    with pytest.raises(ValueError, match="at most 2097152"):
        g.seed_edge_exclusion(np.zeros(2 ** 21 + 1, dtype=np.int64), exclude="self")
    with pytest.raises(ValueError, match="at most 2097152"):
        engine.EdgeIdSet(np.zeros(2 ** 21 + 1, dtype=np.int64))
    with pytest.raises(ValueError, match="int64"):
        engine.EdgeIdSet(torch.tensor([1], dtype=torch.int32))
    with pytest.raises(ValueError, match="one-dimensional"):
        engine.EdgeIdSet(np.zeros((2, 2), dtype=np.int64))
    seeds = np.array([1, 2, 3], dtype=np.int32)
    for bad in (np.array([1], dtype=np.int64), [1, 2], "self", 5, True):
        for call in (lambda: g.full_neighbor_block(seeds, exclude_eids=bad), lambda: g.labor_block(seeds, 3, exclude_eids=bad),
                     lambda: g.sample_distinct_block(seeds, 3, exclude_eids=bad)):
            with pytest.raises(ValueError, match="exclude_eids must be an EdgeIdSet"):
                call()
    # the ops' own checks still come first
    with pytest.raises(ValueError, match="return_eids"):
        g.full_neighbor_block(seeds, return_eids=1, exclude_eids=None)
    with pytest.raises(ValueError, match="fanout"):
        g.labor_block(seeds, 0, exclude_eids=None)
    d, s, e = np.zeros(3, np.int32), np.zeros(3, np.int32), np.zeros(3, np.int64)
    for bad in (None, [1], np.array([1], dtype=np.int64)):
        with pytest.raises(ValueError, match="edge_set must be an EdgeIdSet"):
            engine.exclude_edges(d, s, e, bad)
    fake = engine.EdgeIdSet.__new__(engine.EdgeIdSet)
    with pytest.raises(ValueError, match="dst must be int32"):
        engine.exclude_edges(torch.zeros(3, dtype=torch.int64), s, e, fake)
    with pytest.raises(ValueError, match="eids must be int64"):
        engine.exclude_edges(d, s, torch.zeros(3, dtype=torch.int32), fake)
    with pytest.raises(ValueError, match="one length"):
        engine.exclude_edges(d, s[:2], e, fake)
    with pytest.raises(ValueError, match="one-dimensional"):
        engine.exclude_edges(np.zeros((3, 1), np.int32), s, e, fake)


# ---- the reference against brute force ------------------------------------------------------------------------------------------
def _against_the_loop(indptr, col, what, every=1):
    ids = np.concatenate([np.arange(-2, col.size + 6, every), [col.size - 1] if col.size else []]).astype(np.int64)
    assert np.array_equal(ref.reverse_edge_ids(indptr, col, ids), ref.reverse_loop(indptr, col, ids)), what


def test_the_reverse_ids_are_the_loop():
    for name, (indptr, col) in link_ref.small_graphs().items():
        _against_the_loop(indptr, col, name)
    _against_the_loop(*link_ref.complete_graph(), "complete")
    _against_the_loop(*link_ref.ring_graph(), "ring")
    _against_the_loop(*reverse_ref.class_graph([0, 1, 2, 5, 9, 0, 3], 4, dead=5, outside=4), "a small class graph")
    indptr, col, _ = node2vec_ref.sym_graph()
    _against_the_loop(indptr, col, "sym", every=97)
    for indptr, col in (link_ref.complete_graph(), link_ref.ring_graph()):
        e = np.arange(col.size)
        rev = ref.reverse_edge_ids(indptr, col, e)
        assert (rev >= 0).all() and np.array_equal(ref.reverse_edge_ids(indptr, col, rev), e), "no parallel edges: an involution"
    loop = link_ref.small_graphs()["loop"]
    assert ref.reverse_edge_ids(*loop, [0]).tolist() == [0], "a self-loop maps to itself"


def test_the_set_and_the_filter_are_the_loops():
    rng = np.random.RandomState(5)
    members = np.concatenate([rng.randint(0, 50, 30), [-1, -3, 2 ** 32 + 4]]).astype(np.int64)
    ids = np.concatenate([np.arange(-3, 55), [2 ** 32 + 4, 4, 2 ** 33 + 4]]).astype(np.int64)
    inside = {int(x) for x in members if x >= 0}
    assert ref.contains(members, ids).tolist() == [int(int(x) in inside) for x in ids]
    dst = np.array([0, 0, 1, -1, 2, 2, -1], dtype=np.int32)
    src = np.array([5, -1, 6, 7, -1, 8, -1], dtype=np.int32)
    eid = np.array([10, 11, 12, 13, 14, 15, -1], dtype=np.int64)
    d, s, e, K = ref.exclude_edges(dst, src, eid, [11, 15, -1], cap=6)
    assert K == 3 and d.tolist() == [0, 1, 2, -1, -1, -1] and s.tolist() == [5, 6, -1, -1, -1, -1] and e.tolist() == [10, 12, 14, -1, -1, -1]
    assert ref.exclude_edges(dst, src, eid, [11, 15, -1], cap=2)[0].tolist() == [0, 1]
    assert ref.exclude_edges(dst, src, eid, [])[3] == 5 and ref.exclude_edges(dst, src, eid, eid)[3] == 0


def test_the_homes_invert():
    for k, homes in ((300, [77, 1023, 0]), (2 ** 21, [0, 2 ** 22 - 1, 12345])):
        ids = ref.ids_with_home(k, homes, 5)
        assert np.array_equal(ref.home_slots(ids, k), np.repeat(homes, 5)) and (ids >= 0).all()
    far = ref.ids_with_home(300, [9], 40, high=2 ** 32)
    assert far.min() >= 2 ** 32 and np.unique(ref.home_slots_hash32(far, 300)).size > 10


# ---- the figures the GPU files rely on ---------------------------------------------------------------------------------------------
def test_the_issues_figures():
    indptr, col, _ = node2vec_ref.sym_graph()
    assert ref.figures(indptr, col) == gpu_ids.SYM_FIGURES
    assert gpu_ids.SYM_FIGURES == dict(entries=53448, live=53418, no_reverse=29, loops=856, loops_fixed=856, not_involution=603, longest=4097)
    indptr, col, _, _ = far_rows.live_graph()
    assert ref.figures(indptr, col) == gpu_far.LIVE_FIGURES
    assert gpu_far.LIVE_FIGURES == dict(entries=10065, live=10059, no_reverse=6, loops=141, loops_fixed=141, not_involution=110, longest=513)
    assert node2vec_ref.rows_sorted(indptr, col)


def test_the_figures_of_the_reverse_id_file():
    for build, cond in ((gpu_ids.sym, gpu_ids.sym_conditions), (gpu_ids.directed, gpu_ids.directed_conditions)):
        indptr, col = build()
        ids, want = cond(indptr, col)
        assert ids.size == col.size + 3
        for n in gpu_ids.SIZES:
            assert gpu_ids.ids_for(indptr, col, n).size == n
    assert gpu_ids.SIZES == [0, 1, 255, 256, 257, 1023, 1024, 1025] and gpu_ids.STRIDE_N == 2048 * 1024 + 1025
    ids, want = gpu_ids.stride_case()
    assert ids.size == gpu_ids.STRIDE_N


def test_the_figures_of_the_set_file():
    assert gpu_set.SIZES == [0, 1, 128, 129, 2 ** 21]
    for k in gpu_set.SIZES:
        members = gpu_set.members_for(k)
        assert members.size == k
        gpu_set.conditions(members, gpu_set.queries_for(members))
    members, longest, wraps = gpu_set.clustered()
    print("clustered: longest probe run", longest, "wraps", wraps)


def test_the_figures_of_the_filter_file():
    assert gpu_filter.SIZES == [0, 1, 1023, 1024, 1025, 256 * 1024 + 1] and gpu_filter.STRIDE_M == 2048 * 1024 + 1025
    for m in gpu_filter.SIZES[:-1]:
        dst, src, eid = gpu_filter.edge_list(m, seed=m % 97)
        gpu_filter.conditions(dst, src, eid, gpu_filter.members_for(eid, "some") if m else np.array([3, 4], dtype=np.int64))
    dst, src, eid = gpu_filter.edge_list(5000, seed=21, tail=700)
    members = gpu_filter.members_for(eid, "some", seed=22)
    K = ref.exclude_edges(dst, src, eid, members)[3]
    want = ref.exclude_edges(dst, src, eid, members, K + 2500)
    wrong = ref.exclude_tail_unfilled(dst, src, eid, members, K + 2500, gpu_filter.POISON)
    assert not np.array_equal(wrong[0], want[0]) and np.array_equal(wrong[0][:K], want[0][:K])


def test_the_figures_of_the_far_row_file():
    for boundary in ("5000", "2^31", "2^32"):
        g = far_rows.layout(boundary)
        ids, want = gpu_far.want_reverse_ids(g)
        gpu_far.set_case(g, ids, want)
        wrong = ref.reverse_e32(g.indptr_ref, g.col_ref, np.arange(g.live_E))
        assert np.array_equal(wrong, ref.reverse_edge_ids(g.indptr_ref, g.col_ref, np.arange(g.live_E))), "the view itself is small"
    g = far_rows.layout("5000")
    whole = np.concatenate([np.full(g.offset, -1, np.int32), g.col_ref])
    ids, want = gpu_far.want_reverse_ids(g)
    assert np.array_equal(ref.reverse_edge_ids(g.indptr, whole, ids), want), "the view is the whole graph"


def test_the_figures_of_the_block_file():
    indptr, col, eids, seeds = gpu_blocks.seed_edges()
    made = gpu_blocks.conditions(indptr, col, eids, seeds)
    assert len(made) == 9


def test_the_fuzz_seed_set_holds_its_conditions():
    made = {}
    gpu_fuzz.seed_set_conditions(lambda seed: made.setdefault(seed, gpu_fuzz.shape(seed)))
    assert len(made) == 24


# ---- the wrong kernels differ -------------------------------------------------------------------------------------------------------
def test_the_models_of_wrong_kernels_are_the_reference_where_they_should_be():
    indptr, col = link_ref.ring_graph()
    e = np.arange(-1, col.size + 1)
    want = ref.reverse_edge_ids(indptr, col, e)
    for got in (ref.reverse_first_probed(indptr, col, e), ref.reverse_dead_given(indptr, col, e), ref.reverse_e32(indptr, col, e),
                ref.stale_second_trip(want, ref.IDS_STRIDE)):
        assert np.array_equal(got, want), "no parallel edge, no dead entry, no far entry, one trip: the model is the reference"
    members = np.array([7, 21, 7 * 2 ** 10], dtype=np.int64)
    q = np.arange(0, 2 ** 21, 7, dtype=np.int64)
    assert np.array_equal(ref.contains_key32(members, q), ref.contains(members, q)), "no id past 2^32: the 32-bit key is right"
    assert not np.array_equal(ref.contains_key32(members, q + 2 ** 32), ref.contains(members, q + 2 ** 32))
    dst, src, eid = gpu_filter.edge_list(900, seed=1)
    mem = gpu_filter.members_for(eid, "none")
    for a, b in zip(ref.exclude_unstable(dst, src, eid, mem)[:3], ref.exclude_edges(dst, src, eid, mem)[:3]):
        assert not np.array_equal(a, b), "one tile reversed"
    assert np.array_equal(ref.exclude_tail_unfilled(dst, src, eid, mem, 900)[0], ref.exclude_edges(dst, src, eid, mem, 900)[0]), "cap == K: no tail"
