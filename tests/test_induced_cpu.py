"""A vertex set and induced subgraphs without a GPU: the entry points in the header, the ctypes table and the library, the arguments the
Python side refuses before it touches a device, the numpy restatement (tests/induced_ref.py) against brute-force Python loops on the
symmetric graph and the small graphs, the figures the GPU files rely on, and the numpy models of wrong kernels differing from the
reference on the GPU files' own inputs."""
import os
import re
import subprocess

import numpy as np
import pytest

from legion_amd import engine, lib
from tests import in_edges_ref
from tests import induced_ref as ref
from tests import far_rows, link_ref, node2vec_ref, walk_ref
# the inputs of the GPU files come from their own builders: what is proven here is what they launch
from tests import test_gpu_induced as gpu_main
from tests import test_gpu_induced_far_rows as gpu_far
from tests import test_gpu_induced_fuzz as gpu_fuzz
from tests import test_gpu_induced_stride as gpu_stride
from tests import test_gpu_node_set as gpu_set
from tests import test_gpu_node_subgraph as gpu_sub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "legion_hip.h")
LIB = os.path.join(ROOT, "legion_amd", "liblegion_hip.so")
NAMES = ["legion_node_set_bytes", "legion_node_set_build", "legion_node_set_lookup", "legion_induced_scratch_bytes", "legion_induced_count",
         "legion_induced_edges", "legion_dst_offsets"]


@pytest.fixture(scope="module")
def world():
    indptr, col, _ = node2vec_ref.sym_graph()
    return {"indptr": indptr, "col": col, "table": gpu_main.table(indptr, col)}


# ---- the entry points -----------------------------------------------------------------------------------------------------------
def test_symbols_in_header_ctypes_table_and_library():
    text = open(HEADER).read()
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NAMES:
        assert re.search(r"\bint(32|64)_t\s+" + name + r"\s*\(", text), name
    assert re.search(r"#define\s+LEGION_NODE_SET_MAX_IDS\s+1048576\b", text) and re.search(r"#define\s+LEGION_INDUCED_MAX_SLOTS\s+1073741824\b", text)
    assert set(NAMES) <= exported
    c_p, c_i32, c_i64 = lib.c_p, lib.c_i32, lib.c_i64
    assert lib.SIGNATURES["legion_node_set_bytes"] == (c_i64, [c_i32])
    assert lib.SIGNATURES["legion_node_set_build"] == (c_i32, [c_p, c_p, c_i32, c_p, c_i64, c_p])
    assert lib.SIGNATURES["legion_node_set_lookup"] == (c_i32, [c_p, c_p, c_i64, c_i32, c_p, c_i64, c_p])
    assert lib.SIGNATURES["legion_induced_scratch_bytes"] == (c_i64, [c_i64])
    assert lib.SIGNATURES["legion_induced_count"] == (c_i32, [c_p, c_p, c_p, c_i32, c_p, c_i64, c_p, c_i64, c_i32, c_p, c_p, c_i64])
    assert lib.SIGNATURES["legion_induced_edges"] == (c_i32, [c_p, c_p, c_p, c_i32, c_p, c_i64, c_p, c_i64, c_i32, c_p, c_i64, c_i64, c_p, c_p, c_p])
    assert lib.SIGNATURES["legion_dst_offsets"] == (c_i32, [c_p, c_p, c_i64, c_p, c_i32, c_p])


def test_the_python_side_has_the_class_and_the_methods():
    assert callable(getattr(engine, "NodeSet", None)) and callable(getattr(engine.NodeSet, "lookup", None))
    for name in ("induced_edges", "node_subgraph"):
        assert callable(getattr(engine.GraphStorage, name, None)), name
    doc = engine.GraphStorage.node_subgraph.__doc__
    for phrase in ("ClusterGCN", "GraphSAINT", "ShaDow-GNN", "GraphStorage(1, indptr_sub, col_sub)", "subgraph.edata[dgl.EID]", "sorted rows stay\n        sorted"):
        assert phrase in doc, phrase
    assert "twice" in engine.GraphStorage.induced_edges.__doc__
    assert engine.NODE_SET_MAX_IDS == ref.MAX_IDS


def test_null_pointers_and_illegal_counts_are_refused_without_a_device():
    L = lib.load()
    assert L.legion_node_set_build(None, None, 1, None, 1 << 20, None) == -1
    assert L.legion_node_set_lookup(None, None, 1 << 20, 1, None, 1, None) == -1
    assert L.legion_induced_count(None, None, None, 1, None, 1, None, 1 << 20, 1, None, None, 1 << 20) == -1
    assert L.legion_induced_edges(None, None, None, 1, None, 1, None, 1 << 20, 1, None, 1 << 20, 1, None, None, None) == -1
    assert L.legion_dst_offsets(None, None, 1, None, 1, None) == -1
    for m in (-1, 0, 1, 1024, 1025, 262144, 262145, 2 ** 30, 2 ** 30 + 1):
        assert L.legion_induced_scratch_bytes(m) == ref.scratch_bytes(m), m
    for k in (-1, 0, 1, 127, 128, 129, 3000, 2 ** 19, 2 ** 19 + 1, 2 ** 20, 2 ** 20 + 1):
        assert L.legion_node_set_bytes(k) == ref.set_bytes(k), k
    assert ref.set_bytes(2 ** 20) == 2 ** 24 and ref.set_bytes(0) == 2048 and ref.scratch_bytes(2 ** 30) == 8 * (2 ** 20 + 1 + 4096)


def test_the_header_states_the_rule_and_what_is_not_offered():
    text = open(HEADER).read()
    for phrase in ("pos(v) = min{ j : nodes[j] == v }", "Negative entries of nodes are members of nothing", "int32 keys[S] then uint32 first[S]",
                   "2654435769u", "an empty key is\n * all-ones", "pos and the count do not", "v >= 0 is tested before any probe",
                   "accepted only if it lies in [0, k)", "Memory safety does not rest on what the set holds", "rows and the set are independent",
                   "dead entries never are", "It is a lower-bound search over dst[0 .. L) and nothing\n * else", "edge_subgraph", "out-edges",
                   "khop_in_subgraph", "heterogeneous graphs", "nodes[src_local], one gather"):
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
    many = np.zeros(2 ** 20 + 1, dtype=np.int32)
    with pytest.raises(ValueError, match="int32"):
        g.induced_edges(torch.tensor([1, 2], dtype=torch.int64), ok)
    with pytest.raises(ValueError, match="int32"):
        g.induced_edges(ok, torch.tensor([1, 2], dtype=torch.int64))
    with pytest.raises(ValueError, match="one-dimensional"):
        g.induced_edges(np.zeros((2, 2), dtype=np.int32), ok)
    with pytest.raises(ValueError, match="one-dimensional"):
        g.induced_edges(ok, np.zeros((2, 2), dtype=np.int32))
    with pytest.raises(ValueError, match="rows in one call, at most"):
        g.induced_edges(many, ok)
    with pytest.raises(ValueError, match="nodes in one call, at most"):
        g.induced_edges(ok, many)
    for method in (g.node_subgraph, engine.NodeSet):
        with pytest.raises(ValueError, match="int32"):
            method(torch.tensor([1, 2], dtype=torch.int64))
        with pytest.raises(ValueError, match="one-dimensional"):
            method(np.zeros((2, 2), dtype=np.int32))
        with pytest.raises(ValueError, match="at most 1048576"):
            method(many)
    for flag in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="return_eids"):
            g.induced_edges(ok, ok, return_eids=flag)
        with pytest.raises(ValueError, match="return_eids"):
            g.node_subgraph(ok, return_eids=flag)


def test_the_predicates():
    assert ref.refused("build", k=-1) and ref.refused("build", k=2 ** 20 + 1) and not ref.refused("build", k=2 ** 20)
    assert ref.refused("build", k=129, set_b=2048) and not ref.refused("build", k=128, set_b=2048)
    assert ref.refused("lookup", k=5, m=-1) and ref.refused("lookup", k=5, m=2 ** 31) and not ref.refused("lookup", k=5, m=2 ** 31 - 1)
    assert ref.refused("count", -1, 5, 5) and ref.refused("count", 2 ** 20 + 1, 5, 5) and not ref.refused("count", 2 ** 20, 2 ** 30, 2 ** 20)
    assert ref.refused("count", 5, -1, 5) and ref.refused("count", 5, 2 ** 30 + 1, 5) and ref.refused("count", 5, 5, -1)
    assert ref.refused("count", 5, 1025, 5, scratch=31) and not ref.refused("count", 5, 1025, 5, scratch=32)
    assert ref.refused("edges", 5, 5, 5, cap=-1) and ref.refused("edges", 5, 5, 5, cap=2 ** 31) and not ref.refused("edges", 5, 5, 5, cap=2 ** 31 - 1)
    assert ref.refused("dst_offsets", n=-1) and ref.refused("dst_offsets", n=2 ** 20 + 1) and ref.refused("dst_offsets", cap=2 ** 31)
    assert not ref.refused("dst_offsets", n=2 ** 20, cap=2 ** 31 - 1)


# ---- the reference against brute force ------------------------------------------------------------------------------------------
def _loop(indptr, col, rows, nodes, m=None):
    """The definition in Python: the rows' entries one after another, the first m slots looked at."""
    N = indptr.size - 1
    nodes = np.asarray(nodes).tolist()
    dst, local, eid, p = [], [], [], 0
    for i, r in enumerate(np.asarray(rows).tolist()):
        if 0 <= r < N:
            for e in range(int(indptr[r]), int(indptr[r + 1])):
                t = int(col[e])
                if (m is None or p < m) and t >= 0 and t in nodes:
                    dst.append(i)
                    local.append(nodes.index(t))
                    eid.append(e)
                p += 1
    return np.array(dst, dtype=np.int64), np.array(local, dtype=np.int64), np.array(eid, dtype=np.int64)


def _against_the_loop(indptr, col, rows, nodes, what):
    off = in_edges_ref.row_offsets(indptr, rows)
    M = int(off[-1])
    for m in (M, max(M - 3, 0), M // 2):
        reads = {}
        K, dst, local, eid = ref.edges(indptr, col, rows, off, m, nodes, reads=reads)
        want = _loop(indptr, col, rows, nodes, m)
        assert K == want[0].size == ref.count(indptr, col, rows, off, m, nodes)
        for g, w in zip((dst, local, eid), want):
            assert np.array_equal(g, w), (what, m)
        assert dst.dtype == np.int32 and local.dtype == np.int32 and eid.dtype == np.int64
        walk_ref.assert_reads_in_bounds(reads, indptr.size - 1, col.size)
        capped = ref.edges(indptr, col, rows, off, m, nodes, cap=K + 5)
        assert capped[0] == K and np.array_equal(capped[1][:K], dst) and np.all(capped[1][K:] == -1) and np.all(capped[3][K:] == -1)
        if K:
            assert np.array_equal(ref.edges(indptr, col, rows, off, m, nodes, cap=K - 1)[2], local[:K - 1])
        n = np.asarray(rows).size
        ptr = ref.dst_offsets(dst, K, K, n)
        assert ptr.tolist() == [sum(1 for d in dst.tolist() if d < i) for i in range(n + 1)], what


def test_pos_is_the_definition():
    nodes = np.array([5, 9, 5, -1, 0, 9, 2 ** 31 - 1, -7, 0], dtype=np.int32)
    asked = np.array([5, 9, 0, -1, -7, 2 ** 31 - 1, 4, 6000], dtype=np.int32)
    assert ref.pos(nodes, asked).tolist() == [0, 1, 4, -1, -1, 6, -1, -1]
    assert ref.pos(nodes, asked, last=True).tolist() == [2, 5, 8, -1, -1, 6, -1, -1]
    assert ref.distinct(nodes) == 4 and ref.distinct(np.zeros(0, np.int32)) == 0 and ref.pos(np.zeros(0, np.int32), asked).tolist() == [-1] * 8
    assert ref.pos(nodes, np.zeros(0, np.int32)).shape == (0,)


def test_the_reference_is_the_loop(world):
    indptr, col = world["indptr"], world["col"]
    half = gpu_main.half_set()
    sets = {"eight": gpu_main.EIGHT, "repeats": np.concatenate([half[:60], half[:30], [-1, 6000, 6005]]).astype(np.int32), "none": np.zeros(0, np.int32)}
    for n in (1, 63, 257):
        for what, nodes in sets.items():
            _against_the_loop(indptr, col, node2vec_ref.seeds_for(n), nodes, f"sym {n} {what}")
    _against_the_loop(indptr, col, gpu_main.gap_rows(), sets["repeats"], "gap")
    _against_the_loop(indptr, col, gpu_main.empty_rows(), sets["eight"], "empty")
    for name, (ip, c) in gpu_main.small_cases().items():
        n = ip.size - 1
        for nodes in (np.arange(n), np.concatenate([[n + 3, -1], np.arange(n)[::-1], [n]]), np.arange(0, n, 2), np.array([0, 0])):
            _against_the_loop(ip, c, gpu_main.small_rows(ip), nodes.astype(np.int32), name)


def test_the_subgraph_reference_is_the_loop():
    for name, (indptr, col, nodes) in gpu_sub.graphs().items():
        if nodes.size > 2100:
            nodes = nodes[:300]
        indptr_sub, col_sub, eids = ref.node_subgraph(indptr, col, nodes)
        dst, local, eid = _loop(indptr, col, nodes, nodes)
        assert np.array_equal(col_sub, local) and np.array_equal(eids, eid), name
        assert np.array_equal(np.repeat(np.arange(nodes.size), np.diff(indptr_sub)), dst), name
    with pytest.raises(AssertionError):
        ref.node_subgraph(indptr, col, np.array([5, 5], dtype=np.int32))
    with pytest.raises(AssertionError):
        ref.node_subgraph(indptr, col, np.array([5, -1], dtype=np.int32))


def test_dst_offsets_is_the_definition():
    dst = np.array([0, 0, 2, 2, 2, 5, 9, 9], dtype=np.int32)
    assert ref.dst_offsets(dst, 8, 8, 10).tolist() == [0, 2, 2, 5, 5, 5, 6, 6, 6, 6, 8]
    assert ref.dst_offsets(dst, 8, 8, 10, upper=True).tolist() == [2, 2, 5, 5, 5, 6, 6, 6, 6, 8, 8]
    assert ref.dst_offsets(dst, 8, 3, 3).tolist() == [0, 2, 2, 3] and ref.dst_offsets(dst, 5, 2 ** 40, 3).tolist() == [0, 2, 2, 5]
    assert ref.dst_offsets(dst, 8, -4, 2).tolist() == [0, 0, 0] and ref.dst_offsets(dst[:0], 0, 0, 0).tolist() == [0]


# ---- the figures the GPU files rely on, and the wrong kernels differing -------------------------------------------------------------
def test_the_figures_of_the_table(world):
    """The table of cases: rows, set, M, K and what each case gives; conditions() asserts the figures and that the wrong models --
    the last position, no wrap, a dead entry matched, dst's membership, the global source, lane-major ranks -- differ where they should."""
    indptr, col = world["indptr"], world["col"]
    assert col.size == 53448 and int((col < 0).sum()) == 30 and indptr.size - 1 == 6000
    seen = {}
    for name in gpu_main.CASES:
        rows, nodes, M, K = world["table"][name]
        out = gpu_main.conditions(name, indptr, col, rows, nodes, M, K)
        seen[name] = (out[1], out[3])
    assert [seen[n] for n in ("third", "identity", "hubs", "shuffled", "eight-of-all", "eight", "repeats")] == \
        [(20560, 7956), (53448, 53418), (39387, 29794), (28647, 15475), (53448, 4934), (4953, 26), (53448, 8147)]
    assert [seen[f"rows-{n}"][1] for n in gpu_main.COUNTS] == [2063, 23399, 21346, 23409, 104528, 104534, 422849, 420798, 422861]
    assert seen["rows-1"][0] == 4097 and seen["rows-1025"][0] == 839294
    gpu_main.prefix_case(indptr, col)
    assert len(list(gpu_main.offsets_cases(indptr, col))) == 3              # asserts that an upper-bound dst_offsets differs


def test_the_wrap_input(world):
    nodes, last = ref.wrap_set()
    assert nodes.size == 100 and last.size == 46 and last[:4].tolist() == [144, 288, 377, 521] and np.unique(nodes).size == 100
    assert np.all(link_ref.home_slots(last, 100) >= 254) and np.all(link_ref.home_slots(nodes[46:], 100) < 254)
    runs = []
    for order in (np.arange(100), np.arange(100)[::-1]):
        _, longest, wraps = link_ref.probe_table(nodes, 100, order)
        runs.append(longest)
        assert wraps == 44 and len(ref.lost_without_wrap(nodes, order)) == 44
    assert sorted(runs) == [49, 58]
    assert np.isin(last, world["col"]).all(), "all 46 are sources of some entry"


def test_the_conditions_of_the_other_gpu_files():
    gpu_set.test_the_inputs_hold_their_conditions_before_any_launch()
    gpu_stride.test_the_cases_hold_their_conditions_before_any_launch()     # asserts that a stale second trip differs
    gpu_sub.test_the_inputs_hold_their_conditions_before_any_launch()
    for name in far_rows.BOUNDARIES:                                        # asserts that e in 32 bits differs at the far boundaries
        g = far_rows.layout(name)
        for with_zero in (False, True):
            gpu_far.want_induced(g, with_zero)


def test_e_in_32_bits_differs_on_a_far_layout_and_not_on_the_small_graph(world):
    indptr, col = world["indptr"], world["col"]
    rows, nodes = world["table"]["third"][:2]
    off = in_edges_ref.row_offsets(indptr, rows)
    want = ref.edges(indptr, col, rows, off, int(off[-1]), nodes)
    wrong = ref.edges(indptr, col, rows, off, int(off[-1]), nodes, wrong="e32")
    assert all(np.array_equal(a, b) for a, b in zip(want[1:], wrong[1:])), "below 2^31 the model is the reference"


def test_the_fuzz_seed_set_holds_its_conditions():
    made = {}
    gpu_fuzz.seed_set_conditions(lambda seed: made.setdefault(seed, gpu_fuzz.induced_shape(seed)))
    assert len(made) == 24
