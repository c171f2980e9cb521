"""Layer-neighbour sampling without a GPU: the entry points in the header, the ctypes table and the library, the arguments the Python
methods refuse before they touch a device, the numpy restatement (tests/labor_ref.py) against brute-force Python loops, the identity at
large fan-outs, monotonicity in the fan-out, the uniformity and independence of the hash as conditions, the figures the GPU files rely
on, and the numpy models of wrong kernels differing from the reference on the GPU files' own inputs."""
import os
import re
import subprocess

import numpy as np
import pytest

from legion_amd import engine, lib
from tests import in_edges_ref
from tests import labor_ref as ref
from tests import link_ref, node2vec_ref, walk_ref
# the inputs of the GPU files come from their own builders: what is proven here is what they launch
from tests import test_gpu_labor as gpu_main
from tests import test_gpu_labor_block as gpu_block
from tests import test_gpu_labor_fuzz as gpu_fuzz
from tests import test_gpu_labor_stride as gpu_stride

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "legion_hip.h")
LIB = os.path.join(ROOT, "legion_amd", "liblegion_hip.so")
NAMES = ["legion_labor_scratch_bytes", "legion_labor_count", "legion_labor_edges"]


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
    assert re.search(r"#define\s+LEGION_LABOR_MAX_SLOTS\s+1073741824\b", text)
    assert set(NAMES) <= exported
    c_p, c_i32, c_i64 = lib.c_p, lib.c_i32, lib.c_i64
    assert lib.SIGNATURES["legion_labor_scratch_bytes"] == (c_i64, [c_i64])
    assert lib.SIGNATURES["legion_labor_count"] == (c_i32, [c_p, c_p, c_p, c_i32, c_p, c_i64, c_i32, c_i64, c_p, c_p, c_i64])
    assert lib.SIGNATURES["legion_labor_edges"] == (c_i32, [c_p, c_p, c_p, c_i32, c_p, c_i64, c_i32, c_i64, c_p, c_i64, c_i64, c_p, c_p, c_p])


def test_the_python_side_has_the_methods():
    for name in ("labor_edges", "labor_block"):
        assert callable(getattr(engine.GraphStorage, name, None)), name
        doc = getattr(engine.GraphStorage, name).__doc__
        assert "The same salt for every layer" in doc and "a new salt per batch is the caller's to choose" in doc, name
    assert "twice" in engine.GraphStorage.labor_edges.__doc__
    assert engine.GraphStorage.LABOR_MAX_SLOTS == ref.MAX_SLOTS


def test_null_pointers_and_illegal_counts_are_refused_without_a_device():
    L = lib.load()
    assert L.legion_labor_count(None, None, None, 1, None, 1, 1, 0, None, None, 1 << 20) == -1
    assert L.legion_labor_edges(None, None, None, 1, None, 1, 1, 0, None, 1 << 20, 1, None, None, None) == -1
    for m in (-1, 0, 1, 1024, 1025, 262144, 262145, 2 ** 30, 2 ** 30 + 1):
        assert L.legion_labor_scratch_bytes(m) == ref.scratch_bytes(m), m
    assert ref.scratch_bytes(2 ** 30) == 8 * (2 ** 20 + 1 + 4096) and ref.scratch_bytes(0) == 8


def test_the_header_states_the_rule_and_what_is_not_offered():
    text = open(HEADER).read()
    for phrase in ("h * d < fanout * 2^32", "The salt is hashed first", "there is no floating point anywhere in the rule",
                   "from the pair loaded once, not from offsets", "cap is a capacity", "Memory safety does not rest on the content of scratch",
                   "LABOR-1, LABOR-*", "Hajek estimator", "prob=", "out-edges", "heterogeneous graphs", "the server, the launcher and the\n * wire"):
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
    for method in (g.labor_edges, g.labor_block):
        with pytest.raises(ValueError, match="int32"):
            method(torch.tensor([1, 2], dtype=torch.int64), 5)
        with pytest.raises(ValueError, match="one-dimensional"):
            method(np.zeros((2, 2), dtype=np.int32), 5)
        with pytest.raises(ValueError, match="at most"):
            method(np.zeros(2 ** 20 + 1, dtype=np.int32), 5)
        for fanout in (0, -1, 2 ** 31):
            with pytest.raises(ValueError, match="fanout must lie"):
                method(ok, fanout)
        for fanout in (2.0, True, None, "5"):
            with pytest.raises(ValueError, match="fanout must be an integer"):
                method(ok, fanout)
        for salt in (2 ** 63, -2 ** 63 - 1):
            with pytest.raises(ValueError, match="salt must be an int64"):
                method(ok, 5, salt=salt)
        for salt in (1.5, None, False):
            with pytest.raises(ValueError, match="salt must be an integer"):
                method(ok, 5, salt=salt)
        for flag in (1, 0, None, "yes"):
            with pytest.raises(ValueError, match="return_eids"):
                method(ok, 5, return_eids=flag)
    with pytest.raises(ValueError, match="at most 2\\^30"):
        engine.GraphStorage._check_labor_slots(2 ** 30 + 1)
    engine.GraphStorage._check_labor_slots(2 ** 30)
    engine.GraphStorage._check_labor(2 ** 31 - 1, -2 ** 63, False)
    engine.GraphStorage._check_labor(np.int64(1), np.int64(2 ** 63 - 1), True)


def test_the_predicates():
    assert ref.refused("count", -1, 5, 5) and ref.refused("count", 2 ** 20 + 1, 5, 5) and not ref.refused("count", 2 ** 20, 2 ** 30, 1)
    assert ref.refused("count", 5, -1, 5) and ref.refused("count", 5, 2 ** 30 + 1, 5) and ref.refused("count", 5, 5, 0)
    assert ref.refused("count", 5, 1025, 5, scratch=31) and not ref.refused("count", 5, 1025, 5, scratch=32)
    assert ref.refused("edges", 5, 5, 5, cap=-1) and ref.refused("edges", 5, 5, 5, cap=2 ** 31) and not ref.refused("edges", 5, 5, 5, cap=2 ** 31 - 1)
    assert not ref.refused("edges", 0, 0, 1, scratch=8, cap=0) and ref.refused("edges", 0, 0, 1, scratch=7, cap=0)


# ---- the reference against brute force ------------------------------------------------------------------------------------------
MASK = 2 ** 64 - 1


def _splitmix(x):
    x = (x + 0x9E3779B97F4A7C15) & MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK
    return x ^ (x >> 31)


def _hash(v, salt):
    return _splitmix(_splitmix(salt & MASK) ^ (v & 0xFFFFFFFF)) >> 32


def _loop(indptr, col, rows, fanout, salt, m=None):
    """The definition in Python integers: the rows' entries one after another, the first m slots looked at."""
    N = indptr.size - 1
    dst, src, eid, p = [], [], [], 0
    for i, r in enumerate(np.asarray(rows).tolist()):
        if 0 <= r < N:
            d = int(indptr[r + 1]) - int(indptr[r])
            for e in range(int(indptr[r]), int(indptr[r + 1])):
                t = int(col[e])
                if (m is None or p < m) and t >= 0 and _hash(t, salt) * d < fanout * 2 ** 32:
                    dst.append(i)
                    src.append(t)
                    eid.append(e)
                p += 1
    return np.array(dst, dtype=np.int64), np.array(src, dtype=np.int64), np.array(eid, dtype=np.int64)


def _against_the_loop(indptr, col, rows, what, fanouts=(1, 3, 25), salts=(0, -1, 2 ** 63 - 1)):
    off = in_edges_ref.row_offsets(indptr, rows)
    M = int(off[-1])
    for fanout in fanouts:
        for salt in salts:
            for m in (M, max(M - 3, 0), M // 2):
                reads = {}
                K, dst, src, eid = ref.edges(indptr, col, rows, off, m, fanout, salt, reads=reads)
                want = _loop(indptr, col, rows, fanout, salt, m)
                assert K == want[0].size == ref.count(indptr, col, rows, off, m, fanout, salt)
                for g, w in zip((dst, src, eid), want):
                    assert np.array_equal(g, w), (what, fanout, salt, m)
                assert dst.dtype == np.int32 and src.dtype == np.int32 and eid.dtype == np.int64
                walk_ref.assert_reads_in_bounds(reads, indptr.size - 1, col.size)
                capped = ref.edges(indptr, col, rows, off, m, fanout, salt, cap=K + 5)
                assert capped[0] == K and np.array_equal(capped[1][:K], dst) and np.all(capped[1][K:] == -1) and np.all(capped[3][K:] == -1)
                if K:
                    assert np.array_equal(ref.edges(indptr, col, rows, off, m, fanout, salt, cap=K - 1)[2], src[:K - 1])


def test_the_hash_and_the_predicate_are_the_definition():
    v = np.array([0, 1, 7, 12345, 2 ** 31 - 1], dtype=np.int32)
    for salt in (0, 3, -1, -2 ** 63, 2 ** 63 - 1):
        assert ref.hashes(v, salt).tolist() == [_hash(int(x), salt) for x in v.tolist()], salt
    assert ref.hashes([0], 0)[0] == 0xa706dd2f and ref.hashes([7], 3)[0] == 0xe880a903
    rng = np.random.RandomState(5)
    h = np.concatenate([rng.randint(0, 2 ** 32, 4000, dtype=np.int64), [0, 1, 2 ** 32 - 1, 2 ** 31, 2 ** 31 - 1]])
    for d in (1, 2, 5, 6, 37, 1000, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40 + 12345, 2 ** 61 + 7):
        for fanout in (1, 5, 25, 2 ** 31 - 1):
            got = ref.keeps(h, np.full(h.size, d, np.int64), fanout)
            assert got.tolist() == [ref.keep_one(x, d, fanout) for x in h.tolist()], (d, fanout)
            assert d > fanout or got.all()
    assert ref.keeps(np.array([3]), np.array([2 ** 62 + 1]), 1).tolist() == [False]


def test_the_reference_is_the_loop(world):
    indptr, col = world["indptr"], world["col"]
    for n in (1, 63, 257):
        _against_the_loop(indptr, col, node2vec_ref.seeds_for(n), f"sym {n}", fanouts=(1, 25), salts=(0, -1))
    _against_the_loop(indptr, col, gpu_main.gap_rows(), "gap", fanouts=(5,), salts=(0,))
    _against_the_loop(indptr, col, gpu_main.empty_rows(), "empty", fanouts=(5,), salts=(0,))
    for name, (ip, c) in gpu_main.small_cases().items():
        _against_the_loop(ip, c, gpu_main.small_rows(ip), name)


def test_the_block_reference_is_the_loop():
    for name, (indptr, col, seeds) in gpu_block.graphs().items():
        b = gpu_block.block_conditions(indptr, col, seeds, gpu_block.FANOUT[name])
        dst, src, eid = _loop(indptr, col, seeds, gpu_block.FANOUT[name], gpu_block.SALT)
        assert np.array_equal(b["dst"], dst) and np.array_equal(b["src"], src) and np.array_equal(b["eids"], eid), name
        seen = {int(v): i for i, v in enumerate(seeds.tolist())}
        for v in src.tolist():
            if v not in seen:
                seen[v] = len(seen)
        assert b["input_nodes"].tolist() == list(seen), name
        assert b["src_local"].tolist() == [seen[int(v)] for v in src.tolist()], name
    with pytest.raises(AssertionError):
        ref.block(indptr, col, np.array([5, 5], dtype=np.int32), 3, 0)


# ---- properties of the rule ---------------------------------------------------------------------------------------------------------
def test_a_fanout_of_the_largest_degree_keeps_exactly_the_live_entries(world):
    indptr, col = world["indptr"], world["col"]
    top = int(np.diff(indptr).max())
    for rows in (gpu_main.rows_for(257), gpu_main.rows_for("all"), gpu_main.gap_rows()):
        off = in_edges_ref.row_offsets(indptr, rows)
        full = in_edges_ref.in_edges(indptr, col, rows, off, int(off[-1]))
        live = full[1] >= 0
        for fanout in (top, top + 1, 2 ** 31 - 1):
            got = ref.edges_full(indptr, col, rows, fanout, 9)
            for g, w in zip(got, full):
                assert np.array_equal(g, w[live])
        assert ref.edges_full(indptr, col, rows, top - 1, 9)[0].size <= live.sum()


def test_the_kept_set_grows_with_the_fanout(world):
    indptr, col = world["indptr"], world["col"]
    rows = gpu_main.rows_for(257)
    off = in_edges_ref.row_offsets(indptr, rows)
    M = int(off[-1])
    for salt in (0, 1, -1):
        before = np.zeros(M, dtype=bool)
        for fanout in (1, 2, 3, 4, 5, 10, 24, 25, 26, 100, 4096, 4097):
            kept = ref.slot_mask(indptr, col, rows, off, M, fanout, salt)[0]
            assert np.all(kept[before]) and kept.sum() >= before.sum(), (salt, fanout)
            before = kept
    v = np.arange(2 ** 12)
    h = ref.hashes(v, 4)
    for d in (2, 37, 1000):
        for fanout in range(1, 40):
            assert np.all(ref.keeps(h, np.full(v.size, d), fanout + 1)[ref.keeps(h, np.full(v.size, d), fanout)])


SALTS = (0, 1, 2, 12345, 2 ** 63 - 1)


def test_the_kept_share_is_the_probability():
    """A condition, not a measurement: over v in [0, 2^16) the kept share lies within 4 binomial standard deviations of fanout / d."""
    v = np.arange(2 ** 16)
    worst = 0.0
    for salt in SALTS:
        h = ref.hashes(v, salt)
        for fanout, d in ((1, 2), (10, 37), (25, 1000), (3, 4)):
            p = fanout / d
            share = ref.keeps(h, np.full(v.size, d), fanout).mean()
            z = abs(share - p) / np.sqrt(p * (1 - p) / v.size)
            worst = max(worst, z)
            assert z <= 4.0, (salt, fanout, d, share, z)
    print(f"largest deviation: {worst:.2f} standard deviations")


def test_two_salts_are_independent():
    """The keep masks of salts 0 and 1 at probability one half agree on a share within 4 standard deviations of one half."""
    v = np.arange(2 ** 16)
    a, b = (ref.keeps(ref.hashes(v, salt), np.full(v.size, 2), 1) for salt in (0, 1))
    share = (a == b).mean()
    print(f"agreement: {share:.4f}")
    assert abs(share - 0.5) <= 4 * np.sqrt(0.25 / v.size)
    raw = [ref.keeps(ref.hashes(v, salt, raw_key=True), np.full(v.size, 2), 1) for salt in (0, 1)]
    assert np.array_equal(raw[0][0::2], raw[1][1::2]), "with the salt raw as the key, salt 1 permutes salt 0's numbers among neighbouring ids"


# ---- the figures the GPU files rely on ---------------------------------------------------------------------------------------------
def test_the_figures_of_the_main_file(world):
    indptr, col = world["indptr"], world["col"]
    for (n, fanout, salt), K in gpu_main.FIGURES.items():
        assert gpu_main.conditions(indptr, col, gpu_main.rows_for(n), fanout, salt)[3] == K, (n, fanout, salt)
    none = full = 0
    for n in gpu_main.COUNTS + ["all"]:
        for fanout in gpu_main.FANOUTS:
            kept = gpu_main.conditions(indptr, col, gpu_main.rows_for(n), fanout, 0)[2]
            t = gpu_main.tile_counts(kept)
            none, full = none + int((t == 0).sum()), full + int((t == ref.TILE).sum())
    print("tiles that keep nothing:", none, "tiles that keep everything:", full)
    assert none >= 100 and full >= 100
    assert {256, 1023, 1024, 1025} <= set(gpu_main.COUNTS) and gpu_main.MAX_DEGREE in gpu_main.FANOUTS
    rows, off, m, want = gpu_main.prefix_case(indptr, col)
    assert 0 < want[0] < m


def test_the_figures_of_the_stride_and_block_files(world):
    rows, off, kept, K, dst, src, eid = gpu_stride.slot_case(world["indptr"], world["col"])
    print("5 000 seeds: K", K)
    indptr, col, rows, K, dst, src, eid = gpu_stride.wide_case()
    print("wide: K", K)
    assert K == dst.size == src.size == eid.size and src.min() >= 1
    c = gpu_block.graphs()["sym-every-third"]
    gpu_block.two_layer_case(c[0], c[1], c[2][:300])


def test_the_fuzz_seed_set_holds_its_conditions():
    made = {}
    gpu_fuzz.seed_set_conditions(lambda seed: made.setdefault(seed, gpu_fuzz.labor_shape(seed)))
    assert len(made) == 24


# ---- the wrong kernels differ -------------------------------------------------------------------------------------------------------
def test_each_wrong_predicate_differs_on_the_main_files_inputs(world):
    indptr, col = world["indptr"], world["col"]
    differs = {name: 0 for name in ref.WRONG if name != "degree-below-m"}
    for n in (63, 257, 1025):
        rows = gpu_main.rows_for(n)
        off = in_edges_ref.row_offsets(indptr, rows)
        M = int(off[-1])
        for fanout in (1, 5, 25):
            for salt in gpu_main.SALTS:
                want = ref.slot_mask(indptr, col, rows, off, M, fanout, salt)[0]
                for name in differs:
                    differs[name] += int((ref.slot_mask(indptr, col, rows, off, M, fanout, salt, **ref.WRONG[name])[0] != want).sum())
    print(differs)
    assert differs["raw-salt"] >= 1000 and differs["hash-of-dst"] >= 1000


def test_lane_major_ranks_a_stale_trip_and_the_prefix_degree_differ(world):
    indptr, col = world["indptr"], world["col"]
    for n in (63, 257):
        for fanout in (1, 5, 25):
            out = gpu_main.conditions(indptr, col, gpu_main.rows_for(n), fanout, 0)
            assert not np.array_equal(ref.lane_major(out[6], out[2]), out[6])
            assert np.array_equal(np.sort(ref.lane_major(out[6], out[2])), np.sort(out[6])), "the same triples, another order"
    gpu_stride.slot_case(indptr, col)                                  # asserts that a stale second trip differs
    gpu_main.prefix_case(indptr, col)                                  # asserts that d as the slots below m differs
