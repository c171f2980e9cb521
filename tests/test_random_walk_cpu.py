"""Random walks without a GPU: the new entry point in the header, the ctypes table and the library, the arguments
GraphStorage.random_walk refuses before it touches a device, and the numpy restatement's (tests/walk_ref.py) own properties on the
hand-built graph the GPU tests walk."""
import os
import re
import subprocess

import numpy as np
import pytest

from legion_amd import engine, lib
from tests import walk_ref as ref
from tests import weighted_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "legion_hip.h")
LIB = os.path.join(ROOT, "legion_amd", "liblegion_hip.so")


@pytest.fixture(scope="module")
def world():
    indptr, col, w = ref.hand_graph()
    return {"indptr": indptr, "col": col, "w": w, "table": weighted_ref.cdf(indptr, w), "seeds": ref.seeds_for(600)}


# ---- the entry point ------------------------------------------------------------------------------------------------------------
def test_symbol_in_header_ctypes_table_and_library():
    text = open(HEADER).read()
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert re.search(r"\bint32_t\s+legion_random_walk\s*\(", text)
    assert "legion_random_walk" in exported
    assert lib.SIGNATURES["legion_random_walk"] == (lib.c_i32, [lib.c_p, lib.c_p, lib.c_p, lib.c_i32, lib.c_i32, lib.c_i32,
                                                                 lib.ctypes.c_float, lib.c_i64, lib.c_p, lib.c_p])


def test_graph_storage_has_the_method():
    assert callable(getattr(engine.GraphStorage, "random_walk", None))


def test_null_pointers_are_refused_before_anything_else():
    L = lib.load()
    assert L.legion_random_walk(None, None, None, 1, 1, 0, 0.0, 0, None, None) == -1


def _bare_graph():
    g = engine.GraphStorage.__new__(engine.GraphStorage)      # (no handle: the checks come before the library call)
    g.node_num, g.edge_num = 10, 20
    return g


@pytest.mark.parametrize("kw, match", [
    (dict(length=0), "length"), (dict(length=-3), "length"), (dict(length=2.0), "length"), (dict(length=True), "length"),
    (dict(base=-1), "base"), (dict(base=1.5), "base"),
    (dict(base=2 ** 31 - 1 - 3 * 4 + 1), "draw index"), (dict(length=2 ** 30), "draw index"),
    (dict(weighted=1), "weighted"), (dict(weighted=None), "weighted"), (dict(return_eids=0), "return_eids"),
    (dict(restart_prob=-0.1), "restart_prob"), (dict(restart_prob=1.5), "restart_prob"), (dict(restart_prob=float("nan")), "restart_prob"),
    (dict(restart_prob="0.5"), "restart_prob"), (dict(restart_prob=None), "restart_prob"),
])
def test_engine_refuses_before_touching_a_device(kw, match):
    args = dict(length=4)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        _bare_graph().random_walk(np.array([1, 2, 3], dtype=np.int32), **args)


def test_engine_refuses_seeds_of_a_wrong_dtype_or_shape():
    import torch
    with pytest.raises(ValueError, match="int32"):
        _bare_graph().random_walk(torch.tensor([1, 2], dtype=torch.int64), 3)
    with pytest.raises(ValueError, match="one-dimensional"):
        _bare_graph().random_walk(np.zeros((2, 2), dtype=np.int32), 3)


def test_the_largest_legal_base_is_accepted_by_the_python_check():
    engine.GraphStorage._check_walk(3, 4, False, 0.0, False, 2 ** 31 - 1 - 12)
    engine.GraphStorage._check_walk(0, 4, True, 1.0, True, 2 ** 31 - 1)
    assert not ref.refused(3, 4, 0, 0.0, 2 ** 31 - 1 - 12, False) and ref.refused(3, 4, 0, 0.0, 2 ** 31 - 12, False)


# ---- the reference's own properties ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "weighted"])
@pytest.mark.parametrize("restart", [0.0, 0.3])
def test_every_transition_is_an_edge_and_minus_one_absorbs(world, weighted, restart):
    reads = {}
    traces, eids = ref.walk(world["indptr"], world["col"], world["seeds"], 17, table=world["table"] if weighted else None,
                            restart_prob=restart, base=5, reads=reads)
    ref.check(world["indptr"], world["col"], world["seeds"], traces, eids)
    ref.assert_reads_in_bounds(reads, ref.NODE_NUM, world["col"].size)
    assert (traces[:, 5] >= 0).any() and (traces[:, 1] < 0).any()        # some walks go on, some end at once
    if weighted:
        live = eids >= 0
        assert np.all(weighted_ref.sanitise(world["w"])[eids[live]] > 0)  # an entry of weight zero is never drawn
        assert np.all(traces[world["seeds"] == ref.ZERO_ROW, 1] == -1)    # the all-zero row yields no step


def test_seeds_outside_the_graph_read_nothing(world):
    reads = {}
    seeds = np.array([-1, ref.NODE_NUM, -7, 2 ** 31 - 1], dtype=np.int32)
    traces, eids = ref.walk(world["indptr"], world["col"], seeds, 5, table=world["table"], restart_prob=0.5, reads=reads)
    assert np.array_equal(traces[:, 0], seeds) and np.all(traces[:, 1:] == -1) and np.all(eids == -1)
    assert all(i.size == 0 for chunks in reads.values() for i in chunks)


def test_restart_one_ends_every_walk_after_its_seed(world):
    traces, eids = ref.walk(world["indptr"], world["col"], world["seeds"], 9, restart_prob=1.0)
    assert np.array_equal(traces[:, 0], world["seeds"]) and np.all(traces[:, 1:] == -1) and np.all(eids == -1)


def test_restart_zero_is_the_rule_without_restart(world):
    """restart_prob = 0 takes no restart draw: the walk is the one a rule without step 2 gives -- here a restart draw that can never
    fire (the smallest positive float32 is below every r2 > 0, and r2 == 0 needs y == 1, which these indices do not reach)."""
    plain = ref.walk(world["indptr"], world["col"], world["seeds"], 12, table=world["table"], base=77)
    never = ref.walk(world["indptr"], world["col"], world["seeds"], 12, table=world["table"], base=77, restart_prob=1e-45)
    assert np.array_equal(plain[0], never[0]) and np.array_equal(plain[1], never[1])


def test_unit_weights_are_the_unweighted_walk(world):
    unit = weighted_ref.cdf(world["indptr"], np.ones(world["col"].size, np.float32))
    a = ref.walk(world["indptr"], world["col"], world["seeds"], 20, base=1000)
    b = ref.walk(world["indptr"], world["col"], world["seeds"], 20, base=1000, table=unit)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_draws_are_the_samplers(world):
    """pow(48271, k, 2^31 - 1) is the table-driven power the sampler's references use, and the uniform first step is their draw."""
    from tests.distinct_ref import draw, minstd_pow
    k = np.array([1, 2, 2047, 2048, 2 ** 22, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1], dtype=np.uint64)
    assert [ref.minstd(int(i)) for i in k] == minstd_pow(k).tolist()
    seeds = np.full(50, 9, dtype=np.int32)
    traces, eids = ref.walk(world["indptr"], world["col"], seeds, 1, base=300)
    want = world["indptr"][9] + draw(300 + np.arange(50), np.full(50, 4097))
    live = traces[:, 1] >= 0
    assert np.array_equal(eids[live, 0], want[live]) and np.all(world["col"][want[~live]] < 0)


def test_first_step_frequencies_follow_the_weights():
    """200 000 first steps from a row of D = 8 with weights [0, 1, 0, 3, 4, 0, 8, 0] / 8: each neighbour's count within five binomial
    standard deviations of n w / T, zero-weight neighbours never.  The sequence is fixed: this passes or it does not."""
    w = (np.array([0, 1, 0, 3, 4, 0, 8, 0], dtype=np.float32) / np.float32(8))
    indptr = np.array([0, 8] + [8] * 8, dtype=np.int64)                 # vertex 0 has the row; its neighbours 1 .. 8 have none
    col = np.arange(1, 9, dtype=np.int32)
    n = 200000
    traces, eids = ref.walk(indptr, col, np.zeros(n, dtype=np.int32), 1, table=weighted_ref.cdf(indptr, w))
    assert traces[:, 1].min() >= 1 and np.array_equal(eids[:, 0], traces[:, 1] - 1)
    counts = np.bincount(eids[:, 0], minlength=8)
    prob = w.astype(np.float64) / float(w.sum())
    for i in range(8):
        if w[i] == 0:
            assert counts[i] == 0, i
        else:
            sd = np.sqrt(n * prob[i] * (1 - prob[i]))
            assert abs(counts[i] - n * prob[i]) <= 5 * sd, (i, counts[i], n * prob[i], sd)
