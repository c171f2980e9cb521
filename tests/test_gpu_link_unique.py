"""engine.unique_ids / legion_unique_ids on the GPU, bit for bit against tests/link_ref.py: every tile and table-size boundary in the
count up to the limit of 2^20, the concatenation a link-prediction batch makes, all distinct, all one value, all -1, -1s scattered
through the input, and the ids i * 8192 (whose low bits are all zero: the hash has to spread them).  Every input runs twice: the table fills in whatever order the device takes the
ids, and the results are the same."""
import functools

import numpy as np
import pytest
import torch

from tests import link_ref as ref
from tests import node2vec_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
COUNTS = [1, 63, 64, 65, 256, 257, 1023, 1024, 1025, 3073, 70001, 2 ** 20]
KINDS = ["batch", "distinct", "scattered", "strided", "dead"]
STRIDED_VALUES = 2 ** 18                                           # i * 8192 for i below this fits a non-negative int32


@functools.lru_cache(maxsize=None)
def _graph():
    return node2vec_ref.sym_graph()


def ids_of(kind, m):
    i = np.arange(m, dtype=np.int64)
    if kind == "batch":                                            # [rows | cols | negatives] of B seed edges with k = 5, cut to m
        indptr, col, _ = _graph()
        B = m // 7 + 1
        out = ref.edge_prediction_seeds(indptr, col, ref.eids_for(indptr, col, B), 5, base=3)["ids"][:m]
    elif kind == "distinct":
        out = (i * 2654435761 % (2 ** 31 - 1))[np.random.RandomState(m % 1000).permutation(m)]
        assert np.unique(out).size == m
    elif kind == "scattered":                                      # a few hundred values, every third entry -1
        out = np.where(i % 3 == 1, -1 - (i % 2), i * 7919 % 389)
    elif kind == "strided":                                        # i * 8192 as int32 allows it: 2^18 distinct multiples of 8 192, in turn
        out = (i % STRIDED_VALUES) * 8192
    else:
        out = np.full(m, -1)
    return out.astype(np.int32)


def _run(ids):
    from legion_amd import engine
    unique, local, count = engine.unique_ids(torch.from_numpy(ids).to(DEV))
    torch.cuda.synchronize()
    assert count.shape == (1,) and count.dtype == torch.int32 and count.is_cuda
    return unique.cpu().numpy(), local.cpu().numpy(), int(count.item())


def _check(ids, ctx):
    want = ref.unique_ids(ids)
    first, second = _run(ids), _run(ids)
    for name, g, g2, w in zip(("unique", "local"), first, second, want):
        assert g.dtype == np.int32 and g.shape == ids.shape, ctx
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, f"{ctx}: {bad.size} entries of {name} differ, first at {bad[0]}: got {g[bad[0]]} want {w[bad[0]]}"
        assert np.array_equal(g, g2), f"{ctx}: {name} differs between two runs"
    assert first[2] == second[2] == want[2], f"{ctx}: count {first[2]}, {second[2]}, want {want[2]}"


def test_the_inputs_are_what_they_are_called(hip):
    for m in (65, 3073):
        b = ids_of("batch", m)
        u = ref.unique_ids(b)
        assert (b < 0).any() and u[2] < (b >= 0).sum(), "a batch has -1s and repeats"
        assert ref.unique_ids(ids_of("distinct", m))[2] == m and ref.unique_ids(ids_of("dead", m))[2] == 0
        s = ids_of("scattered", m)
        assert (s == -1).any() and (s == -2).any() and (s >= 0).sum() > m // 2
    for m in COUNTS:                                               # strided: ids i * 8192, every value min(m, 2^18) of them distinct
        s = ids_of("strided", m)
        assert s.min() == 0 and np.array_equal(s.astype(np.int64), (np.arange(m) % STRIDED_VALUES) * 8192)
        assert ref.unique_ids(s)[2] == min(m, STRIDED_VALUES)
        # why they are worth a case: their low 13 bits are zero, so the low bits of the id name at most slots / 8192 (one, up to m =
        # 4096) of the table's slots -- a table that took its slot from them would probe through one run as long as the input has
        # distinct ids.  The library's multiplicative hash (ref.home_slots) spreads them: more home slots than a tenth of the distinct ids
        slots = ref.table_slots(m)
        low = np.unique(s.astype(np.int64) & (slots - 1)).size
        assert low == max(min(slots // 8192, STRIDED_VALUES), 1), (m, low)
        homes = np.unique(ref.home_slots(np.unique(s), m)).size
        assert homes <= min(m, STRIDED_VALUES) and (m < 64 or homes * 10 > min(m, STRIDED_VALUES)), (m, homes)
    assert ref.table_slots(1024) == 2048 and ref.table_slots(1025) == 4096 and COUNTS[-1] == ref.MAX_IDS


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m", COUNTS)
def test_unique_ids_is_the_reference_bit_for_bit(hip, m, kind):
    _check(ids_of(kind, m), f"{kind} {m}")


def test_all_one_value(hip):
    _check(np.full(5000, 77, dtype=np.int32), "5000 times 77")
    _check(np.full(5000, 0, dtype=np.int32), "5000 times 0")
    _check(np.full(5000, 2 ** 31 - 1, dtype=np.int32), "5000 times 2^31 - 1")


def test_an_empty_call_counts_zero(hip):
    from legion_amd import engine
    unique, local, count = engine.unique_ids(np.zeros(0, np.int32))
    assert unique.shape == (0,) and local.shape == (0,) and int(count.item()) == 0 and count.is_cuda
