"""engine.EdgeIdSet and the C ABI's legion_edge_set_bytes / legion_edge_set_build / legion_edge_set_contains on the GPU, bit for bit
against tests/exclude_ref.py: k at 0, 1, 128 (exactly half of 256 slots), 129 (the table moves to 512) and 2^21; duplicates and negative
ids in the input; ids whose home slots cluster in one slot, and in the last slots so that probing wraps (the odd 64-bit multiplier
inverted); ids that differ from members only above bit 31; two sets on two objects; another stream; the refusals.  What makes a wrong
kernel fail is asserted from the numpy reference alone before any launch."""
import numpy as np
import pytest
import torch

from tests import exclude_ref as ref
from tests.compare import same_arrays

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = [0, 1, 128, 129, 2 ** 21]
EXPECTED_SLOTS = {0: 256, 1: 256, 128: 256, 129: 512, 2 ** 21: 2 ** 22}


def members_for(k):
    """k ids: distinct multiples spread over 2^40, with duplicates, negatives and ids past 2^32 once there is room (k >= 128)."""
    ids = (np.arange(k, dtype=np.int64) * 2654435761 + 12345) % (2 ** 40)
    if k >= 128:
        ids[5], ids[6], ids[7] = -1, -5, -2 ** 63
        ids[20:30] = ids[10:20]                                    # duplicates
        ids[40] = 2 ** 32 + 17
        ids[41] = 17
    return ids


def queries_for(members, m=4096):
    """m ids: members, their neighbours, negatives, and ids that differ from a member only above bit 31."""
    members = np.asarray(members, dtype=np.int64)
    live = members[members >= 0]
    rng = np.random.RandomState(members.size % 1000)
    parts = [np.array([-1, -5, 0, 1, 2 ** 62], dtype=np.int64)]
    if live.size:
        take = live[rng.randint(0, live.size, m // 4)]
        parts += [take, take + 1, take ^ (1 << 32), take ^ (1 << 40), take + (1 << 33)]
    parts.append(rng.randint(0, 2 ** 40, m, dtype=np.int64))
    return np.concatenate(parts)[:m]


def conditions(members, queries):
    """Members and non-members among the queries; from 128 ids on, queries that a key or a hash cut to 32 bits answers wrongly."""
    want = ref.contains(members, queries)
    k = len(members)
    assert ref.set_slots(k) == EXPECTED_SLOTS.get(k, ref.set_slots(k))
    if (np.asarray(members) >= 0).any():
        assert want.sum() >= 100 and (want == 0).sum() >= 100 if k >= 128 else want.sum() >= 1
    if k >= 128:
        assert (ref.contains_key32(members, queries) != want).sum() >= 50, "a key cut to 32 bits differs"
        assert (queries < 0).sum() >= 2 and want[queries < 0].sum() == 0
    return want


def clustered(k=300):
    """300 ids of a 1 024-slot table: 120 whose home is slot 77 and 120 whose homes are the last three slots, so that probing wraps
    past the end; then sixty ids past 2^32 in slot 500.  (members, longest probe run, wraps)."""
    slots = ref.set_slots(k)
    ids = np.concatenate([ref.ids_with_home(k, [77], 120), ref.ids_with_home(k, [slots - 3, slots - 2, slots - 1], 40),
                          ref.ids_with_home(k, [500], 60, high=2 ** 32)])
    assert ids.size == k and slots == 1024
    longest, wraps = ref.probe_lengths(ids, k)
    assert longest >= 120 and wraps >= 100, (longest, wraps)
    assert np.unique(ref.home_slots_hash32(ids, k)).size > 50, "a hash cut to 32 bits would not cluster them: the homes are the 64-bit hash's"
    return ids, longest, wraps


def test_bytes_and_slots(hip):
    for k in SIZES + [127, 130, 256, 257, 2 ** 20, 2 ** 20 + 1]:
        assert hip.legion_edge_set_bytes(k) == ref.set_bytes(k) == 8 * ref.set_slots(k), k
    for k in (-1, 2 ** 21 + 1, 2 ** 31 - 1):
        assert hip.legion_edge_set_bytes(k) == ref.set_bytes(k) == -1, k


@pytest.mark.parametrize("k", SIZES)
def test_contains_is_the_reference(hip, k):
    from legion_amd import engine
    members = members_for(k)
    queries = queries_for(members, 4096 if k < 2 ** 21 else ref.ITEM_STRIDE + 257)      # the large set: also past contains' capped grid
    want = conditions(members, queries)
    s = engine.EdgeIdSet(members)
    assert s.k == k and s.set_bytes == ref.set_bytes(k) and s.table.numel() == ref.set_slots(k)
    same_arrays(s.contains(queries), want, f"k {k}")
    same_arrays(s.contains(queries[:0]), want[:0], f"k {k}, no query")
    same_arrays(s.contains(queries[:1]), want[:1], f"k {k}, one query")
    if k == 2 ** 21:
        table = s.table.cpu().numpy()
        live = np.unique(members[members >= 0])
        assert np.array_equal(np.sort(table[table != -1]), live), "every distinct id sits in the table once, whole"


def test_clustered_homes_and_a_wrapping_probe(hip):
    from legion_amd import engine
    members, longest, wraps = clustered()
    print(f"clustered: longest probe run {longest}, {wraps} keys below their home")
    queries = np.concatenate([members, members + 1, members ^ (1 << 32), ref.ids_with_home(300, [77, 1023, 0, 1], 30)[::-1]])
    want = ref.contains(members, queries)
    assert want[:300].all() and (want[300:] == 0).sum() >= 300
    s = engine.EdgeIdSet(members[::-1].copy())                     # (another arrival order of the index)
    same_arrays(s.contains(queries), want, "clustered")
    table = s.table.cpu().numpy()
    assert np.array_equal(np.sort(table[table != -1]), np.sort(members)) and (table[:40] != -1).sum() >= 30, "the wrap filled the first slots"


def test_two_sets_and_another_stream(hip):
    from legion_amd import engine
    a, b = members_for(129), members_for(1000) + 3
    side = torch.cuda.Stream()
    sa = engine.EdgeIdSet(a)
    sb = engine.EdgeIdSet(b, stream=side)
    q = np.concatenate([a, b])
    got_b = sb.contains(q, stream=side)
    side.synchronize()
    same_arrays(sa.contains(q), ref.contains(a, q), "the first set")
    same_arrays(got_b, ref.contains(b, q), "the second set, on another stream")
    assert not np.array_equal(ref.contains(a, q), ref.contains(b, q))


def test_refusals(hip):
    L = hip
    s = torch.cuda.current_stream().cuda_stream
    ids = torch.arange(300, dtype=torch.int64, device=DEV)
    table = torch.full((1024,), 7, dtype=torch.int64, device=DEV)
    out = torch.full((300,), -7, dtype=torch.int32, device=DEV)
    assert L.legion_edge_set_build(s, None, 300, table.data_ptr(), 8192) == -1
    assert L.legion_edge_set_build(s, ids.data_ptr(), 300, None, 8192) == -1
    assert L.legion_edge_set_build(s, ids.data_ptr(), 300, table.data_ptr(), 8191) == -1
    assert L.legion_edge_set_build(s, ids.data_ptr(), -1, table.data_ptr(), 8192) == -1
    assert L.legion_edge_set_build(s, ids.data_ptr(), 2 ** 21 + 1, table.data_ptr(), 2 ** 40) == -1
    assert L.legion_edge_set_contains(s, None, 8192, 300, ids.data_ptr(), 300, out.data_ptr()) == -1
    assert L.legion_edge_set_contains(s, table.data_ptr(), 8192, 300, None, 300, out.data_ptr()) == -1
    assert L.legion_edge_set_contains(s, table.data_ptr(), 8192, 300, ids.data_ptr(), 300, None) == -1
    assert L.legion_edge_set_contains(s, table.data_ptr(), 8191, 300, ids.data_ptr(), 300, out.data_ptr()) == -1
    assert L.legion_edge_set_contains(s, table.data_ptr(), 8192, -1, ids.data_ptr(), 300, out.data_ptr()) == -1
    assert L.legion_edge_set_contains(s, table.data_ptr(), 8192, 300, ids.data_ptr(), -1, out.data_ptr()) == -1
    assert L.legion_edge_set_contains(s, table.data_ptr(), 8192, 300, ids.data_ptr(), 2 ** 31, out.data_ptr()) == -1
    assert L.legion_edge_set_contains(s, table.data_ptr(), 8192, 300, ids.data_ptr(), 0, out.data_ptr()) == 0
    torch.cuda.synchronize()
    assert (table == 7).all() and (out == -7).all(), "a refused call and m == 0 touch no buffer"
    # memory safety does not rest on what the set holds: a table that no build wrote, full of one key
    assert L.legion_edge_set_contains(s, table.data_ptr(), 8192, 300, ids.data_ptr(), 300, out.data_ptr()) == 0
    torch.cuda.synchronize()
    assert out.cpu().numpy().tolist() == [1 if i == 7 else 0 for i in range(300)], "S probes, then no"
    assert L.legion_edge_set_build(s, ids.data_ptr(), 0, table.data_ptr(), 8192) == 0      # k == 0 clears its 256 slots, nothing else
    torch.cuda.synchronize()
    assert (table[:256] == -1).all() and (table[256:] == 7).all()
