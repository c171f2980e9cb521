"""engine.unique_ids / legion_unique_ids on inputs that fill its table badly, bit for bit against tests/link_ref.py and run twice: ids
made by inverting the hash (link_ref.ids_with_home) so that they all start probing in the table's LAST slot -- every id but one has to
wrap to slot 0, and one of them is found only after as many probes as there are ids, under a compare-and-swap race on every slot of the
run --; 25 600 ids whose homes are the last 64 slots, spread through an ordinary input of 70 001 and of 2^20 ids; and 2^20 - 1 copies of
one id, every lane's atomicMin on one word.

Before any launch each test asserts, from the inputs alone, what makes a wrong table unable to pass: by pigeonhole (whatever the order
the device takes the ids in) how many ids wrap and how long the longest run is, confirmed by link_ref.probe_table, the insert done one
id at a time, in three arrival orders.  tests/test_link_cpu.py proves the same without a GPU, and that a table that stops at its last
slot, or one that keeps the first claimer's index instead of the minimum, gives other results on these inputs."""
import numpy as np
import pytest

from tests import link_ref as ref
from tests.test_gpu_link_unique import _check, ids_of

pytestmark = pytest.mark.gpu

ONE_HOME = [2, 200, 1000, 3000]
CLUSTERS = [70001, 2 ** 20]
CLUSTER_HOMES, CLUSTER_PER = 64, 400
HOT = 2 ** 20


def orders(n):
    """Three arrival orders: by index, by index backwards, shuffled."""
    return [np.arange(n), np.arange(n)[::-1], np.random.RandomState(n % 997).permutation(n)]


def one_home(m, interleaved):
    """m distinct ids that all start probing in the last slot of the table their input gets.  Alone: the m ids, shuffled.  Interleaved:
    every id three times -- its first appearance in descending order of the ids, its second right behind the next id's first, its
    third somewhere in a shuffled tail -- and a -1 behind every third first appearance."""
    rng = np.random.RandomState(m)
    if not interleaved:
        ids = ref.ids_with_home(m, [ref.table_slots(m) - 1], m)
        return ids[rng.permutation(m)]
    total = 3 * m + (m + 2) // 3
    desc = np.sort(ref.ids_with_home(total, [ref.table_slots(total) - 1], m))[::-1]
    out = []
    for j in range(m):
        out.append(desc[j])
        if j % 3 == 0:
            out.append(-1)
        if j >= 1:
            out.append(desc[j - 1])
    out.append(desc[m - 1])
    out = np.concatenate([np.array(out, dtype=np.int32), desc[rng.permutation(m)]])
    assert out.size == total
    return out


def one_home_conditions(ids, m):
    """All m distinct ids have the last slot as home, so -- in every arrival order -- they fill that slot and slots 0 .. m - 2: m - 1 of
    them wrap, and the one in slot m - 2 is reached by the m-th probe.  probe_table says the same in three orders."""
    total, live = ids.size, ids[ids >= 0]
    slots = ref.table_slots(total)
    assert np.unique(live).size == m and np.all(ref.home_slots(live, total) == slots - 1) and 2 * m <= slots
    first = live[np.sort(np.unique(live, return_index=True)[1])]
    if total > m:
        assert np.all(np.bincount(np.unique(live, return_inverse=True)[1]) == 3) and (ids == -1).sum() == (m + 2) // 3
        assert np.all(np.diff(first.astype(np.int64)) < 0), "first appearances in descending order of the ids"
    for order in orders(total):
        slot, longest, wraps = ref.probe_table(ids, total, order)
        assert wraps == m - 1 and longest == m, (m, total, wraps, longest)
        assert set(slot[ids >= 0].tolist()) == {slots - 1} | set(range(m - 1))


def cluster(m):
    """A `distinct` input of m ids in which CLUSTER_HOMES x CLUSTER_PER entries, the first and the last index among them, are ids whose
    homes are the table's last CLUSTER_HOMES slots."""
    slots = ref.table_slots(m)
    ids = ids_of("distinct", m).copy()
    late = ref.ids_with_home(m, range(slots - CLUSTER_HOMES, slots), CLUSTER_PER)
    late = late[np.random.RandomState(m % 1000 + 1).permutation(late.size)]
    at = np.unique(np.linspace(0, m - 1, late.size).astype(np.int64))
    assert at.size == late.size and at[0] == 0 and at[-1] == m - 1
    ids[at] = late
    return ids, at


def cluster_conditions(ids, at, m):
    """More clustered ids than there are slots from their lowest home to the table's end: all but at most CLUSTER_HOMES
    of them wrap in every order (the figure returned; tests/test_link_cpu.py confirms it with probe_table)."""
    slots = ref.table_slots(m)
    homes = ref.home_slots(ids[at], m)
    assert homes.min() == slots - CLUSTER_HOMES and np.unique(homes).size == CLUSTER_HOMES
    distinct = np.unique(ids[at]).size
    assert distinct == CLUSTER_HOMES * CLUSTER_PER > slots - homes.min()
    assert np.unique(ids).size >= m - at.size, "the rest stays an ordinary distinct input"
    return distinct - CLUSTER_HOMES                                # at least this many wrap


def hot_key():
    ids = np.full(HOT, 123456789, dtype=np.int32)
    ids[-1] = 7
    return ids


@pytest.mark.parametrize("interleaved", [False, True], ids=["alone", "interleaved"])
@pytest.mark.parametrize("m", ONE_HOME)
def test_every_id_starts_in_the_last_slot(hip, m, interleaved):
    ids = one_home(m, interleaved)
    one_home_conditions(ids, m)
    _check(ids, f"{m} ids of one home, {'interleaved' if interleaved else 'alone'}")


@pytest.mark.parametrize("m", CLUSTERS)
def test_a_cluster_at_the_tables_end(hip, m):
    ids, at = cluster(m)
    cluster_conditions(ids, at, m)
    _check(ids, f"a cluster of {at.size} ids in the last {CLUSTER_HOMES} slots, m {m}")


def test_one_hot_key(hip):
    ids = hot_key()
    unique, local, count = ref.unique_ids(ids)
    assert count == 2 and np.all(local[:-1] == 0) and local[-1] == 1 and unique[:2].tolist() == [123456789, 7]
    _check(ids, "2^20 - 1 copies of one id and another at the end")
