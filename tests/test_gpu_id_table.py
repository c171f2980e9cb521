"""One table, two users: a NodeSet built from a list of ids and unique_ids over the same list agree, bit for bit with numpy.  For ids of
m entries: NodeSet(ids).lookup(ids)[i] is the first index of ids[i] in ids (-1 for a negative id); unique[local[i]] is ids[i];
unique[:count] is ids at the sorted first positions of its distinct values; NodeSet.distinct is count.  m = 1, 128, 129 (the table
doubles), 255, 256, 257 (unique_ids' tile is 256) and 1 025; the contents: all equal, all distinct, negatives interleaved, and ids whose
home slot is the table's last or the one before it -- computed with Python integers from the hash, several to a home -- so that the probe
chains wrap."""
import numpy as np
import pytest
import torch

from tests.compare import same_arrays

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = [1, 128, 129, 255, 256, 257, 1025]
KINDS = ["equal", "distinct", "negatives", "last-homes"]
HASH = 2654435769
HASH_INV = pow(HASH, -1, 2 ** 32)


def slots_of(m):
    s = 256
    while s < 2 * m:
        s *= 2
    return s


def home(v, m):
    return ((v * HASH) % 2 ** 32) >> (32 - (slots_of(m).bit_length() - 1))


def ids_at_home(h, m, count):
    """count non-negative int32 ids whose home slot in the table of m ids is h: the hash inverted over the values that shift down to h."""
    shift = 32 - (slots_of(m).bit_length() - 1)
    out, y = [], h << shift
    while len(out) < count:
        assert y < (h + 1) << shift, (h, m, count)
        v = (y * HASH_INV) % 2 ** 32
        if v < 2 ** 31:
            out.append(v)
        y += 1
    return out


def ids_of(kind, m):
    rng = np.random.RandomState(1000 + m)
    if kind == "equal":
        return np.full(m, 77, np.int32)
    if kind == "distinct":
        return rng.choice(10 ** 6, m, replace=False).astype(np.int32)
    if kind == "negatives":
        ids = rng.randint(0, max(m // 3, 2), m).astype(np.int32)              # repeats among the rest
        ids[::3] = -1 - rng.randint(0, 5, ids[::3].size).astype(np.int32)
        return ids
    S = slots_of(m)
    pool = ids_at_home(S - 1, m, m - m // 2) + ids_at_home(S - 2, m, m // 2)
    ids = np.array(pool, dtype=np.int64)[rng.permutation(m)]
    ids[m // 2:] = ids[:m - m // 2][::-1]                                     # every id of the first half again
    return ids.astype(np.int32)


def reference(ids):
    """(pos int32 [m], the sorted first positions of the distinct non-negative values)."""
    first = {}
    for i, v in enumerate(ids.tolist()):
        if v >= 0:
            first.setdefault(v, i)
    pos = np.array([first.get(v, -1) for v in ids.tolist()], dtype=np.int32)
    return pos, np.array(sorted(first.values()), dtype=np.int64)


def test_the_inputs_are_what_they_are_called():
    assert [slots_of(m) for m in SIZES] == [256, 256, 512, 512, 512, 1024, 4096]
    for m in SIZES:
        assert np.unique(ids_of("distinct", m)).size == m and np.unique(ids_of("equal", m)).size == 1
        neg = ids_of("negatives", m)
        assert (neg[::3] < 0).all() and (m < 6 or np.unique(neg[neg >= 0]).size < (neg >= 0).sum()), "negatives between ids that repeat"
        last = ids_of("last-homes", m)
        S = slots_of(m)
        homes = [home(int(v), m) for v in last.tolist()]
        assert (last >= 0).all() and set(homes) <= {S - 1, S - 2}
        if m > 1:
            per_home = [np.unique(last[np.array(homes) == h]).size for h in (S - 1, S - 2)]
            assert min(per_home) >= 20 and np.unique(last).size < m, "several ids to a home, so the chains run past the table's end, and repeats"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m", SIZES)
def test_a_node_set_and_unique_ids_agree_with_numpy(hip, m, kind):
    from legion_amd import engine
    ids = ids_of(kind, m)
    assert ids.shape == (m,) and ids.dtype == np.int32
    pos, firsts = reference(ids)
    d_ids = torch.from_numpy(ids).to(DEV)
    ns = engine.NodeSet(d_ids)
    local_pos = ns.lookup(d_ids)
    unique, local, count = engine.unique_ids(d_ids)
    torch.cuda.synchronize()
    what = f"{kind}, m {m}"
    same_arrays(local_pos, pos, what + ": NodeSet.lookup")
    U = int(count.item())
    assert U == firsts.size == int(ns.distinct.item()), f"{what}: count {U}, distinct {int(ns.distinct.item())}, want {firsts.size}"
    unique, local = unique.cpu().numpy(), local.cpu().numpy()
    same_arrays(unique[:U], ids[firsts], what + ": unique[:count]")
    assert np.all(unique[U:] == -1) and np.array_equal(local < 0, ids < 0), what
    live = ids >= 0
    same_arrays(unique[local[live]], ids[live], what + ": unique[local]")
    same_arrays(firsts[local[live]].astype(np.int32), pos[live], what + ": the two users name the same first index")
