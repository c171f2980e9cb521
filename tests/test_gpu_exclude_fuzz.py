"""Seed-edge exclusion by fuzz: 24 seeds from RandomState(63000 + seed), each a random graph (sorted rows or not, parallel edges,
self-loops, dead entries and entries outside the graph), random edge ids for reverse_edge_ids through the path the graph allows (and
through both where it allows both), a random set and a random edge list with a -1 tail through the filter at a random capacity; all bit
for bit against tests/exclude_ref.py.  Over the set of seeds every class the other files name must occur; that is asserted from numpy
alone (tests/test_exclude_cpu.py asserts it without a GPU too)."""
import numpy as np
import pytest
import torch

from tests import exclude_ref as ref
from tests import node2vec_ref
from tests.compare import same_arrays

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEEDS = list(range(24))
POISON = 7


def shape(seed):
    """Everything a seed runs, and the classes it falls in."""
    rng = np.random.RandomState(63000 + seed)
    N = int(rng.choice([1, 2, 7, 60, 400]))
    deg = rng.randint(0, int(rng.choice([3, 12, 40])), N)
    if seed % 6 == 1:
        deg[rng.randint(N)] += 1500                                # a row longer than a tile
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    E = int(indptr[-1])
    rows = np.repeat(np.arange(N), deg)
    col = rng.randint(0, N, E).astype(np.int32)
    back = rng.rand(E) < 0.5                                       # half the edges point where an edge came from: reverses exist
    if E:
        col[back] = rows[rng.randint(0, E, int(back.sum()))]
        loops = rng.rand(E) < 0.05
        col[loops] = rows[loops]
        col[rng.rand(E) < 0.03] = -1
        col[rng.rand(E) < 0.02] = N + rng.randint(0, 5)
    sort_rows = seed % 2 == 0
    if sort_rows and E:
        order = np.lexsort((col, rows))
        col = col[order]
    is_sorted = bool(node2vec_ref.rows_sorted(indptr, col))
    n = int(rng.choice([0, 1, 300, 1500, 5000])) if seed % 8 else 0
    ids = rng.randint(-2, E + 3, n).astype(np.int64)
    want_rev = ref.reverse_edge_ids(indptr, col, ids)
    # the set and the list
    m = int(rng.choice([0, 1, 1000, 1024, 3000, 9000])) if seed % 8 != 3 else 0
    tail = int(rng.randint(0, m // 3 + 1))
    dst = np.sort(rng.randint(0, max(m // 5, 1), m)).astype(np.int32)
    src = rng.randint(-1, 50, m).astype(np.int32)
    eid = rng.randint(0, 2 ** 34, m).astype(np.int64)
    if tail:
        dst[m - tail:], src[m - tail:], eid[m - tail:] = -1, -1, -1
    kind = ["some", "none", "all", "empty"][seed % 4]
    live = eid[eid >= 0]
    if kind == "some":
        members = np.concatenate([live[rng.rand(live.size) < 0.4], live[:20], [-1, -1], live[20:60] ^ (1 << 32), rng.randint(0, 2 ** 34, 50)])
    elif kind == "none":
        members = np.concatenate([rng.randint(2 ** 35, 2 ** 36, 100), [-1]])
    elif kind == "all":
        members = np.concatenate([live, live[:10]])
    else:
        members = np.zeros(0, dtype=np.int64)
    members = members.astype(np.int64)
    K = ref.exclude_edges(dst, src, eid, members)[3]
    cap = int([K, max(K - 7, 0), K + 1500, m][rng.randint(4)])
    keep = ref.kept_mask(dst, eid, members)
    first = ref.reverse_first_probed(indptr, col, ids) if is_sorted else want_rev
    classes = {"sorted" if is_sorted else "unsorted"}
    classes |= {"no ids"} if n == 0 else set()
    classes |= {"an answer"} if (want_rev >= 0).any() else set()
    classes |= {"no reverse"} if ((want_rev < 0) & (ids >= 0) & (ids < E)).any() else set()
    classes |= {"id outside"} if ((ids < 0) | (ids >= E)).any() else set()
    classes |= {"dead given differs"} if (ref.reverse_dead_given(indptr, col, ids) != want_rev).any() else set()
    classes |= {"first probed differs"} if (first != want_rev).any() else set()
    classes |= {"self-loop"} if (E and (col[np.clip(ids, 0, E - 1)] == rows[np.clip(ids, 0, E - 1)])[(ids >= 0) & (ids < E)].any()) else set()
    classes |= {"long row"} if deg.max() > 1024 else set()
    classes |= {"empty list"} if m == 0 else set()
    classes |= {"empty set"} if members.size == 0 else set()
    classes |= {"keeps all"} if m and K == (dst >= 0).sum() and K > 0 else set()
    classes |= {"keeps none"} if m and K == 0 else set()
    classes |= {"keeps some"} if 0 < K < (dst >= 0).sum() else set()
    classes |= {"tail"} if tail else set()
    classes |= {"dead kept"} if (src[keep] == -1).any() else set()
    classes |= {"cap below"} if cap < K else {"cap above"} if cap > K else {"cap at"}
    classes |= {"key32 differs"} if (ref.contains_key32(members, eid) != ref.contains(members, eid)).any() else set()
    classes |= {"duplicates"} if np.unique(members).size < members.size else set()
    return dict(indptr=indptr, col=col, sorted=is_sorted, ids=ids, want_rev=want_rev, dst=dst, src=src, eid=eid, members=members, cap=cap,
                K=K, classes=classes)


WANTED = {"sorted", "unsorted", "no ids", "an answer", "no reverse", "id outside", "dead given differs", "first probed differs", "self-loop",
          "long row", "empty list", "empty set", "keeps all", "keeps none", "keeps some", "tail", "dead kept", "cap below", "cap above", "cap at",
          "key32 differs", "duplicates"}


def seed_set_conditions(make=shape):
    seen = {}
    for seed in SEEDS:
        for c in make(seed)["classes"]:
            seen.setdefault(c, []).append(seed)
    assert WANTED <= set(seen), sorted(WANTED - set(seen))
    for c in ("sorted", "unsorted", "an answer", "no reverse", "keeps some"):
        assert len(seen[c]) >= 3, (c, seen[c])
    return seen


@pytest.fixture(scope="module")
def shapes(hip):
    made = {}
    seed_set_conditions(lambda seed: made.setdefault(seed, shape(seed)))
    return made


@pytest.mark.parametrize("seed", SEEDS)
def test_fuzz(hip, shapes, seed):
    from legion_amd import engine
    c = shapes[seed]
    d_col = torch.from_numpy(c["col"]).to(DEV) if c["col"].size else torch.zeros(0, dtype=torch.int32, device=DEV)
    graph = engine.GraphStorage(1, torch.from_numpy(c["indptr"]).to(DEV), d_col)
    try:
        ids, want = c["ids"], c["want_rev"]
        same_arrays(graph.reverse_edge_ids(ids), want, f"seed {seed}: reverse_edge_ids")
        if ids.size:
            assert graph.rows_sorted() == c["sorted"]
            graph.reverse()
            d_ids = torch.from_numpy(ids).to(DEV)
            h = torch.cuda.current_stream().cuda_stream
            for via in (0, 1):
                out = torch.full((ids.size,), -POISON, dtype=torch.int64, device=DEV)
                rc = hip.legion_reverse_edge_ids(h, graph.handle, d_ids.data_ptr(), ids.size, via, out.data_ptr())
                assert rc == (0 if via == 1 or c["sorted"] else -1), (seed, via)
                same_arrays(out, want if rc == 0 else np.full(ids.size, -POISON, dtype=np.int64), f"seed {seed}: via {via}")
        s = engine.EdgeIdSet(c["members"])
        q = np.concatenate([c["eid"], c["members"], c["members"] + 1, [-1, 0]]).astype(np.int64)
        same_arrays(s.contains(q), ref.contains(c["members"], q), f"seed {seed}: contains")
        got = engine.exclude_edges(c["dst"], c["src"], c["eid"], s)
        same_arrays(got, ref.exclude_edges(c["dst"], c["src"], c["eid"], c["members"])[:3], f"seed {seed}: exclude_edges", ("dst", "src", "eid"))
        if c["dst"].size:                                          # the C ABI at the seed's capacity, into poisoned buffers
            m, cap = c["dst"].size, c["cap"]
            dev = [torch.from_numpy(c[k]).to(DEV) for k in ("dst", "src", "eid")]
            nbytes = hip.legion_edge_filter_scratch_bytes(m)
            scratch = torch.full((nbytes // 8,), POISON, dtype=torch.int64, device=DEV)
            count = torch.full((1,), POISON, dtype=torch.int64, device=DEV)
            outs = [torch.full((max(cap, 1),), POISON, dtype=t, device=DEV) for t in (torch.int32, torch.int32, torch.int64)]
            h = torch.cuda.current_stream().cuda_stream
            head = [x.data_ptr() for x in dev] + [m, s.table.data_ptr(), s.set_bytes, s.k]
            assert hip.legion_edge_filter_count(h, *head, count.data_ptr(), scratch.data_ptr(), nbytes) == 0
            assert hip.legion_edge_filter_edges(h, *head, scratch.data_ptr(), nbytes, cap, *[o.data_ptr() for o in outs]) == 0
            torch.cuda.synchronize()
            assert int(count.item()) == c["K"]
            want = ref.exclude_edges(c["dst"], c["src"], c["eid"], c["members"], cap)[:3]
            same_arrays([o[:cap] for o in outs], want, f"seed {seed}: cap {cap}, K {c['K']}", ("dst", "src", "eid"))
            assert all((o[cap:] == POISON).all() for o in outs), "nothing past the capacity"
    finally:
        torch.cuda.synchronize()
        graph.close()
