"""engine.exclude_edges and the C ABI's legion_edge_filter_scratch_bytes / legion_edge_filter_count / legion_edge_filter_edges on the GPU,
bit for bit against tests/exclude_ref.py: m at 0, 1, either side of a tile of 1 024, one past 256 tiles (the scan's second level) and
one past the capped grid; a set that excludes nothing and one that excludes everything; whole tiles excluded between kept ones (the
write pass's skip); capacities below, at and above the kept number; an input with a -1 tail and with dead entries; edge ids past 2^32;
overlapping outputs refused.  What makes a wrong kernel fail is asserted from the numpy reference alone before any launch."""
import numpy as np
import pytest
import torch

from tests import exclude_ref as ref
from tests.compare import same_arrays

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = [0, 1, 1023, 1024, 1025, 256 * 1024 + 1]
STRIDE_M = ref.STRIDE + 1025                                       # 2 048 workgroups x 1 024 entries, + 1 025
NAMES = ("dst", "src", "eid")
POISON = 7


def edge_list(m, seed=0, tail=0):
    """(dst int32 [m] non-decreasing, src int32 [m] with dead entries, eid int64 [m] distinct, some past 2^32); the last `tail`
    entries are the -1 / -1 / -1 of a capacity call."""
    rng = np.random.RandomState(seed)
    dst = np.sort(rng.randint(0, max(m // 7, 1), m)).astype(np.int32)
    src = rng.randint(0, 10 ** 6, m).astype(np.int32)
    src[rng.rand(m) < 0.02] = -1
    eid = np.arange(m, dtype=np.int64) * 3 + np.where(np.arange(m) % 5 == 0, 2 ** 32, 0)
    if tail:
        dst[m - tail:], src[m - tail:], eid[m - tail:] = -1, -1, -1
    return dst, src, eid


def members_for(eid, kind, seed=1):
    """The ids of the set.  "some": a third of the list's ids, ids that are none of its, negatives; "none" / "all" / "tiles": nothing of
    the list, all of it, every entry of its tiles 1, 2 and 4 and of its last tile."""
    rng = np.random.RandomState(seed)
    live = eid[eid >= 0]
    if kind == "none":
        return np.array([1, 2 ** 32 + 1, -1, 2 ** 40], dtype=np.int64)
    if kind == "all":
        return live.copy()
    if kind == "tiles":
        t = np.arange(eid.size) // ref.TILE
        return eid[(t == 1) | (t == 2) | (t == 4) | (t == t.max())]
    pick = live[rng.rand(live.size) < 1 / 3]
    return np.concatenate([pick, pick[:50] + 1, [-1, -1], live[:5] ^ (1 << 32)]).astype(np.int64)


def conditions(dst, src, eid, members, kind="some"):
    """Returns the reference at cap None; asserts what the case is for."""
    want = ref.exclude_edges(dst, src, eid, members)
    m, K = dst.size, want[3]
    keep = ref.kept_mask(dst, eid, members)
    if kind == "some" and m >= 1023:
        assert 0.5 * m < K < 0.8 * m
        assert (src[keep] == -1).sum() >= 3, "dead entries are kept"
        assert (eid[~keep] >= 2 ** 32).sum() >= 10 and (eid[keep] >= 2 ** 32).sum() >= 10, "ids past 2^32 on both sides"
        assert not np.array_equal(ref.kept_mask(dst, eid, members), (dst >= 0) & (ref.contains_key32(members, eid) == 0)), "a 32-bit key differs"
        for got, w in zip(ref.exclude_unstable(dst, src, eid, members)[:3], want[:3]):
            assert not np.array_equal(got, w), "an unstable compaction differs"
    if kind == "none":
        assert K == (dst >= 0).sum()
    if kind == "all":
        assert K == 0
    if kind == "tiles":
        per = np.add.reduceat(keep.astype(np.int64), np.arange(0, m, ref.TILE))
        assert per[0] == ref.TILE and per[1] == per[2] == per[4] == per[-1] == 0 and per[3] == ref.TILE, "whole tiles kept and skipped"
    return want


def stride_case():
    dst, src, eid = edge_list(STRIDE_M, seed=5)
    members = members_for(eid, "some", seed=6)
    want = conditions(dst, src, eid, members)
    keep = ref.kept_mask(dst, eid, members)
    stale = ref.stale_second_trip(keep, ref.STRIDE)
    assert (stale != keep).sum() >= 100, "a stale second trip keeps other entries"
    return dst, src, eid, members, want


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_c(L, dst, src, eid, members, cap, stream=None):
    """Both passes through the C ABI into poisoned buffers of cap entries: (K, dst_out, src_out, eid_out)."""
    from legion_amd import engine
    s = engine.EdgeIdSet(members)
    m = dst.size
    d, c, e = dev(dst), dev(src), dev(eid)
    nbytes = L.legion_edge_filter_scratch_bytes(m)
    assert not ref.filter_refused(m, s.k, s.set_bytes, nbytes, cap) and ref.filter_refused(m, s.k, s.set_bytes, nbytes - 1, cap)
    scratch = torch.full((nbytes // 8,), POISON, dtype=torch.int64, device=DEV)
    count = torch.full((1,), POISON, dtype=torch.int64, device=DEV)
    outs = [torch.full((max(cap, 1),), POISON, dtype=t, device=DEV) for t in (torch.int32, torch.int32, torch.int64)]
    h = (stream or torch.cuda.current_stream()).cuda_stream
    anchor = torch.zeros(1, dtype=torch.int64, device=DEV)          # (an empty tensor has no address to hand over)
    p = lambda t: t.data_ptr() if t.numel() else anchor.data_ptr()
    head = (p(d), p(c), p(e), m, s.table.data_ptr(), s.set_bytes, s.k)
    assert L.legion_edge_filter_count(h, *head, count.data_ptr(), scratch.data_ptr(), nbytes) == 0
    assert L.legion_edge_filter_edges(h, *head, scratch.data_ptr(), nbytes, cap, *[o.data_ptr() for o in outs]) == 0
    torch.cuda.synchronize()
    return int(count.item()), [o[:cap] for o in outs]


@pytest.mark.parametrize("m", SIZES)
def test_sizes(hip, m):
    from legion_amd import engine
    dst, src, eid = edge_list(m, seed=m % 97)
    members = members_for(eid, "some") if m else np.array([3, 4], dtype=np.int64)
    want = conditions(dst, src, eid, members)
    got = engine.exclude_edges(dst, src, eid, engine.EdgeIdSet(members))
    same_arrays(got, want[:3], f"m {m}", NAMES)
    K, outs = run_c(hip, dst, src, eid, members, want[3] + 5)
    assert K == want[3]
    same_arrays(outs, ref.exclude_edges(dst, src, eid, members, want[3] + 5)[:3], f"m {m} through the C ABI, five past K", NAMES)


def test_past_the_grid_cap(hip):
    from legion_amd import engine
    dst, src, eid, members, want = stride_case()
    same_arrays(engine.exclude_edges(dev(dst), dev(src), dev(eid), engine.EdgeIdSet(members)), want[:3], f"m {STRIDE_M}", NAMES)


@pytest.mark.parametrize("kind", ["none", "all", "tiles"])
def test_nothing_everything_and_whole_tiles(hip, kind):
    from legion_amd import engine
    dst, src, eid = edge_list(6 * ref.TILE + 300, seed=11, tail=40)
    if kind == "tiles":
        dst[:], src[-40:] = np.maximum(dst, 0), 5                  # (no -1 tail here: the tiles are whole)
        eid[-40:] = eid[-41] + 1 + np.arange(40)
    members = members_for(eid, kind)
    want = conditions(dst, src, eid, members, kind)
    same_arrays(engine.exclude_edges(dst, src, eid, engine.EdgeIdSet(members)), want[:3], kind, NAMES)
    K, outs = run_c(hip, dst, src, eid, members, dst.size)
    assert K == want[3]
    same_arrays(outs, ref.exclude_edges(dst, src, eid, members, dst.size)[:3], kind + ", a capacity of m", NAMES)


@pytest.mark.parametrize("where", ["below", "at", "above", "zero"])
def test_capacities_and_the_tail(hip, where):
    dst, src, eid = edge_list(5000, seed=21, tail=700)
    members = members_for(eid, "some", seed=22)
    K = ref.exclude_edges(dst, src, eid, members)[3]
    assert (dst < 0).sum() == 700 and 2000 < K < 4300 - 1024
    cap = {"below": K - 1500, "at": K, "above": K + 2500, "zero": 0}[where]
    want = ref.exclude_edges(dst, src, eid, members, cap)
    if where == "above":
        assert not np.array_equal(ref.exclude_tail_unfilled(dst, src, eid, members, cap, POISON)[0], want[0]), "an unfilled tail differs"
        assert (want[0][K:] == -1).all() and (want[2][K:] == -1).all() and cap - K > 2 * ref.TILE
    got_K, outs = run_c(hip, dst, src, eid, members, cap)
    assert got_K == K, "the count does not depend on the capacity"
    same_arrays(outs, want[:3], f"cap {where} K", NAMES)


def test_the_python_op_takes_a_tail_and_tensors_on_the_device(hip):
    from legion_amd import engine
    dst, src, eid = edge_list(3000, seed=31, tail=123)
    members = members_for(eid, "some", seed=32)
    want = conditions(dst, src, eid, members, "tail")
    assert want[3] < 3000 - 123
    s = engine.EdgeIdSet(members)
    side = torch.cuda.Stream()
    got = engine.exclude_edges(dev(dst), dev(src), dev(eid), s, stream=side)
    side.synchronize()
    same_arrays(got, want[:3], "a -1 tail, device tensors, another stream", NAMES)
    same_arrays(engine.exclude_edges(dst, src, eid, s), want[:3], "again: the set is used any number of times", NAMES)


def test_refusals(hip):
    from legion_amd import engine
    L = hip
    h = torch.cuda.current_stream().cuda_stream
    m = 2000
    dst, src, eid = [dev(a) for a in edge_list(m, seed=41)]
    s = engine.EdgeIdSet(np.arange(10, dtype=np.int64))
    nbytes = L.legion_edge_filter_scratch_bytes(m)
    assert nbytes == 8 * (2 + 1 + 1) and L.legion_edge_filter_scratch_bytes(-1) == -1 and L.legion_edge_filter_scratch_bytes(2 ** 30 + 1) == -1
    assert L.legion_edge_filter_scratch_bytes(2 ** 30) == 8 * (2 ** 20 + 1 + 4096) and L.legion_edge_filter_scratch_bytes(0) == 8
    scratch = torch.full((nbytes // 8,), POISON, dtype=torch.int64, device=DEV)
    count = torch.full((1,), POISON, dtype=torch.int64, device=DEV)
    o = [torch.full((m,), POISON, dtype=t, device=DEV) for t in (torch.int32, torch.int32, torch.int64)]
    P = lambda t: t.data_ptr()
    ok = [P(dst), P(src), P(eid), m, P(s.table), s.set_bytes, s.k]
    for i in (0, 1, 2, 4):
        bad = list(ok)
        bad[i] = None
        assert L.legion_edge_filter_count(h, *bad, P(count), P(scratch), nbytes) == -1, i
        assert L.legion_edge_filter_edges(h, *bad, P(scratch), nbytes, m, P(o[0]), P(o[1]), P(o[2])) == -1, i
    assert L.legion_edge_filter_count(h, *ok, None, P(scratch), nbytes) == -1
    assert L.legion_edge_filter_count(h, *ok, P(count), None, nbytes) == -1
    assert L.legion_edge_filter_count(h, *ok, P(count), P(scratch), nbytes - 1) == -1
    for i, v in ((3, -1), (3, 2 ** 30 + 1), (5, s.set_bytes - 1), (6, -1), (6, 2 ** 21 + 1)):
        bad = list(ok)
        bad[i] = v
        assert L.legion_edge_filter_count(h, *bad, P(count), P(scratch), 2 ** 40) == -1, (i, v)
        assert L.legion_edge_filter_edges(h, *bad, P(scratch), 2 ** 40, m, P(o[0]), P(o[1]), P(o[2])) == -1, (i, v)
    assert L.legion_edge_filter_edges(h, *ok, None, nbytes, m, P(o[0]), P(o[1]), P(o[2])) == -1
    assert L.legion_edge_filter_edges(h, *ok, P(scratch), nbytes, m, None, P(o[1]), P(o[2])) == -1
    assert L.legion_edge_filter_edges(h, *ok, P(scratch), nbytes, m, P(o[0]), None, P(o[2])) == -1
    assert L.legion_edge_filter_edges(h, *ok, P(scratch), nbytes - 1, m, P(o[0]), P(o[1]), P(o[2])) == -1
    for cap in (-1, 2 ** 31):
        assert L.legion_edge_filter_edges(h, *ok, P(scratch), nbytes, cap, P(o[0]), P(o[1]), P(o[2])) == -1
    # outputs that overlap inputs: in place, one entry inside, eid_out over dst
    assert L.legion_edge_filter_edges(h, *ok, P(scratch), nbytes, m, P(dst), P(o[1]), P(o[2])) == -1
    assert L.legion_edge_filter_edges(h, *ok, P(scratch), nbytes, m, P(o[0]), P(src) + 4 * (m - 1), P(o[2])) == -1
    assert L.legion_edge_filter_edges(h, *ok, P(scratch), nbytes, m, P(o[0]), P(o[1]), P(eid)) == -1
    assert L.legion_edge_filter_edges(h, *ok, P(scratch), nbytes, 1, P(o[0]), P(o[1]), P(dst) + 4 * (m - 2)) == -1
    assert L.legion_edge_filter_edges(h, *ok, P(scratch), nbytes, 0, P(dst), P(src), P(eid)) == 0, "cap == 0: no byte of an output"
    assert L.legion_edge_filter_edges(h, *ok, P(scratch), nbytes, 0, P(dst) + 4, P(src) + 400, P(eid) + 8) == 0, "... wherever it points"
    torch.cuda.synchronize()
    assert (scratch == POISON).all() and (count == POISON).all() and all((x == POISON).all() for x in o), "a refused call touches no buffer"
    # no eid_out: legal
    assert L.legion_edge_filter_count(h, *ok, P(count), P(scratch), nbytes) == 0
    assert L.legion_edge_filter_edges(h, *ok, P(scratch), nbytes, m, P(o[0]), P(o[1]), None) == 0
    torch.cuda.synchronize()
    d, c, e = [a.cpu().numpy() for a in (dst, src, eid)]
    want = ref.exclude_edges(d, c, e, np.arange(10), m)
    assert int(count.item()) == want[3]
    same_arrays(o[:2], want[:2], "without eid_out", NAMES)
    assert (o[2] == POISON).all()
