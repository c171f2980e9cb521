"""engine.NodeSet and the C ABI's legion_node_set_build / legion_node_set_lookup on the GPU, alone, bit for bit against tests/induced_ref.py
(pos by a dict) over sentinel-filled buffers: k = 0, 1, 127, 128, 129 (the table doubles between 128 and 129) and 2^20; ids clustered on
the last two home slots of the table (the probe wraps), on one home slot (a run of a hundred slots) and spread; repeats, negatives and
ids at 2^31 - 1; lookups of members, non-members, -1 and ids whose home slot another key occupies; distinct_out; a set memory that
_build did not write; another stream; a captured graph replayed twice; every refusal.  What makes a wrong kernel fail is asserted from
the numpy reference alone before any launch; an input that fails a condition is replaced, never the condition."""
import ctypes

import numpy as np
import pytest
import torch

from tests import induced_ref as ref
from tests import link_ref
from tests.compare import same_arrays

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 0x5A5A5A5A
TOP = 2 ** 31 - 1


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream_of(stream=None):
    return ctypes.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)


# ---- the inputs: name -> (nodes, ids to look up) --------------------------------------------------------------------------------------
def cluster(k, homes, per):
    """(members, others): per ids of each home slot in the set, per more of the same homes outside it."""
    ids = link_ref.ids_with_home(k, homes, 2 * per).reshape(len(homes), 2 * per)
    return ids[:, :per].reshape(-1), ids[:, per:].reshape(-1)


def sets():
    out = {}
    rng = np.random.RandomState(41)
    spread = rng.choice(10 ** 6, 100, replace=False).astype(np.int32)
    asked = np.concatenate([spread[::-1], rng.randint(0, 10 ** 6, 300), [-1, -7, TOP, 0]]).astype(np.int32)
    out["spread"] = (spread, asked)
    # the last two home slots of the 256-slot table: 80 keys whose probes run past slot 255
    inside, outside = cluster(100, [254, 255], 40)
    nodes = np.concatenate([inside, spread[:20]]).astype(np.int32)
    out["wrap"] = (nodes, np.concatenate([nodes, outside, [-1]]).astype(np.int32))
    out["wrap-reversed"] = (nodes[::-1].copy(), out["wrap"][1])
    inside, outside = cluster(100, [17], 100)
    out["one-home"] = (inside, np.concatenate([inside[::-1], outside, [-1, 17]]).astype(np.int32))
    rep = np.concatenate([spread[:50], [-1, TOP], spread[:30][::-1], [-5, TOP, 0, 0], spread[40:60]]).astype(np.int32)
    out["repeats"] = (rep, np.concatenate([rep, [TOP - 1, 1, -1]]).astype(np.int32))
    out["k-0"] = (np.zeros(0, np.int32), np.array([0, -1, 5, TOP], np.int32))
    out["k-1"] = (np.array([5], np.int32), np.array([0, -1, 5, TOP, 5], np.int32))
    for k in (127, 128, 129):
        nodes = rng.choice(10 ** 6, k, replace=False).astype(np.int32)
        out[f"k-{k}"] = (nodes, np.concatenate([nodes, nodes[:20] + 1, [-1]]).astype(np.int32))
    return out


def big_set():
    """2^20 nodes, a few thousand repeated, and 2^16 + 3 lookups: more than one grid trip of the insert (2 048 x 256 lanes)."""
    rng = np.random.RandomState(43)
    nodes = rng.randint(0, TOP, 2 ** 20).astype(np.int32)
    nodes[10000:14000] = nodes[:4000]
    nodes[7] = -1
    asked = np.concatenate([nodes[::16], [-1, TOP, 0]]).astype(np.int32)
    asked[1::2] ^= 1                                               # half of them: a neighbour id, mostly no member
    return nodes, asked


def conditions(name, nodes, asked):
    want = ref.pos(nodes, asked)
    k = nodes.size
    assert ref.set_bytes(k) == 8 * link_ref.table_slots(k)
    if k:
        assert (want >= 0).sum() >= 1 and (want < 0).sum() >= 1, "members and non-members"
    if name.startswith("wrap"):
        for order in (np.arange(k), np.arange(k)[::-1]):
            slot, longest, wraps = link_ref.probe_table(nodes, k, order)
            assert wraps >= 40 and longest >= 40, (longest, wraps)
        lost = ref.lost_without_wrap(nodes)
        assert len(lost) >= 40 and not np.array_equal(ref.pos(nodes, asked, lost=lost), want), "a table that does not wrap loses members"
    if name == "one-home":
        assert link_ref.probe_table(nodes, k, np.arange(k))[1] == 100, "a run of a hundred slots"
    if name == "repeats":
        assert not np.array_equal(ref.pos(nodes, asked, last=True), want), "the last position differs"
        assert ref.distinct(nodes) < (nodes >= 0).sum() < k
    return want


def test_the_inputs_hold_their_conditions_before_any_launch():
    for name, (nodes, asked) in sets().items():
        conditions(name, nodes, asked)
    assert [link_ref.table_slots(k) for k in (0, 1, 127, 128, 129, 2 ** 20)] == [256, 256, 256, 256, 512, 2 ** 21]
    nodes, asked = big_set()
    assert ref.distinct(nodes) < 2 ** 20 - 4000 + 10 and nodes.size > 2048 * 256


# ---- the C ABI over sentinel-filled buffers -------------------------------------------------------------------------------------------
def build(L, nodes, stream=None, fill=None, offset=0):
    """legion_node_set_build into a sentinel-filled buffer with 8 spare words: (table, set_bytes, k, nodes on the device, distinct).
    fill: a value to fill the set memory with INSTEAD of building (distinct is then None).  offset: the words the set starts behind a
    16-byte boundary (not 0: the kernels probe key by key instead of four keys a load)."""
    k = nodes.size
    nbytes = int(L.legion_node_set_bytes(k))
    assert nbytes == ref.set_bytes(k) and nbytes % 8 == 0
    table = torch.full((nbytes // 4 + 8 + offset,), SENTINEL if fill is None else fill, dtype=torch.int32, device=DEV)[offset:]
    assert table.data_ptr() % 16 == 4 * offset
    d_nodes = torch.from_numpy(np.ascontiguousarray(nodes)).to(DEV) if k else torch.zeros(1, dtype=torch.int32, device=DEV)
    if fill is not None:
        return table, nbytes, k, d_nodes, None
    distinct = torch.full((1 + 8,), SENTINEL, dtype=torch.int32, device=DEV)
    assert L.legion_node_set_build(stream_of(stream), P(d_nodes), k, P(table), nbytes, P(distinct)) == 0
    return table, nbytes, k, d_nodes, distinct


def lookup(L, table, nbytes, k, asked, stream=None):
    m = asked.size
    d_ids = torch.from_numpy(np.ascontiguousarray(asked)).to(DEV)
    local = torch.full((m + 8,), SENTINEL, dtype=torch.int32, device=DEV)
    assert L.legion_node_set_lookup(stream_of(stream), P(table), nbytes, k, P(d_ids), m, P(local)) == 0
    return local


def check(L, nodes, asked, what, stream=None, offset=0):
    table, nbytes, k, _, distinct = build(L, nodes, stream, offset=offset)
    local = lookup(L, table, nbytes, k, asked, stream)
    torch.cuda.synchronize()
    assert bool((table[nbytes // 4:] == SENTINEL).all()) and bool((distinct[1:] == SENTINEL).all()) and bool((local[asked.size:] == SENTINEL).all()), \
        what + ": written past the set, the count or the output"
    assert int(distinct[0].item()) == ref.distinct(nodes), what + f": distinct {int(distinct[0].item())} want {ref.distinct(nodes)}"
    same_arrays(local[:asked.size], ref.pos(nodes, asked), what)
    S = nbytes // 8
    keys = table[:S].cpu().numpy()
    assert sorted(keys[keys != -1].tolist()) == sorted(ref.positions(nodes)), what + ": the keys are the distinct non-negative nodes"


@pytest.mark.parametrize("name", sorted(sets()))
def test_build_and_lookup_are_the_reference(hip, name):
    nodes, asked = sets()[name]
    conditions(name, nodes, asked)
    check(hip, nodes, asked, name)


@pytest.mark.parametrize("offset", [1, 2, 3])
@pytest.mark.parametrize("name", ["wrap", "one-home", "repeats", "k-129"])
def test_a_set_that_starts_behind_a_16_byte_boundary(hip, name, offset):
    nodes, asked = sets()[name]
    check(hip, nodes, asked, f"{name} at {4 * offset} bytes", offset=offset)


def test_a_set_of_2_to_the_20(hip):
    nodes, asked = big_set()
    check(hip, nodes, asked, "2^20 nodes")


def test_the_python_class(hip):
    from legion_amd import engine
    nodes, asked = sets()["repeats"]
    for given in (nodes, torch.from_numpy(nodes).to(DEV)):                # from the host and from the device
        ns = engine.NodeSet(given)
        assert ns.k == nodes.size and ns.nodes.is_cuda and ns.distinct.shape == (1,) and ns.distinct.dtype == torch.int32
        got = ns.lookup(asked)
        again = ns.lookup(torch.from_numpy(asked).to(DEV))
        torch.cuda.synchronize()
        assert int(ns.distinct.item()) == ref.distinct(nodes)
        same_arrays(got, ref.pos(nodes, asked), "NodeSet.lookup")
        same_arrays(again, ref.pos(nodes, asked), "NodeSet.lookup, ids on the device")
    empty = engine.NodeSet(np.zeros(0, np.int32))
    assert empty.k == 0 and empty.lookup(np.zeros(0, np.int32)).shape == (0,)
    got = empty.lookup(asked)
    torch.cuda.synchronize()
    assert int(empty.distinct.item()) == 0 and bool((got == -1).all())


@pytest.mark.parametrize("fill", [-1, 0, SENTINEL], ids=["all-ones", "all-zero", "sentinel"])
def test_a_set_memory_that_build_did_not_write(hip, fill):
    """Only local_out[0 .. m) is written and nothing outside the table is read, whatever the set memory holds: the values are
    unspecified but lie in {-1} u [0, k).  All-ones is the empty table; in the all-zero one vertex 0 sits in every slot with position
    0, and every other id probes all 256 slots; in the sentinel one the id SENTINEL finds its key and a position past k."""
    nodes, asked = sets()["spread"]
    asked = np.concatenate([asked, [SENTINEL, 0, 1, -1]]).astype(np.int32)
    for offset in (0, 1):                                                 # four keys a load, and key by key
        table, nbytes, k, _, _ = build(hip, nodes, fill=fill, offset=offset)
        local = lookup(hip, table, nbytes, k, asked)
        torch.cuda.synchronize()
        got = local.cpu().numpy()
        assert np.all(got[asked.size:] == SENTINEL) and bool((table == fill).all())
        got = got[:asked.size]
        assert np.all((got == -1) | ((got >= 0) & (got < k)))
        if fill == 0:
            assert np.array_equal(got, np.where(asked == 0, 0, -1))
        else:
            assert np.all(got == -1)


def test_another_stream_and_a_captured_graph(hip):
    L = hip
    nodes, asked = sets()["wrap"]
    want = ref.pos(nodes, asked)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    assert s != torch.cuda.current_stream()
    check(L, nodes, asked, "another stream", stream=s)

    k, m = nodes.size, asked.size
    nbytes = int(L.legion_node_set_bytes(k))
    d_nodes, d_ids = torch.from_numpy(nodes).to(DEV), torch.from_numpy(asked).to(DEV)
    table = torch.zeros(nbytes // 4, dtype=torch.int32, device=DEV)
    distinct = torch.zeros(1, dtype=torch.int32, device=DEV)
    local = torch.zeros(m, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cs = stream_of()
        rc = [L.legion_node_set_build(cs, P(d_nodes), k, P(table), nbytes, P(distinct)),
              L.legion_node_set_lookup(cs, P(table), nbytes, k, P(d_ids), m, P(local))]
    assert rc == [0, 0]
    for _ in range(2):
        for x in (table, distinct, local):
            x.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        assert int(distinct.item()) == ref.distinct(nodes)
        same_arrays(local, want, "captured")


def test_c_abi_refusals_leave_the_buffers_untouched(hip):
    L = hip
    k, m = 100, 16
    nodes = torch.full((k,), SENTINEL, dtype=torch.int32, device=DEV)
    table = torch.full((2048 // 4,), SENTINEL, dtype=torch.int32, device=DEV)
    distinct = torch.full((2,), SENTINEL, dtype=torch.int32, device=DEV)
    ids = torch.full((m,), SENTINEL, dtype=torch.int32, device=DEV)
    local = torch.full((m,), SENTINEL, dtype=torch.int32, device=DEV)
    s = stream_of()
    for bad_k in (-1, 2 ** 20 + 1, 2 ** 31 - 1):
        assert L.legion_node_set_bytes(bad_k) == -1 == ref.set_bytes(bad_k)
    assert L.legion_node_set_bytes(k) == 2048 == ref.set_bytes(k)
    ok = dict(nodes=P(nodes), k=k, set=P(table), bytes=2048, distinct=P(distinct))
    for change in (dict(nodes=None), dict(set=None), dict(distinct=None), dict(k=-1), dict(k=2 ** 20 + 1, bytes=1 << 40), dict(bytes=2047),
                   dict(bytes=0), dict(bytes=-1), dict(k=129)):
        a = dict(ok, **change)
        assert None in (a["nodes"], a["set"], a["distinct"]) or ref.refused("build", k=a["k"], set_b=a["bytes"]), change
        assert L.legion_node_set_build(s, a["nodes"], a["k"], a["set"], a["bytes"], a["distinct"]) == -1, change
    ok = dict(set=P(table), bytes=2048, k=k, ids=P(ids), m=m, local=P(local))
    for change in (dict(set=None), dict(ids=None), dict(local=None), dict(k=-1), dict(k=2 ** 20 + 1, bytes=1 << 40), dict(bytes=2047),
                   dict(bytes=-1), dict(k=129), dict(m=-1), dict(m=2 ** 31), dict(m=2 ** 40)):
        a = dict(ok, **change)
        assert None in (a["set"], a["ids"], a["local"]) or ref.refused("lookup", k=a["k"], set_b=a["bytes"], m=a["m"]), change
        assert L.legion_node_set_lookup(s, a["set"], a["bytes"], a["k"], a["ids"], a["m"], a["local"]) == -1, change
    assert L.legion_node_set_lookup(s, P(table), 2048, k, P(ids), 0, P(local)) == 0           # m == 0: nothing runs
    torch.cuda.synchronize()
    for x in (nodes, table, distinct, ids, local):
        assert bool((x == SENTINEL).all()), "a refused call wrote"
    assert L.legion_node_set_build(s, P(nodes), 0, P(table), 2048, P(distinct)) == 0             # k == 0: clears, writes 0, nothing else
    torch.cuda.synchronize()
    assert bool((table == -1).all()) and distinct[0].item() == 0 and distinct[1].item() == SENTINEL
