"""Every gather_kernel instance alone, bit for bit against tests/gather_ref.py, through legion_gather_rows_fmt.

gather_plan.h picks one of about two dozen instances (six row formats x the tile sizes ROWS of each x LASTOP).  Whole-batch tests
reach the bf16 formats at ROWS = 16 and one tile per workgroup only, and the float32 single-kernel tests a few (format, ROWS) pairs.
Here each case says which instance it means to run and checks with plan_out that this is the one that ran:
  a. every (format, ROWS), one tile per workgroup, over the D at which a row's chunking changes;
  b. the tile walk (more tiles than workgroups: the software-pipelined loop with its t+1 / t+2 prefetches and the LDS buffer flip),
     more than two tiles per workgroup and a partial last tile, for every (format, ROWS);
  c. the clamps and the refusals.
The whole dst buffer and the whole cache_index are compared: rows before / after the range, skipped rows and -- with bf16 output
rows of odd D -- the neighbours of every stored element must keep their sentinel.  bf16 source tables hold a NaN in their pad
elements, so a stored pad element shows."""
import contextlib
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import gather_ref as ref
from tests.gather_ref import BF16, F32

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PAIRS = [(F32, F32), (BF16, F32), (BF16, BF16), (F32, BF16)]          # (dtype, out_dtype)
PAIR_IDS = ["f32-f32", "bf16-f32", "bf16-bf16", "f32-bf16"]
TILES = [16, 32, 64, 128, 256]
# D < 4, D < 8, the D % 4 and D % 8 tails, odd D, exactly 256 chunks a row and more than 256 (dr = 0)
DS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 24, 100, 104, 128, 256, 602, 1024, 1026, 2049, 2056, 4099]
SENTINEL = {F32: 0xFFC0DEAD, BF16: 0xBEEF}
IDX_SENTINEL = 99
OFF = 123
TARGET_WG = 8192                 # LG_GATHER_TARGET_WG: the workgroups of a full launch


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    """bit patterns -> device tensor of the signed type of the same width"""
    signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint16): np.int16, np.dtype(np.int32): np.int32}[a.dtype]
    return torch.from_numpy(np.ascontiguousarray(a).view(signed)).cuda()


@contextlib.contextmanager
def gather_rows_env(hip, monkeypatch, rows):
    """LEGION_GATHER_ROWS = rows (0: unset) for the launches inside."""
    if rows:
        monkeypatch.setenv("LEGION_GATHER_ROWS", str(rows))
    else:
        monkeypatch.delenv("LEGION_GATHER_ROWS", raising=False)
    hip.legion_tuning_from_env()
    try:
        yield
    finally:
        monkeypatch.delenv("LEGION_GATHER_ROWS", raising=False)
        hip.legion_tuning_from_env()


class Case:
    """One set of inputs, built once and never changed: a float32 table of N rows (bit patterns; the first rows awkward values), two
    cache tables of `cap` rows addressed through one node_map, ids (hits, misses, ids < 0) and carried slots, and their stored
    forms per dtype on the host and on the device."""

    def __init__(self, D, N, cap, total, seed):
        rng = np.random.RandomState(seed)
        self.D, self.N, self.cap, self.total, self.Kg = D, N, cap, total, 2
        rand = lambda n: rng.randint(0, 2 ** 32, size=(n, D), dtype=np.uint64).astype(np.uint32)
        n_awk = ref.AWKWARD.size
        bits = rand(N)
        bits[:n_awk] = ref.awkward_rows(n_awk, D)
        cbits = [rand(cap), rand(cap)]
        cbits[1][:n_awk] = ref.awkward_rows(n_awk, D)[::-1]
        self.bits = {F32: (bits, cbits)}
        slots = self.Kg * cap
        self.node_map = np.full(N, ref.MISS, dtype=np.int32)
        cached = rng.permutation(N)[:slots]
        self.node_map[cached] = (np.arange(slots) % self.Kg) * cap + np.arange(slots) // self.Kg     # slot (t % Kg) * cap + t // Kg
        ids = rng.randint(0, N, size=total).astype(np.int32)
        ids[OFF + 3:OFF + 3 + n_awk] = np.arange(n_awk)                          # the table's awkward rows (hits or misses)
        ids[OFF + 40:OFF + 40 + n_awk] = cached[1:2 * n_awk:2]                   # the awkward rows of cache table 1
        ids[::97] = -1                                                           # skipped rows
        self.ids = ids
        # carried slots: what node_map says, UNKNOWN on a third of the rows, and on some rows another slot or a miss
        g = np.where(ids >= 0, self.node_map[np.maximum(ids, 0)], ref.MISS).astype(np.int32)
        g[rng.permutation(total)[:total // 3]] = ref.UNKNOWN
        other = rng.permutation(total)[:total // 10]
        g[other] = rng.randint(0, slots, size=other.size)
        g[rng.permutation(total)[:total // 50]] = ref.MISS
        self.slots = g
        self.differ = int(np.sum((g >= 0) & (g != np.where(ids >= 0, self.node_map[np.maximum(ids, 0)], ref.MISS))))
        self.d = {"map": _dev(self.node_map), "ids": _dev(ids), "slots": _dev(g)}

    def host(self, dtype):
        if dtype not in self.bits:
            t, c = self.bits[F32]
            self.bits[dtype] = (ref.stored(t, dtype), [ref.stored(x, dtype) for x in c])
        return self.bits[dtype]

    def device(self, dtype):
        if ("table", dtype) not in self.d:
            t, c = self.host(dtype)
            self.d["table", dtype] = _dev(t)
            self.d["caches", dtype] = [_dev(x) for x in c]
            self.d["ptrs", dtype] = torch.tensor([x.data_ptr() for x in self.d["caches", dtype]], dtype=torch.int64).cuda()
        return self.d["table", dtype], self.d["ptrs", dtype]


@pytest.fixture(scope="module")
def cases():
    """The inputs of this file, shared by its tests and dropped with the module."""
    made = {}

    def get(D, N=2000, cap=500, total=3000):
        key = (D, N, cap, total)
        if key not in made:
            made[key] = Case(D, N, cap, total, seed=1000 * D + total % 997)
        return made[key]
    yield get
    made.clear()
    torch.cuda.empty_cache()


def differences(got, want, what):
    if got.shape == want.shape and np.array_equal(got, want):
        return None
    bad = np.argwhere(got != want)
    at = tuple(int(x) for x in bad[0])
    return f"{what}: {len(bad)} elements differ, the first at {at}: got {int(got[at]):#x}, expected {int(want[at]):#x}"


def run(hip, case, dtype, out_dtype, cnt, *, max_rows=None, dst_rows=None, grid_rows=0, last_op=1, carried=False, use_map=True,
        ids=None, what=""):
    """One launch over rows OFF .. OFF + cnt - 1 of a buffer of case.total rows; the whole buffer and cache_index against the
    reference.  Returns plan_out."""
    D, total = case.D, case.total
    assert OFF + cnt <= total
    max_rows = cnt if max_rows is None else max_rows
    dst_rows = total if dst_rows is None else dst_rows
    assert dst_rows <= total                                    # the kernel's clamp is never looser than the buffer
    table, ptrs = case.device(dtype)
    h_table, h_caches = case.host(dtype)
    h_ids, d_ids = (case.ids, case.d["ids"]) if ids is None else (ids, _dev(ids))
    dst0 = np.full((total, D), SENTINEL[out_dtype], dtype=ref.BITS[out_dtype])
    idx0 = np.full(total, IDX_SENTINEL, dtype=np.int32)
    dst, cidx = _dev(dst0), _dev(idx0)
    rng_dev = torch.tensor([OFF, cnt], dtype=torch.int32).cuda()
    plan = (ctypes.c_int32 * 3)(-9, -9, -9)
    rc = hip.legion_gather_rows_fmt(_stream(), dtype, out_dtype, _p(table), _p(ptrs), _p(case.d["map"]) if use_map else None, case.cap, D,
                                    case.N, _p(d_ids), _p(case.d["slots"]) if carried else None, _p(cidx), _p(rng_dev), _p(dst), max_rows,
                                    dst_rows, grid_rows, last_op, plan)
    torch.cuda.synchronize()
    assert rc == 0
    want, want_idx = ref.gather(dtype, out_dtype, D, h_table, h_caches, case.node_map if use_map else None, case.cap, h_ids,
                                case.slots if carried else None, OFF, cnt, max_rows, dst_rows, dst0, idx0)
    what = f"{PAIR_IDS[PAIRS.index((dtype, out_dtype))]} D {D} plan {list(plan)} {what}"
    bad = differences(cidx.cpu().numpy(), want_idx, what + " cache_index") or \
        differences(dst.cpu().numpy().view(ref.BITS[out_dtype]), want, what + " dst")
    assert bad is None, bad
    return list(plan)


# ---- a. every instance, one tile per workgroup -----------------------------------------------------------------------------
def single_plan(dtype, out_dtype, D, rows):
    """(format, ROWS) of a launch of a few thousand rows with LEGION_GATHER_ROWS = rows: the override does not apply to F32Scalar
    (always 64) and F32Tail (16 for a launch of few tiles)."""
    f = ref.expected_format(dtype, out_dtype, D)
    return f, {"F32Tail": 16, "F32Scalar": 64}.get(ref.FORMATS[f], rows)


SINGLE_CNT, SINGLE_MAX = 2500, 3000
TAIL64_DS = [5, 7, 9, 15, 17, 102, 254]         # F32Tail at ROWS = 64: rows of at most 1 KB ...
TAIL64_MAX_ROWS = 300_000                       # ... in a launch sized for 4096 tiles of 64 rows and more (of which cnt rows exist)


def check_single(plan, want, max_rows):
    assert plan[:2] == list(want), (plan, want)
    assert plan[2] == min(TARGET_WG, -(-max_rows // plan[1])) and plan[2] * plan[1] >= SINGLE_CNT      # no workgroup has a second tile


@pytest.mark.parametrize("rows", TILES)
@pytest.mark.parametrize("dtype,out_dtype", PAIRS, ids=PAIR_IDS)
def test_every_instance_one_tile_per_workgroup(hip, monkeypatch, cases, dtype, out_dtype, rows):
    with gather_rows_env(hip, monkeypatch, rows):
        for D in DS:
            plan = run(hip, cases(D), dtype, out_dtype, SINGLE_CNT, max_rows=SINGLE_MAX - OFF)
            check_single(plan, single_plan(dtype, out_dtype, D, rows), SINGLE_MAX - OFF)


def test_f32tail_at_64_rows_one_tile_per_workgroup(hip, monkeypatch, cases):
    with gather_rows_env(hip, monkeypatch, 0):
        for D in TAIL64_DS:
            plan = run(hip, cases(D), F32, F32, SINGLE_CNT, max_rows=TAIL64_MAX_ROWS)
            check_single(plan, (ref.FORMATS.index("F32Tail"), 64), TAIL64_MAX_ROWS)


@pytest.mark.parametrize("dtype,out_dtype", PAIRS, ids=PAIR_IDS)
def test_the_instances_of_the_early_gathers(hip, monkeypatch, cases, dtype, out_dtype):
    """last_op = 0: the instances without LASTOP."""
    with gather_rows_env(hip, monkeypatch, 32):
        for D in DS:
            plan = run(hip, cases(D), dtype, out_dtype, SINGLE_CNT, max_rows=SINGLE_MAX - OFF, last_op=0, what="last_op 0")
            check_single(plan, single_plan(dtype, out_dtype, D, 32), SINGLE_MAX - OFF)


@pytest.mark.parametrize("dtype,out_dtype", PAIRS, ids=PAIR_IDS)
def test_carried_slots_are_served(hip, monkeypatch, cases, dtype, out_dtype):
    """node_slot: LG_FS_UNKNOWN on a third of the rows (looked up), and on some rows a slot that is not node_map[id]: the row of the
    carried slot is what the gather serves."""
    with gather_rows_env(hip, monkeypatch, 64):
        for D in DS:
            case = cases(D)
            assert case.differ > 100 and np.sum(case.slots == ref.UNKNOWN) > case.total // 4
            plan = run(hip, case, dtype, out_dtype, SINGLE_CNT, max_rows=SINGLE_MAX - OFF, carried=True, what="carried slots")
            check_single(plan, single_plan(dtype, out_dtype, D, 64), SINGLE_MAX - OFF)


# ---- b. the walk -------------------------------------------------------------------------------------------------------------
WALK_ROWS = {16: 300_017, 32: 530_001, 64: 1_200_003, 128: 2_200_005, 256: 4_300_007}      # just above 2 * 8192 * ROWS
# (dtype, out_dtype, LEGION_GATHER_ROWS, D, cnt, grid_rows, (format, ROWS) meant)
WALK = []
for _pair in PAIRS:
    _f = ref.expected_format(*_pair, 8)
    WALK += [(*_pair, r, 8, WALK_ROWS[r], 0, (_f, r)) for r in TILES]                           # one chunk per row
    WALK += [(*_pair, r, D, WALK_ROWS[r], 0, (_f, r)) for r in (16, 32) for D in (24, 100)]     # dc != 0; a partial last chunk per row
WALK += [
    # F32Tail at 16 rows: D > 256, D % 4 != 0.  140 000 rows are 8750 tiles; the grid is sized for 65 536 rows (4096 workgroups), as
    # for a lane that has more rows than lanes typically have, so that the first workgroups take a third tile
    (F32, F32, 0, 258, 140_000, 65_536, (ref.FORMATS.index("F32Tail"), 16)),
    (F32, F32, 0, 3, 1_200_003, 0, (ref.FORMATS.index("F32Scalar"), 64)),
    (F32, F32, 0, 7, 1_200_003, 0, (ref.FORMATS.index("F32Tail"), 64)),
]
WALK_IDS = [f"{PAIR_IDS[PAIRS.index((a, b))]}-{ref.FORMATS[m[0]]}-rows{m[1]}-D{D}" for a, b, _, D, _, _, m in WALK]


@pytest.mark.parametrize("dtype,out_dtype,env_rows,D,cnt,grid_rows,meant", WALK, ids=WALK_IDS)
def test_the_walk_over_more_than_two_tiles_per_workgroup(hip, monkeypatch, cases, dtype, out_dtype, env_rows, D, cnt, grid_rows, meant):
    """One launch whose lane has more than twice as many tiles as the launch has workgroups, and a partial last tile: the first
    workgroups copy three tiles, so the ids fetched two tiles ahead, the slot lookups one tile ahead, both LDS pointer buffers and
    the late cache_index writes are all in use.  Cases of D = 24 carry slots as well (they are prefetched with the ids)."""
    case = cases(D, N=40_000, cap=4_500, total=OFF + cnt + 50)
    with gather_rows_env(hip, monkeypatch, env_rows):
        plan = run(hip, case, dtype, out_dtype, cnt, grid_rows=grid_rows, carried=(D == 24), what="walk")
    assert plan[:2] == list(meant), (plan, meant)
    tiles = -(-cnt // plan[1])
    assert tiles > 2 * plan[2] and (cnt % plan[1] != 0 or D == 258), (tiles, plan)      # (140 000 rows end on a full tile of 16)


def test_the_cases_cover_every_instance():
    """Every (format, ROWS) of GATHER_FORMATS' tile masks (read from gather_plan.h) is meant by a one-tile case and by a walk case;
    each case checks what it means against plan_out."""
    text = open(os.path.join(ROOT, "legion_amd", "csrc", "gather_plan.h")).read()
    table = re.findall(r"^\s*\{\d+, (?:true|false), (?:true|false), ([0-9 |]+)\},?\s*// (\w+):", text, flags=re.M)
    assert [name for _, name in table] == list(ref.FORMATS)
    masks = {(ref.FORMATS.index(name), int(r)) for tiles, name in table for r in tiles.split("|")}
    assert len(masks) == 23
    single = {single_plan(a, b, D, r) for a, b in PAIRS for r in TILES for D in DS} | {(ref.FORMATS.index("F32Tail"), 64)}
    assert single == masks, sorted(single ^ masks)
    walk = {m for *_, m in WALK}
    assert walk == masks, sorted(walk ^ masks)


# ---- c. clamps and refusals -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,out_dtype", PAIRS, ids=PAIR_IDS)
def test_clamps(hip, monkeypatch, cases, dtype, out_dtype):
    """max_rows < cnt and dst_rows - OFF < cnt: the rows past the clamp keep their sentinel (run() compares the whole buffer); cnt = 0
    and max_rows = 0 write nothing."""
    with gather_rows_env(hip, monkeypatch, 0):
        for D in (9, 100):
            case = cases(D)
            f = ref.expected_format(dtype, out_dtype, D)
            assert run(hip, case, dtype, out_dtype, SINGLE_CNT, max_rows=1001, what="max_rows")[0] == f
            assert run(hip, case, dtype, out_dtype, SINGLE_CNT, dst_rows=OFF + 777, what="dst_rows")[0] == f
            assert run(hip, case, dtype, out_dtype, SINGLE_CNT, max_rows=1001, dst_rows=OFF + 1500, what="both")[0] == f
            assert run(hip, case, dtype, out_dtype, SINGLE_CNT, dst_rows=OFF - 5, what="dst_rows < off")[0] == f
            assert run(hip, case, dtype, out_dtype, 0, max_rows=SINGLE_CNT, what="cnt 0")[0] == f
            assert run(hip, case, dtype, out_dtype, SINGLE_CNT, max_rows=0, what="max_rows 0") == [-1, 0, 0]      # nothing launched


@pytest.mark.parametrize("dtype,out_dtype", PAIRS, ids=PAIR_IDS)
def test_no_node_map_every_row_a_miss(hip, monkeypatch, cases, dtype, out_dtype):
    """node_map = NULL: every row comes from the full table (ids >= N wrap, as in the reference's modulo), carried slots are not read."""
    with gather_rows_env(hip, monkeypatch, 0):
        for D in (9, 100):
            case = cases(D)
            ids = case.ids.copy()
            ids[5::13] += case.N
            ids[::97] = -1
            for carried in (False, True):
                plan = run(hip, case, dtype, out_dtype, SINGLE_CNT, use_map=False, carried=carried, ids=ids, what="no node_map")
                assert plan[0] == ref.expected_format(dtype, out_dtype, D)


@pytest.mark.parametrize("dtype,out_dtype", [(2, F32), (F32, 2), (-1, BF16), (BF16, 7)])
def test_an_unknown_dtype_is_refused(hip, cases, dtype, out_dtype):
    case = cases(100)
    table, ptrs = case.device(F32)
    dst = torch.full((case.total, case.D), -7.0, dtype=torch.float32).cuda()
    cidx = torch.full((case.total,), IDX_SENTINEL, dtype=torch.int32).cuda()
    rng_dev = torch.tensor([OFF, SINGLE_CNT], dtype=torch.int32).cuda()
    plan = (ctypes.c_int32 * 3)(-9, -9, -9)
    rc = hip.legion_gather_rows_fmt(_stream(), dtype, out_dtype, _p(table), _p(ptrs), _p(case.d["map"]), case.cap, case.D, case.N,
                                    _p(case.d["ids"]), None, _p(cidx), _p(rng_dev), _p(dst), SINGLE_CNT, case.total, 0, 1, plan)
    torch.cuda.synchronize()
    assert rc == -1 and list(plan) == [-9, -9, -9]
    assert bool((dst == -7.0).all()) and bool((cidx == IDX_SENTINEL).all())
