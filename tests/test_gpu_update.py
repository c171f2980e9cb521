"""legion_row_update and FeatureStorage.update_rows on the GPU against tests/update_ref.py.  In the exact cases gradients are small
integers and lr is a power of two: the sum of an id's rows is exact in any order, and every later step is one correctly rounded
float32 operation that numpy repeats, so the table, the cache copy and the state must match bit for bit, over the whole arrays (rows
no id names are unchanged).  Cache rows differ from the table's by 1000, so a wrong target shows."""
import ctypes

import numpy as np
import pytest
import torch

from tests import update_ref as ref
from tests.compare import same_arrays

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

DEV = "cuda:0"
K = 256
CODE = {"sum": 0, "mean": 1, "sgd": 0, "adagrad": 1, "adam": 2}
WAVES = 2048 * 4                                                       # the grid's waves: chunks past them are a second trip
NEEDS = {"sgd": (), "adagrad": ("state1",), "adam": ("state1", "state2", "state_pow")}


def fresh(N, D, optimizer, rng):
    """{table: integers and halves, the optimizer's state as the caller initialises it}."""
    arrays = {k: (np.ones((N, 2), np.float32) if k == "state_pow" else np.zeros((N, D), np.float32)) for k in NEEDS[optimizer]}
    return dict(arrays, table=(rng.integers(-16, 17, (N, D)) / 2).astype(np.float32))


def pattern(N, rng):
    """All ids once, a hub of 20 K + 3 entries, a Zipf-like mix, and dead ids (-1, N, 2^31 - 1) sprinkled in; shuffled."""
    ids = np.concatenate([np.arange(N), np.full(20 * K + 3, 7), (N * rng.random(2000) ** 4).astype(np.int64),
                          np.resize(np.array([-1, N, 2 ** 31 - 1]), 90)]).astype(np.int32)
    return rng.permutation(ids)


def run(L, arrays, ids, grads, combine, optimizer, lr, node_map=None):
    """The C ABI on copies of the arrays (table, the state, cache), each with a sentinel row behind it, and a scratch filled with NaN
    bits.  Returns the new arrays as numpy."""
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    (N, D), m = arrays["table"].shape, ids.size
    d = {k: torch.from_numpy(np.concatenate([a, np.full((1, a.shape[1]), -12288.0, np.float32)])).to(DEV) for k, a in arrays.items()}
    d_map = torch.from_numpy(node_map).to(DEV) if node_map is not None else None
    d_ids = torch.from_numpy(np.resize(ids, max(m, 1))).to(DEV)        # (m == 0: still an address)
    d_grads = torch.from_numpy(np.resize(grads, (max(m, 1), D))).to(DEV)
    nbytes = int(L.legion_row_update_scratch_bytes(m, N, D))
    scratch = torch.full((nbytes // 8 + 2,), -1, dtype=torch.int64, device=DEV)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.legion_row_update(s, P(d["table"]), P(d.get("cache")), P(d_map), D, N, P(d_ids), P(d_grads), m, CODE[combine], CODE[optimizer],
                               lr, 1e-10, 0.9, 0.999, P(d.get("state1")), P(d.get("state2")), P(d.get("state_pow")), P(scratch), nbytes) == 0
    torch.cuda.synchronize()
    out = {k: t.cpu().numpy() for k, t in d.items()}
    assert all(np.all(a[-1] == -12288.0) for a in out.values()), "written past a last row"
    return {k: a[:-1] for k, a in out.items()}


def check(L, arrays, ids, grads, combine, optimizer, lr, what, node_map=None):
    """One step on the GPU equals one step of the reference, bit for bit, everywhere; returns the new arrays."""
    got = run(L, arrays, ids, grads, combine, optimizer, lr, node_map)
    want = {k: a.copy() for k, a in arrays.items()}
    ref.update(want["table"], ids, grads, combine, optimizer, lr, state=want, node_map=node_map, cache=want.get("cache"))
    same_arrays([got[k].view(np.uint32) for k in want], [want[k].view(np.uint32) for k in want], what, list(want))
    return want


@pytest.mark.parametrize("combine", ["sum", "mean"])
@pytest.mark.parametrize("optimizer", ["sgd", "adagrad", "adam"])
@pytest.mark.parametrize("D", [1, 3, 4, 100, 128, 260])
def test_exact_at_every_row_width(hip, D, optimizer, combine):
    rng = np.random.default_rng(D)
    ids = pattern(300, rng)
    grads = rng.integers(-4, 5, (ids.size, D)).astype(np.float32)
    check(hip, fresh(300, D, optimizer, rng), ids, grads, combine, optimizer, 0.25, f"D {D} {optimizer} {combine}")


@pytest.mark.parametrize("N", [200, 300, 70000])                       # 1, 2 and 3 sort passes
@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 1023, 1024, 1025, 3 * 1024 + 5])
def test_exact_at_every_count_and_pass_count(hip, m, N):
    rng = np.random.default_rng(m + N)
    ids = rng.integers(-1, N + 1, m).astype(np.int32)                  # -1 and N: dead
    ids[: m // 3] = ids[0] if m else 0                                 # and one id many times
    grads = rng.integers(-4, 5, (m, 4)).astype(np.float32)
    check(hip, fresh(N, 4, "adam", rng), rng.permutation(ids), grads, "mean", "adam", 0.5, f"m {m} N {N}")


def test_exact_with_four_sort_passes(hip):
    rng = np.random.default_rng(24)
    N = 2 ** 24 + 3
    ids = np.concatenate([rng.integers(0, N, 3000), [N - 1, N - 1, 0, 2 ** 24, 2 ** 24, N, -1]]).astype(np.int32)
    grads = rng.integers(-4, 5, (ids.size, 1)).astype(np.float32)
    check(hip, fresh(N, 1, "adagrad", rng), ids, grads, "sum", "adagrad", 0.5, "N 2^24 + 3")


@pytest.mark.parametrize("optimizer", ["sgd", "adagrad", "adam"])
def test_the_cache_copy_is_written_with_the_table(hip, optimizer):
    rng = np.random.default_rng(5)
    N, D = 300, 128
    arrays = fresh(N, D, optimizer, rng)
    node_map = np.where(np.arange(N) % 3 == 0, np.arange(N) // 3, -2).astype(np.int32)      # a third of the rows are cached
    arrays["cache"] = arrays["table"][::3] + np.float32(1000)
    ids = pattern(N, rng)[:4000]                                       # not every row: uncached and unnamed rows stay
    grads = rng.integers(-4, 5, (ids.size, D)).astype(np.float32)
    check(hip, arrays, ids, grads, "mean", optimizer, 0.25, f"cache {optimizer}", node_map)


def test_more_groups_than_the_grid_has_waves(hip):
    rng = np.random.default_rng(7)
    m, N = WAVES * 4 + 7, 70000
    arrays = fresh(N, 4, "sgd", rng)
    ids = rng.permutation(N)[:m].astype(np.int32)
    check(hip, arrays, ids, rng.integers(-4, 5, (m, 4)).astype(np.float32), "sum", "sgd", 0.5, "past the grid")


@pytest.mark.parametrize("optimizer", ["adagrad", "adam"])
def test_a_second_step_starts_from_the_first_step_s_state(hip, optimizer):
    rng = np.random.default_rng(9)
    arrays = fresh(300, 100, optimizer, rng)
    for step in range(2):
        ids = pattern(300, rng)[:3000]
        grads = rng.integers(-4, 5, (ids.size, 100)).astype(np.float32)
        arrays = check(hip, arrays, ids, grads, "mean", optimizer, 0.25, f"{optimizer} step {step}")
    if optimizer == "adam":
        assert len(np.unique(arrays["state_pow"][:, 0])) == 3, "rows stepped 0, 1 and 2 times"


def test_random_floats_twice_the_same_bits_and_within_the_bound_of_a_float32_sum(hip):
    """SGD, combine = sum, u = 2^-24.  g = fl(sum of len rows) in any order: |g - S| <= (len - 1) u sum|g_i| to first order, the
    aggregation's bound (len + 2) u sum|g_i| with its slack.  p = fl(lr g): |p - lr S| <= lr (len + 2) u sum|g_i| (the product's
    one rounding is inside the slack).  w' = fl(w - p): |w' - (w - p)| <= u |w - p|, and |w - p| <= |w_ref| (1 + tiny) + the
    error of p.  Together |w' - w_ref| <= lr (len + 2) 2^-24 sum|g_i| + 2^-23 |w_ref|.  Measured: 0.48 of it at most."""
    rng = np.random.default_rng(11)
    N, D, lr = 300, 128, 0.05
    arrays = {"table": rng.standard_normal((N, D)).astype(np.float32)}
    ids = pattern(N, rng)
    grads = rng.standard_normal((ids.size, D)).astype(np.float32)
    got = run(hip, arrays, ids, grads, "sum", "sgd", lr)["table"]
    same_arrays(run(hip, arrays, ids, grads, "sum", "sgd", lr)["table"].view(np.uint32), got.view(np.uint32), "the same call twice")
    uniq, sums, count = ref.combine(ids, grads, N)
    _, mass, _ = ref.combine(ids, np.abs(grads), N)
    want = arrays["table"].astype(np.float64)
    want[uniq] -= float(np.float32(lr)) * sums
    bound = 2.0 ** -23 * np.abs(want)
    bound[uniq] += float(np.float32(lr)) * (count[:, None] + 2) * 2.0 ** -24 * mass
    err = np.abs(got.astype(np.float64) - want)
    assert count.max() > 20 * K and np.all(err <= bound), float(np.max(err - bound))


def test_the_python_surface(hip):
    """update_rows with each optimizer and its state dict, and a served batch after the updates: the gather returns the new rows,
    those it resolves through the cache included."""
    from tests.gpu_harness import GpuSide
    from tests.helpers import Workload
    wl = Workload(scale=10, edge_factor=8, dim=32, n_seeds=600)
    gpu = GpuSide(wl, 64, [5, 4])
    try:
        for it in range((wl.sets[(0, 0)][0].size - 1) // 64):
            gpu.run(0, it, 0, is_presc=True)
        gpu.cache.candidate_selection(0, gpu.graph)
        gpu.cache.set_capacity(200, 100)
        gpu.cache.fill_up(gpu.feature, gpu.graph)
        rng = np.random.default_rng(3)
        table, states, wants = wl.features.copy(), {}, {}
        for optimizer in ("sgd", "adagrad", "adam", "adam"):
            ids = rng.integers(-1, wl.N + 1, 5000).astype(np.int32)
            grads = rng.integers(-4, 5, (ids.size, wl.D)).astype(np.float32)
            state = gpu.feature.update_rows(torch.from_numpy(ids).to(DEV), grads, optimizer=optimizer, lr=0.125, state=states.get(optimizer),
                                            cache=gpu.cache)
            assert sorted(state) == sorted(NEEDS[optimizer]) and states.setdefault(optimizer, state) is state
            want = wants.setdefault(optimizer, fresh(wl.N, wl.D, optimizer, rng))
            ref.update(table, ids, grads, "mean", optimizer, 0.125, state=want)
            same_arrays([gpu.features] + [state[k] for k in state], [table] + [want[k] for k in state], optimizer, ["table"] + list(state))
        assert gpu.feature.update_rows(np.zeros(0, np.int32), np.zeros((0, wl.D), np.float32), lr=1.0) == {}
        out = gpu.run(0, 0, 0)
        assert (out["cache_search_buffer"] >= 0).sum() > 0, "some rows are gathered from the cache"
        assert np.mean(np.any(table[out["sampled_ids"]] != wl.features[out["sampled_ids"]], axis=1)) > 0.9, "nearly every row was stepped"
        same_arrays(out["float_features"], table[out["sampled_ids"]], "the gather after the updates")
    finally:
        torch.cuda.synchronize()
        gpu.close()
