"""The seeded random shapes of tests/test_gpu_fuzz.py through the opt-in modes and their 24 combinations -- the draw (with
replacement, without, weighted) x edge ids x float32 / bfloat16 feature storage x float32 / bfloat16 rows out -- against the
composed CPU reference of tests/mode_ref.py, bit for bit: plain enqueue without a cache, the whole PreSC -> cost model -> fill ->
lane-group Pipeline path, striped cliques of 2 and 4 logical GPUs (with and without a replica) and the hybrid tier.

A case's combination is (case seed // 4) % 16 for the seeds below 1024 and 16 + (case seed // 4) % 8, a weighted one, from 1024 on
(random_case takes the graph kind from seed % 4, so the two do not alias), and a case whose seed is odd has 5 % of its column
entries dead (-1).  A weighted case's weights are mode_ref.case_weights of its seed.  Before anything runs on the GPU each test's
seed set is checked, from the reference alone, to exercise what it is there for (see _conditions_*; tests/test_mode_ref_cpu.py
checks the weighted lists without a GPU): a seed set that does not is replaced, never the condition.  A failure names the seed,
the combination and the shape."""
import functools

import numpy as np
import pytest

from oracle import ffi
from tests import mode_ref, weighted_ref
from tests.gpu_harness import GpuSide
from tests.helpers import Workload
from tests.test_gpu_fuzz import random_case

pytestmark = pytest.mark.gpu

# case seeds: (seed // 4) % 16 is the combination, seed % 4 random_case's graph kind
# a: every (graph kind, combination) pair once.  0..63, but for four seeds whose combination samples without replacement and whose
# four shapes of 0..63 have no D > f frontier entry across two super tiles that shows the carried prefix (_conditions_a): the same
# pair 64 k further on, where one has
SEEDS_A = [{35: 163, 39: 103, 55: 311, 59: 187}.get(s, s) for s in range(64)]
SEEDS_B = [128 + 4 * i + (i + i // 4) % 4 for i in range(16)]           # one per combination, the kinds going round
SEEDS_C = [320 + 4 * i + (i + i // 4 + 1) % 4 for i in range(16)]
# the weighted combinations: 16 + (seed // 4) % 8
WEIGHTED_SEEDS = 1024
SEEDS_AW = list(range(1024, 1056))                                      # every (graph kind, weighted combination) pair once
# b: one per weighted combination, the kinds going round; but 1169, a graph of 95 edges sampled one seed at a time whose served
# batches are those of unit weights (_conditions_b_weighted): the same pair 32 further on
SEEDS_BW = [{1169: 1201}.get(s, s) for s in (1152 + 4 * i + (i + i // 4) % 4 for i in range(8))]
# c: case i has the combination 16 + i % 8 and _case_c's clique / replica / hybrid of i; its seed is the first of 1280 + 4 * (i % 8)
# + 32 k + kind, k = 0, 1, .., kind = 0 .. 3, not taken by an earlier case, whose case meets what _conditions_c_weighted asks of it
# (a striped case: its own three sources and the wrong-base row; the hybrid cases 2, 5 and 11: both tiers, 2 and 11: over four hops)
SEEDS_CW = [1283, 1286, 1320, 1292, 1299, 1300, 1306, 1310, 1280, 1287, 1291, 1325, 1331, 1302, 1304, 1311]


def _combo(case_seed):
    if case_seed >= WEIGHTED_SEEDS:
        return mode_ref.COMBOS[16 + (case_seed // 4) % 8]
    return mode_ref.COMBOS[(case_seed // 4) % 16]


def _weighted(combo):
    return combo["draw"] == "weighted"


def _gpu_modes(combo):
    return dict(replace=combo["replace"], edge_ids=combo["edge_ids"], feature_dtype=combo["storage"], feature_out_dtype=combo["out"],
                weighted=_weighted(combo))


def _workload(case_seed, max_hops=4, P=1, min_dim=1):
    c = random_case(case_seed, max_hops)
    col = mode_ref.with_dead_columns(c["col"], case_seed) if case_seed % 2 else c["col"]
    wl = Workload(dim=max(c["dim"], min_dim), n_seeds=c["n_seeds"], n_valid=c["n_valid"], n_test=c["n_test"], partition_count=P,
                  indptr=c["indptr"], col=col)
    combo = _combo(case_seed)
    weights = mode_ref.case_weights(wl.indptr, case_seed) if _weighted(combo) else None
    ctx = (f"seed {case_seed} [{mode_ref.combo_name(combo)}] (N {wl.N}, E {wl.E}, dead {int((col < 0).sum())}, fan-out {c['fanout']}, "
           f"batch {c['batch']}, D {wl.D}, P {P}")
    return c, wl, combo, weights, ctx


def _n_batches(wl, dev, mode, batch):
    return (wl.sets[(dev, mode)][0].size + batch - 1) // batch + 1                # one past the end: the empty batch


def _presc(wl, cpu, combo, batch, fanout, weights=None):
    """The reference's PreSC epoch on every partition: (batches {(p, it): want}, node hotness [P], edge hotness [P], max ids [P],
    steps)."""
    steps = max(min((wl.sets[(p, 0)][0].size - 1) // batch for p in range(wl.P)), 1)
    na = [np.zeros(wl.N, np.uint64) for _ in range(wl.P)]
    ea = [np.zeros(wl.N, np.uint64) for _ in range(wl.P)]
    wants, max_ids = {}, [0] * wl.P
    for p in range(wl.P):
        for it in range(steps):
            w = mode_ref.expected_batch(wl, p, it, 0, batch, fanout, serve=False, edge_access=ea[p], node_access=na[p], cpu=cpu,
                                        weights=weights, **combo)
            max_ids[p] = max(max_ids[p], int(w["node_counter"][7]))
            wants[(p, it)] = w
    return wants, na, ea, max_ids, steps


def _oracle_caches(wl, combo, na, ea, mode_bits, capacity):
    """One filled OracleCache per clique of 2^mode_bits partitions, from the per-partition hotness."""
    Kg = min(1 << mode_bits, wl.P)
    table = mode_ref.served_table(wl, combo["storage"])
    caches = []
    for ki in range(wl.P // Kg):
        oc = ffi.OracleCache(wl.N, wl.D, Kg, ki)
        oc.candidate_selection(na[ki * Kg:(ki + 1) * Kg], ea[ki * Kg:(ki + 1) * Kg])
        oc.set_capacity(*capacity)
        oc.fill_up(table, wl.indptr, wl.col)
        caches.append(oc)
    return caches


def _topo_owner(oc, frontier):
    """FindTopo's hit mask of a frontier on an oracle cache: the partition that caches the row, or -2."""
    fr = np.asarray(frontier, dtype=np.int64)
    owner = oc.arr("edge_index_map", np.int8)
    return np.where(fr >= 0, owner[np.maximum(fr, 0)], np.int8(-2)).astype(np.int8)


def _differs_from_unit_weights(wl, combo, batch, fanout, served):
    """Is one of the served weighted batches (dev, mode, it, want) another one under unit weights?  If none is, the weights are not
    being used."""
    unit = mode_ref.unit_weights(wl.indptr)
    for dev, mode, it, want in served:
        other = mode_ref.expected_batch(wl, dev, it, mode, batch, fanout, weights=unit, **combo)
        if not (np.array_equal(other["agg_src_ids"], want["agg_src_ids"]) and np.array_equal(other["agg_dst_ids"], want["agg_dst_ids"])):
            return True
    return False


def _gpu_side(case, **kw):
    """The case's GpuSide in its combination's modes; a weighted case's table is the reference's bit for bit."""
    wl, weights = case["wl"], case["weights"]
    gpu = GpuSide(wl, case["c"]["batch"], case["c"]["fanout"], weights=weights.w if weights else None, **_gpu_modes(case["combo"]), **kw)
    if weights:
        assert np.array_equal(gpu.graph.edge_cdf().cpu().numpy().view(np.uint32), weights.table.view(np.uint32)), case["ctx"] + "): edge_cdf"
        assert all(pool.weighted for pool in gpu.pools)
    else:
        assert gpu.graph.edge_cdf() is None and not any(pool.weighted for pool in gpu.pools)
    return gpu


def _run_presc_on_gpu(gpu, case, ctx):
    wl = case["wl"]
    for (p, it), want in case["presc"].items():
        mode_ref.compare_mode_batch(gpu.run(p, it, 0, is_presc=True), want, wl, ctx + f"presc gpu {p} batch {it}: ")
    for p in range(wl.P):
        assert np.array_equal(gpu.cache.array("edge_access_time", p).cpu().numpy().view(np.uint64), case["ea"][p]), ctx + f"edge hotness {p}"
        assert np.array_equal(gpu.cache.array("node_access_time", p).cpu().numpy().view(np.uint64), case["na"][p]), ctx + f"node hotness {p}"
        assert gpu.cache.max_id_num(p) == case["max_ids"][p], ctx + f"max ids {p}"


def _check_topo_mask(pool, want, hops, oc, ctx):
    frontier = mode_ref.hop_frontiers(want, hops)[-1]
    got = pool.buffer("tmp_part_ind")[:frontier.size].cpu().numpy()
    assert np.array_equal(got, _topo_owner(oc, frontier)), ctx + "tmp_part_ind of the last hop"


# ---- a. plain enqueue, no cache ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case_a(case_seed):
    c, wl, combo, weights, ctx = _workload(case_seed)
    batch, fanout = c["batch"], c["fanout"]
    cpu = mode_ref.cpu_side(wl, batch, fanout, combo["storage"])
    wants, stats = {}, {}
    for mode in (0, 1, 2):
        for it in range(_n_batches(wl, 0, mode, batch)):
            wants[(mode, it)] = mode_ref.expected_batch(wl, 0, it, mode, batch, fanout, cpu=cpu, weights=weights, **combo)
            mode_ref.add_stats(stats, mode_ref.batch_stats(wl, wants[(mode, it)], fanout, distinct=not combo["replace"], weights=weights))
    cpu.close()
    if weights:
        stats["differs"] = int(_differs_from_unit_weights(wl, combo, batch, fanout, ((0, m, it, w) for (m, it), w in wants.items())))
    return dict(c=c, wl=wl, combo=combo, weights=weights, ctx=ctx, wants=wants, stats=stats)


def _conditions_weighted(name, s):
    """What every weighted combination saw over its cases: a frontier entry with D > f, one with D = 0, an empty batch, an entry
    with D > 0 whose row total is 0 (it yields no edge), a sampled row that holds zero-weight entries beside positive ones, a
    sampled dead column, and a served batch that is another one under unit weights."""
    assert s["over"] > 0 and s["zero"] > 0 and s["empty"] > 0, f"{name}: {s}"
    assert s["zero_total"] > 0 and s["mixed"] > 0 and s["dead"] > 0 and s["differs"] > 0, f"{name}: {s}"


def _conditions_a(cases, n_combos=16):
    """Every combination saw a frontier entry with D > f, one with D = 0 and an empty batch; every distinct combination an entry
    with D > f whose slots straddle two super tiles of the sampler AND whose later picks depend on the earlier tile's (a later slot
    draws a position an earlier one took: only then does the carried-over prefix show in the batch); dead columns were sampled.
    Every weighted combination: _conditions_weighted, and every one of its cases differs from its unit-weights twin."""
    per_combo = {}
    for case in cases:
        assert not case["weights"] or case["stats"]["differs"], case["ctx"] + "): the batches are those of unit weights"
        mode_ref.add_stats(per_combo.setdefault(mode_ref.combo_name(case["combo"]), {"replace": case["combo"]["replace"],
                                                                                     "weighted": _weighted(case["combo"])}),
                           {k: v for k, v in case["stats"].items()})
    assert len(per_combo) == n_combos
    for name, s in per_combo.items():
        assert s["over"] > 0 and s["zero"] > 0 and s["empty"] > 0, f"{name}: {s}"
        assert s["replace"] or s["carry"] > 0, f"{name}: no D > f entry across two super tiles whose picks depend on the carried prefix: {s}"
        if s["weighted"]:
            _conditions_weighted(name, s)
    assert sum(s["dead"] for s in per_combo.values()) > 0
    return per_combo


@pytest.fixture(scope="module")
def cases_a():
    cases = {s: _case_a(s) for s in SEEDS_A}
    _conditions_a(cases.values())
    return cases


@pytest.fixture(scope="module")
def cases_aw():
    cases = {s: _case_a(s) for s in SEEDS_AW}
    _conditions_a(cases.values(), 8)
    return cases


def _run_a(case, buckets):
    wl = case["wl"]
    ctx = case["ctx"] + f", {buckets} buckets): "
    gpu = _gpu_side(case)
    for (mode, it), want in case["wants"].items():
        mode_ref.compare_mode_batch(gpu.run(0, it, mode), want, wl, ctx + f"mode {mode} batch {it}: ")
    assert gpu.pools[0].error() == 0, ctx
    gpu.close()


@pytest.mark.parametrize("seed", SEEDS_A)
def test_random_shapes_every_mode(hip, buckets, cases_a, seed):
    _run_a(cases_a[seed], buckets)


@pytest.mark.parametrize("seed", SEEDS_AW)
def test_random_shapes_every_weighted_mode(hip, buckets, cases_aw, seed):
    _run_a(cases_aw[seed], buckets)


# ---- b. PreSC -> cost model -> fill -> lane groups under graph replay ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case_b(i, weighted=False):
    from legion_amd import engine
    case_seed = (SEEDS_BW if weighted else SEEDS_B)[i]
    c, wl, combo, weights, ctx = _workload(case_seed, min_dim=3)
    batch, fanout = c["batch"], c["fanout"]
    rng = np.random.RandomState(7000 + case_seed)
    cache_memory = int(rng.choice([20_000, 200_000, 2_000_000]))
    counters = (int(rng.randint(0, 50_000)), int(rng.randint(0, 50_000))) if i % 2 else (0, 0)
    group, slots = int(rng.randint(1, 6)), int(rng.randint(1, 4))
    weave = bool(rng.randint(0, 3))
    cpu = mode_ref.cpu_side(wl, batch, fanout, combo["storage"])
    presc, na, ea, max_ids, steps = _presc(wl, cpu, combo, batch, fanout, weights)
    # D enters the cost model only as row bytes: a bf16 storage's rows are round_up(D, 8) * 2 bytes
    cm = ffi.OracleCache(wl.N, engine.bf16_pitch(wl.D) // 2 if combo["storage"] == "bfloat16" else wl.D, 1, 0)
    cm.candidate_selection(na, ea)
    cm.cost_model(cache_memory, wl.indptr, counters, max_ids, steps)
    capacity = (cm.node_capacity, cm.edge_capacity)
    cm.close()
    oc = _oracle_caches(wl, combo, na, ea, 0, capacity)[0]
    wants, stats = {}, {"topo": 0}
    for mode in (0, 1):
        n = _n_batches(wl, 0, mode, batch)
        for it in range((n + group - 1) // group * group):              # every lane of the last group: empty batches past the end
            w = wants[(mode, it)] = mode_ref.expected_batch(wl, 0, it, mode, batch, fanout, cpu=cpu, weights=weights, **combo)
            mode_ref.add_stats(stats, mode_ref.batch_stats(wl, w, fanout, weights=weights))
            stats["topo"] += int((_topo_owner(oc, mode_ref.hop_frontiers(w, len(fanout))[-1]) >= 0).sum())
    cpu.close()
    if weights:
        stats["differs"] = int(_differs_from_unit_weights(wl, combo, batch, fanout, ((0, m, it, w) for (m, it), w in wants.items())))
    ctx += f", cache {cache_memory} -> {capacity}, group {group} x {slots} {'weave' if weave else 'one-stream'}"
    return dict(c=c, wl=wl, combo=combo, weights=weights, ctx=ctx, presc=presc, na=na, ea=ea, max_ids=max_ids, steps=steps,
                cache_memory=cache_memory, counters=counters, capacity=capacity, oc=oc, group=group, slots=slots, weave=weave, wants=wants,
                stats=stats)


def _conditions_b_weighted(cases):
    """The weighted cases of section b: one per weighted combination, each with batches that unit weights would make other ones;
    over all of them _conditions_weighted, rows served from the cached topology, more than one lane and slot, both stream
    arrangements, and cost models with and without counters."""
    cases = list(cases)
    assert {mode_ref.combo_name(case["combo"]) for case in cases} == {mode_ref.combo_name(c) for c in mode_ref.COMBOS[16:]}
    total = {}
    for case in cases:
        assert case["stats"]["differs"], case["ctx"] + "): the batches are those of unit weights"
        mode_ref.add_stats(total, case["stats"])
    _conditions_weighted("section b", total)
    assert total["topo"] > 0
    assert max(case["group"] for case in cases) > 1 and max(case["slots"] for case in cases) > 1
    assert {case["weave"] for case in cases} == {True, False}
    assert any(case["capacity"][1] > 0 for case in cases) and any(case["capacity"][0] > 0 for case in cases)
    return total


def _run_b(case, buckets):
    from legion_amd import engine
    c, wl, combo = case["c"], case["wl"], case["combo"]
    batch, fanout, group = c["batch"], c["fanout"], case["group"]
    ctx = case["ctx"] + f", {buckets} buckets): "
    gpu = _gpu_side(case, cache_memory=case["cache_memory"])
    _run_presc_on_gpu(gpu, case, ctx)
    gpu.cache.candidate_selection(0, gpu.graph)
    gpu.cache.cost_model(gpu.feature, gpu.graph, case["counters"], case["steps"])
    assert (gpu.cache.node_capacity(0), gpu.cache.edge_capacity(0)) == case["capacity"], ctx + "capacities"
    gpu.cache.fill_up(gpu.feature, gpu.graph)
    pipe = engine.Pipeline(gpu.graph, gpu.feature, gpu.cache, 0, batch, fanout, group, gpu.pools[0].num_ids, True, case["slots"],
                           weave=case["weave"], feature_out_dtype=combo["out"], replace=combo["replace"], edge_ids=combo["edge_ids"],
                           weighted=_weighted(combo))
    assert pipe.weighted is _weighted(combo)
    for mode in (0, 1):
        for g0 in range(0, _n_batches(wl, 0, mode, batch), group):
            sl = pipe.submit(g0, mode)
            pipe.wait(sl)
            for lane in range(group):
                at = ctx + f"mode {mode} batch {g0 + lane} (lane {lane}): "
                want = case["wants"][(mode, g0 + lane)]
                mode_ref.compare_mode_batch(engine.read_batch(pipe.pools[sl][lane]), want, wl, at)
                _check_topo_mask(pipe.pools[sl][lane], want, len(fanout), case["oc"], at)
    if _weighted(combo):
        with pytest.raises(RuntimeError):
            pipe.set_weighted(False)                    # the captured graphs never mix modes
        with pytest.raises(RuntimeError):
            gpu.graph.set_edge_weights(case["weights"].w)                # ... and the table they read stays
    assert all(p.error() == 0 for row in pipe.pools for p in row), ctx
    pipe.close()
    gpu.close()


@pytest.mark.parametrize("seed", range(16))
def test_random_shapes_modes_through_cache_and_pipeline(hip, buckets, seed):
    _run_b(_case_b(seed), buckets)


@pytest.fixture(scope="module")
def cases_bw():
    cases = {i: _case_b(i, True) for i in range(len(SEEDS_BW))}
    _conditions_b_weighted(cases.values())
    return cases


@pytest.mark.parametrize("seed", range(len(SEEDS_BW)))
def test_random_shapes_weighted_modes_through_cache_and_pipeline(hip, buckets, cases_bw, seed):
    _run_b(cases_bw[seed], buckets)


# ---- c. striped cliques (with and without a replica) and the hybrid tier -------------------------------------------------------
def _cached_start(oc, owner, v):
    """Where row v starts in the cached column array of the clique member `owner` that holds it."""
    cache = oc.c.contents
    starts = np.ctypeslib.as_array(cache.topo_indptr[int(owner) - cache.Ki * cache.Kg], shape=(cache.edge_capacity + 1,))
    return int(starts[int(cache.edge_offset_map[int(v)])])


def _picks_at_base(table, base, D, q, f):
    """The sampler's weighted picks of frontier entry q (slots q*f + k, k < min(f, D)) with its row's table read at `base`: the
    search of draw_rule.h (weighted_target, weighted_step) restated, which -- unlike a library search -- is defined on a range
    that is not a row of the table."""
    row = table[base:base + D].astype(np.float64)
    out = []
    for r in weighted_ref.unit_r(q * f + np.arange(min(f, D), dtype=np.int64)).tolist():
        if not row[-1] > 0:
            out.append(-1)
            continue
        t, lo, n = r * row[-1], 0, D
        while n > 0:
            half = n >> 1
            if row[lo + half] <= t:
                lo, n = lo + half + 1, n - half - 1
            else:
                n = half
        out.append(min(lo, D - 1))
    return np.array(out, dtype=np.int32)


def _weighted_topo_stats(wl, weights, oc, p, want, fanout, stats, wrong_base_cap=4):
    """Of a weighted batch's last-hop frontier rows with D > f: how many partition p samples from a PEER's cached topology, from
    its own stripe and from the full CSR; and ("wrong_base", counted up to a cap) the peer-served ones whose start in the owner's
    cached array is not their start in the full CSR, whose weights are not all equal, and whose picks with the table read at the
    cached start are not the reference's -- a table base taken from the cached row shows in the batch."""
    f = fanout[-1]
    fr = np.asarray(mode_ref.hop_frontiers(want, len(fanout))[-1], dtype=np.int64)
    D = np.where(fr >= 0, np.diff(wl.indptr)[np.maximum(fr, 0)], 0)
    owner = _topo_owner(oc, fr)
    over = D > f
    stats["w_peer"] += int((over & (owner >= 0) & (owner != p)).sum())
    stats["w_local"] += int((over & (owner == p)).sum())
    stats["w_full"] += int((over & (owner < 0)).sum())
    ws = weighted_ref.sanitise(weights.w)
    for q in np.nonzero(over & (owner >= 0) & (owner != p))[0].tolist():
        if stats["wrong_base"] >= wrong_base_cap:
            break
        v, d = int(fr[q]), int(D[q])
        start, cached = int(wl.indptr[v]), _cached_start(oc, owner[q], v)
        if cached == start or np.ptp(ws[start:start + d]) == 0:
            continue
        right = weighted_ref.picks([q * f], [start], [d], f, weights.table)[0]
        assert np.array_equal(_picks_at_base(weights.table, start, d, q, f), right)          # (the restated search is the reference's)
        stats["wrong_base"] += int(not np.array_equal(_picks_at_base(weights.table, cached, d, q, f), right))


@functools.lru_cache(maxsize=None)
def _case_c(i, weighted=False):
    case_seed = (SEEDS_CW if weighted else SEEDS_C)[i]
    rng = np.random.RandomState(9000 + case_seed)
    hybrid = i % 3 == 2
    if hybrid:
        P, mode_bits = 1, 0
    else:
        P, mode_bits = [(2, 1), (4, 1), (4, 2)][(i // 3) % 3]
    c, wl, combo, weights, ctx = _workload(case_seed, max_hops=6 if hybrid else 4, P=P, min_dim=3)
    batch, fanout = c["batch"], c["fanout"]
    cpu = mode_ref.cpu_side(wl, batch, fanout, combo["storage"])
    presc, na, ea, max_ids, steps = _presc(wl, cpu, combo, batch, fanout, weights)
    case = dict(c=c, wl=wl, combo=combo, weights=weights, presc=presc, na=na, ea=ea, max_ids=max_ids, hybrid=hybrid, mode_bits=mode_bits)
    stats = {"peer": 0, "topo": 0, "cpu_tier": 0, "gpu_tier": 0, "w_peer": 0, "w_local": 0, "w_full": 0, "wrong_base": 0}
    if hybrid:
        cpu_cap = int(rng.choice([0, 5, wl.N // 7, wl.N // 2, 2 * wl.N]))
        gpu_cap = int(rng.choice([0, 3, wl.N // 5, wl.N // 2, 2 * wl.N]))
        oc = ffi.OracleCache(wl.N, wl.D, 1, 0)
        oc.hybrid_init(na[0], mode_ref.served_table(wl, combo["storage"]), cpu_cap, gpu_cap)
        case.update(caches=[oc], cpu_cap=cpu_cap, gpu_cap=gpu_cap)
        ctx += f", hybrid cpu {cpu_cap} gpu {gpu_cap}"
        served = [(0, mode, it) for mode in (0, 1, 2) for it in range(_n_batches(wl, 0, mode, batch))]
    else:
        capacity = (int(rng.randint(1, wl.N // P)), int(rng.randint(1, wl.N // P)))
        replica_rows = int(rng.randint(1, capacity[0] + 1)) if (i - i // 3) % 2 else 0            # every second striped seed
        case.update(caches=_oracle_caches(wl, combo, na, ea, mode_bits, capacity), capacity=capacity, replica_rows=replica_rows)
        ctx += f", cliques of {1 << mode_bits}, capacity {capacity}, replica {replica_rows}"
        served = [(p, mode, it) for p in range(P) for mode in (0, 1) for it in range(2)]
    wants = {}
    for p, mode, it in served:
        w = wants[(p, mode, it)] = mode_ref.expected_batch(wl, p, it, mode, batch, fanout, cpu=cpu, weights=weights, **combo)
        mode_ref.add_stats(stats, mode_ref.batch_stats(wl, w, fanout, weights=weights))
        oc = case["caches"][p >> mode_bits]
        owner = _topo_owner(oc, mode_ref.hop_frontiers(w, len(fanout))[-1])
        stats["topo"] += int((owner >= 0).sum())
        stats["peer"] += int(((owner >= 0) & (owner != p)).sum())          # rows sampled from a peer's cached topology
        if weights and not hybrid:
            _weighted_topo_stats(wl, weights, oc, p, w, fanout, stats)
        if hybrid:
            slot = oc.arr("node_map", np.int32)[w["sampled_ids"]]
            stats["cpu_tier"] += int(((slot >= 0) & (slot < cpu_cap)).sum())
            stats["gpu_tier"] += int((slot >= cpu_cap).sum())
    cpu.close()
    if weights:
        stats["differs"] = int(_differs_from_unit_weights(wl, combo, batch, fanout, ((p, m, it, w) for (p, m, it), w in wants.items())))
    case.update(ctx=ctx, wants=wants, stats=stats)
    return case


def _conditions_c(cases):
    """Dead columns were sampled; every striped case that records edge ids sampled rows from a PEER's cached topology (so the
    peer's column array was read and the id still is the full CSR's); the hybrid cases hit both tiers."""
    cases = list(cases)
    assert sum(case["stats"]["dead"] for case in cases) > 0
    striped = [case for case in cases if not case["hybrid"]]
    assert {case["wl"].P for case in striped} == {2, 4} and {case["mode_bits"] for case in striped} == {1, 2}
    assert any(case["replica_rows"] for case in striped) and not all(case["replica_rows"] for case in striped)
    for case in striped:
        assert not case["combo"]["edge_ids"] or case["stats"]["peer"] > 0, case["ctx"] + f": no peer-served row: {case['stats']}"
    hybrid = [case for case in cases if case["hybrid"]]
    assert sum(case["stats"]["cpu_tier"] for case in hybrid) > 0 and sum(case["stats"]["gpu_tier"] for case in hybrid) > 0
    assert any(len(case["c"]["fanout"]) > 4 for case in hybrid)             # five or six hops
    for flag in ("replace", "edge_ids"):                                    # both tiers of the file see both values of each mode
        for group in (striped, hybrid):
            assert {case["combo"][flag] for case in group} == {True, False}


def _conditions_c_weighted(cases):
    """The weighted cases of section c.  Every weighted combination has a case; the cliques (P, bits) (2, 1), (4, 1) and (4, 2) each
    run with and without a replica.  EVERY striped case samples, for last-hop frontier rows with D > f, from a peer's cached
    topology, from its own stripe and from the full CSR -- the two branches of the sampler's table base side by side -- and has a
    peer-served row on which a table base taken from the cached row gives other picks (_weighted_topo_stats), and batches that unit
    weights would make other ones.  At least two hybrid cases hit both tiers and one has five or six hops.  Over all of them:
    _conditions_weighted."""
    cases = list(cases)
    assert {mode_ref.combo_name(case["combo"]) for case in cases} == {mode_ref.combo_name(c) for c in mode_ref.COMBOS[16:]}
    striped = [case for case in cases if not case["hybrid"]]
    hybrid = [case for case in cases if case["hybrid"]]
    assert {(case["wl"].P, case["mode_bits"], bool(case["replica_rows"])) for case in striped} == \
        {(P, bits, r) for P, bits in ((2, 1), (4, 1), (4, 2)) for r in (False, True)}
    total = {}
    for case in cases:
        s = case["stats"]
        assert s["differs"], case["ctx"] + "): the batches are those of unit weights"
        if not case["hybrid"]:
            assert s["w_peer"] > 0 and s["w_local"] > 0 and s["w_full"] > 0 and s["wrong_base"] > 0, case["ctx"] + f"): {s}"
        mode_ref.add_stats(total, s)
    _conditions_weighted("section c", total)
    assert sum(case["stats"]["cpu_tier"] > 0 and case["stats"]["gpu_tier"] > 0 for case in hybrid) >= 2         # both tiers in one case
    assert any(len(case["c"]["fanout"]) > 4 for case in hybrid)             # five or six hops
    for group in (striped, hybrid):
        assert {case["combo"]["edge_ids"] for case in group} == {True, False}
    return total


@pytest.fixture(scope="module")
def cases_c():
    cases = {i: _case_c(i) for i in range(16)}
    _conditions_c(cases.values())
    return cases


@pytest.fixture(scope="module")
def cases_cw():
    cases = {i: _case_c(i, True) for i in range(len(SEEDS_CW))}
    _conditions_c_weighted(cases.values())
    return cases


def _run_c(case, col_slots):
    c, wl = case["c"], case["wl"]
    fanout, caches = c["fanout"], case["caches"]
    ctx = case["ctx"] + f", column slots {col_slots}): "
    gpu = _gpu_side(case, cache_memory=200_000)
    _run_presc_on_gpu(gpu, case, ctx)
    if case["hybrid"]:
        gpu.cache.hybrid_init(gpu.feature, gpu.graph, case["cpu_cap"], case["gpu_cap"])
        assert np.array_equal(gpu.cache.array("QF", 0).cpu().numpy(), caches[0].arr("QF", np.int32)), ctx + "QF"
        assert np.array_equal(gpu.cache.array("node_map", 0).cpu().numpy(), caches[0].arr("node_map", np.int32)), ctx + "node_map"
    else:
        Kg = 1 << case["mode_bits"]
        gpu.cache.candidate_selection(case["mode_bits"], gpu.graph)
        gpu.cache.set_capacity(*case["capacity"])
        if case["replica_rows"]:
            gpu.cache.set_replica_memory(case["replica_rows"] * gpu.feature.row_bytes)
        gpu.cache.fill_up(gpu.feature, gpu.graph)
        assert all(gpu.graph.column_slots(p) == col_slots for p in range(wl.P)), ctx
        for ki, oc in enumerate(caches):
            assert np.array_equal(gpu.cache.array("QF", ki * Kg).cpu().numpy(), oc.arr("QF", np.int32)), ctx + f"QF of clique {ki}"
            for p in range(ki * Kg, (ki + 1) * Kg):
                assert gpu.cache.replica_rows(p) == case["replica_rows"], ctx + f"replica rows of gpu {p}"
                for name, dt in (("node_map", np.int32), ("edge_index_map", np.int8), ("edge_offset_map", np.int32)):
                    assert np.array_equal(gpu.cache.array(name, p).cpu().numpy(), oc.arr(name, dt)), ctx + f"{name} of gpu {p}"
    for (p, mode, it), want in case["wants"].items():
        at = ctx + f"serve gpu {p} mode {mode} batch {it}: "
        mode_ref.compare_mode_batch(gpu.run(p, it, mode), want, wl, at)
        _check_topo_mask(gpu.pools[p], want, len(fanout), caches[p >> case["mode_bits"]], at)
    assert all(pool.error() == 0 for pool in gpu.pools), ctx
    gpu.close()


@pytest.mark.parametrize("seed", range(16))
def test_random_shapes_modes_striped_cliques_and_hybrid(hip, col_slots, cases_c, seed):
    _run_c(cases_c[seed], col_slots)


@pytest.mark.parametrize("seed", range(len(SEEDS_CW)))
def test_random_shapes_weighted_modes_striped_cliques_and_hybrid(hip, col_slots, cases_cw, seed):
    _run_c(cases_cw[seed], col_slots)
