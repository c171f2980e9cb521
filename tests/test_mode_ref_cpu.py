"""The three CPU references that tests/mode_ref.py stitches together agree with one another on the fuzz shapes: the oracle (with
replacement), tests/distinct_ref.py (without) and tests/edge_ids_ref.py (both, plus the edge ids) -- every mode, every batch
including the empty one past the end, half of the shapes with dead column entries."""
import itertools

import numpy as np
import pytest

from tests import distinct_ref, edge_ids_ref, mode_ref
from tests import test_gpu_fuzz_modes as fuzz
from tests.helpers import KEYS_EXACT, Workload
from tests.test_gpu_fuzz import random_case


@pytest.mark.parametrize("seed", range(16))
def test_references_agree_on_the_fuzz_shapes(seed):
    c = random_case(seed)
    col = mode_ref.with_dead_columns(c["col"], seed) if seed % 2 else c["col"]
    wl = Workload(dim=c["dim"], n_seeds=c["n_seeds"], n_valid=c["n_valid"], n_test=c["n_test"], indptr=c["indptr"], col=col)
    batch, fanout = c["batch"], c["fanout"]
    cpu = mode_ref.cpu_side(wl, batch, fanout)
    ctx = f"seed {seed} (N {wl.N}, E {wl.E}, fan-out {fanout}, batch {batch}, dead {int((col < 0).sum())}): "
    total = {}
    for mode in (0, 1, 2):
        ids, labels = wl.sets[(0, mode)]
        steps = (ids.size + batch - 1) // batch + 1                  # one past the end: the empty batch
        for it in range(steps):
            at = ctx + f"mode {mode} batch {it}: "
            oracle = cpu.run(0, it, mode)
            with_r = edge_ids_ref.run_batch(wl.indptr, wl.col, ids, labels, batch, it, fanout, True)
            without = edge_ids_ref.run_batch(wl.indptr, wl.col, ids, labels, batch, it, fanout, False)
            distinct = distinct_ref.run_batch(wl.indptr, wl.col, ids, labels, batch, it, fanout)
            for k in KEYS_EXACT:
                assert np.array_equal(with_r[k], oracle[k]), at + f"edge_ids_ref (replace) != oracle on {k}"
                assert np.array_equal(without[k], distinct[k]), at + f"edge_ids_ref (distinct) != distinct_ref on {k}"
            edge_ids_ref.check_edge_ids(wl.indptr, wl.col, with_r)
            edge_ids_ref.check_edge_ids(wl.indptr, wl.col, without)
            # what mode_ref composes from them, and the statistics it takes from a reference batch
            for replace, ref in ((True, with_r), (False, without)):
                want = mode_ref.expected_batch(wl, 0, it, mode, batch, fanout, replace=replace, edge_ids=True, storage="float32",
                                               out="float32", cpu=cpu)
                assert np.array_equal(want["agg_edge_ids"], ref["agg_edge_ids"]), at
                if wl.D > 0:
                    assert np.array_equal(want["rows"], wl.features[ref["sampled_ids"]].view(np.uint32)), at
                s = mode_ref.batch_stats(wl, want, fanout)
                assert s["dead"] >= 0 and (s["dead"] == 0 or seed % 2 == 1), at + str(s)
                assert s["empty"] == (it == steps - 1), at + str(s)
                mode_ref.add_stats(total, s)
    assert total["empty"] == 6, ctx + str(total)
    if seed % 2 and (col < 0).sum() >= 20:
        assert total["dead"] > 0, ctx + str(total)                   # (5 % of the entries of a graph sampled this often)
    cpu.close()


def test_presc_batch_of_the_composed_reference():
    """A PreSC batch (no gathers) of either sampling mode still carries the served batch's edge ids, and its hotness counts are
    the reference's."""
    c = random_case(3)
    wl = Workload(dim=c["dim"], n_seeds=c["n_seeds"], n_valid=c["n_valid"], n_test=c["n_test"], indptr=c["indptr"], col=c["col"])
    batch, fanout = c["batch"], c["fanout"]
    for replace in (True, False):
        cpu = mode_ref.cpu_side(wl, batch, fanout)
        ea, na = np.zeros(wl.N, np.uint64), np.zeros(wl.N, np.uint64)
        want = mode_ref.expected_batch(wl, 0, 0, 0, batch, fanout, replace=replace, edge_ids=True, storage="float32", out="float32",
                                       serve=False, edge_access=ea, node_access=na, cpu=cpu)
        assert "rows" not in want and want["agg_edge_ids"].shape == want["agg_src_ids"].shape
        assert int(ea.sum()) == want["agg_src_ids"].size                       # one count per sampled edge ...
        assert int(na.sum()) == want["sampled_ids"].size                       # ... and per distinct vertex
        if replace:
            assert cpu.node_access[0] is na and cpu.max_ids[0] == int(want["node_counter"][7])
        cpu.close()


# ---- the weighted combinations (COMBOS[16:]) and the fuzz's weighted seed lists --------------------------------------------------
def test_combos_are_pinned():
    """Case seeds map to combinations by index: the first sixteen are replace x edge_ids x storage x out as ever, the weighted
    eight follow."""
    kinds = ("float32", "bfloat16")
    assert len(mode_ref.COMBOS) == 24
    old = [dict(replace=r, edge_ids=e, storage=s, out=o) for r, e, s, o in itertools.product((True, False), (False, True), kinds, kinds)]
    assert [{k: v for k, v in c.items() if k != "draw"} for c in mode_ref.COMBOS[:16]] == old
    assert [c["draw"] for c in mode_ref.COMBOS[:16]] == ["replace"] * 8 + ["distinct"] * 8
    assert mode_ref.COMBOS[16:] == [dict(replace=True, edge_ids=e, storage=s, out=o, draw="weighted")
                                    for e, s, o in itertools.product((False, True), kinds, kinds)]
    assert len({mode_ref.combo_name(c) for c in mode_ref.COMBOS}) == 24
    assert [mode_ref.combo_name(c) for c in mode_ref.COMBOS[::8]] == ["replace storage float32 out float32", "distinct storage float32 out float32",
                                                                      "weighted storage float32 out float32"]
    assert [fuzz._combo(s) for s in (0, 63, 64, 1023)] == [mode_ref.COMBOS[i] for i in (0, 15, 0, 15)]
    assert [fuzz._combo(s) for s in (1024, 1055, 1056)] == [mode_ref.COMBOS[i] for i in (16, 23, 16)]


def test_case_weights():
    """A case's weights: multiples of 1/8 and the sanitised specials, rows of positive degree whose total is 0, a table that is
    exact (so unique), and the statistics batch_stats takes from them."""
    c = random_case(1027)
    w, table = mode_ref.case_weights(c["indptr"], 1027)
    assert w.dtype == np.float32 and w.shape == c["col"].shape and table.dtype == np.float32
    finite = np.isfinite(w)
    assert np.all(w[finite] * 8 == np.round(w[finite] * 8)) and w[finite].max() <= 4
    assert np.isnan(w).any() and np.isposinf(w).any() and (w == -1).any() and np.signbit(w[w == 0]).any()
    assert 0.02 < np.isin(w.view(np.uint32), mode_ref.SPECIAL_WEIGHTS[1:].view(np.uint32)).mean() < 0.08
    ws = mode_ref.weighted_ref.sanitise(w).astype(np.float64)
    exact = np.concatenate([[0], np.cumsum(ws)])
    deg, positive = np.diff(c["indptr"]), mode_ref.row_weight_counts(c["indptr"], w)
    assert ((deg > 0) & (positive == 0)).sum() >= 3 and ((positive > 0) & (positive < deg)).any() and np.all(positive <= deg)
    for v in np.nonzero(deg)[0]:
        s, e = int(c["indptr"][v]), int(c["indptr"][v + 1])
        assert np.array_equal(table[s:e].astype(np.float64), exact[s + 1:e + 1] - exact[s])           # no rounding anywhere
        assert positive[v] == int((ws[s:e] > 0).sum())
    again = mode_ref.case_weights(c["indptr"], 1027)
    assert np.array_equal(again.w.view(np.uint32), w.view(np.uint32)) and not np.array_equal(mode_ref.case_weights(c["indptr"], 1028).w, w)


def test_weighted_seed_lists_meet_their_conditions():
    """Every weighted case of the GPU fuzz is built and its list's conditions hold: a vacuous seed list fails without a GPU."""
    assert len(fuzz.SEEDS_AW) == 32 and {(s % 4, (s // 4) % 8) for s in fuzz.SEEDS_AW} == set(itertools.product(range(4), range(8)))
    assert len(fuzz.SEEDS_BW) == 8 and len(fuzz.SEEDS_CW) == 16
    assert min(fuzz.SEEDS_AW + fuzz.SEEDS_BW + fuzz.SEEDS_CW) >= fuzz.WEIGHTED_SEEDS > max(fuzz.SEEDS_A + fuzz.SEEDS_B + fuzz.SEEDS_C)
    assert len(set(fuzz.SEEDS_AW)) == 32 and len(set(fuzz.SEEDS_BW)) == 8 and len(set(fuzz.SEEDS_CW)) == 16
    fuzz._conditions_a([fuzz._case_a(s) for s in fuzz.SEEDS_AW], 8)
    fuzz._conditions_b_weighted(fuzz._case_b(i, True) for i in range(8))
    fuzz._conditions_c_weighted(fuzz._case_c(i, True) for i in range(16))


def _weighted_case(section, i):
    """(case, its batches as (partition, batch, seed-set mode, served))."""
    if section == "a":
        case = fuzz._case_a(fuzz.SEEDS_AW[i])
        return case, [(0, it, mode, True) for mode, it in case["wants"]]
    case = fuzz._case_b(i, True) if section == "b" else fuzz._case_c(i, True)
    served = [(0, it, mode, True) for mode, it in case["wants"]] if section == "b" else [(p, it, mode, True) for p, mode, it in case["wants"]]
    return case, [(p, it, 0, False) for p, it in case["presc"]] + served


@pytest.mark.parametrize("section,i", [("a", i) for i in range(32)] + [("b", i) for i in range(8)] + [("c", i) for i in range(16)])
def test_weighted_reference_under_unit_weights_is_the_oracle(section, i):
    """The composition of the weighted branch against the one reference the project does not own the text of: every batch of every
    weighted fuzz case -- PreSC and served, on every partition -- composed under UNIT weights is the replace=True oracle batch of
    the same case bit for bit: ids, labels, counters, COO, the edge ids (through edge_ids_ref), and PreSC's hotness counts."""
    case, batches = _weighted_case(section, i)
    wl, batch, fanout = case["wl"], case["c"]["batch"], case["c"]["fanout"]
    assert batches and case["combo"]["draw"] == "weighted" and case["weights"] is not None
    unit = mode_ref.unit_weights(wl.indptr)
    cpu = mode_ref.cpu_side(wl, batch, fanout)
    modes = dict(edge_ids=True, storage="float32", out="float32")
    hot = {draw: [[np.zeros(wl.N, np.uint64) for _ in range(wl.P)] for _ in range(2)] for draw in ("weighted", "replace")}
    for p, it, mode, serve in batches:
        at = case["ctx"] + f"): gpu {p} mode {mode} batch {it} served {serve}: "
        got = {}
        for draw in ("weighted", "replace"):
            ea, na = (None, None) if serve else (hot[draw][0][p], hot[draw][1][p])
            got[draw] = mode_ref.expected_batch(wl, p, it, mode, batch, fanout, replace=True, draw=draw, weights=unit, serve=serve,
                                                edge_access=ea, node_access=na, cpu=cpu, **modes)
        for k in KEYS_EXACT + ["agg_edge_ids"] + (["rows"] if serve and wl.D > 0 else []):
            assert got["weighted"][k].dtype == got["replace"][k].dtype, at + k
            assert np.array_equal(got["weighted"][k], got["replace"][k]), at + k
        assert ("rows" in got["weighted"]) == ("rows" in got["replace"]) == (serve and wl.D > 0), at
    for which in (0, 1):
        for p in range(wl.P):
            assert np.array_equal(hot["weighted"][which][p], hot["replace"][which][p]), case["ctx"] + f"): hotness {which} of gpu {p}"
    cpu.close()
