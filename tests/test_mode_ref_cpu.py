"""The three CPU references that tests/mode_ref.py stitches together agree with one another on the fuzz shapes: the oracle (with
replacement), tests/distinct_ref.py (without) and tests/edge_ids_ref.py (both, plus the edge ids) -- every mode, every batch
including the empty one past the end, half of the shapes with dead column entries."""
import numpy as np
import pytest

from tests import distinct_ref, edge_ids_ref, mode_ref
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
