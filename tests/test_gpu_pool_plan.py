"""Arena pipelines across the cases of a lane's memory plan (legion_amd/csrc/pool_plan.h).  A pipeline sizes its private block from
the plan and its pools allocate by walking it; creation itself checks that every lane took exactly the plan's sum from the block and
ends the process otherwise, so each pipeline created here is that check, and each serves a group that must equal the CPU oracle.
Pools get their arenas from an explicit source: pipelines may be created, used and closed in any order on one thread."""
import numpy as np
import pytest

from tests import edge_ids_ref
from tests.gpu_harness import CpuSide, GpuSide
from tests.helpers import Workload, compare_batches
from tests.mode_ref import bf16_bits

pytestmark = pytest.mark.gpu

GROUP, SLOTS = 2, 2
# one shape per bucket class: LG_LDS_SLOTS_SMALL slots (8 buckets), one batch entry past it (64), past LG_LDS_SLOTS_MEDIUM (256, run_off)
SHAPES = {"small": (64, [6, 3], 8, 11, 32), "2^19": (1024, [32, 16], 8, 12, 4), "2^19+": (1025, [32, 16], 64, 12, 4), "2^22+": (1025, [64, 64], 256, 12, 4)}
_sides = {}


def _side(shape):
    """Graph, feature table and oracle of a shape, with the oracle's batches of the first group: computed once, shared, left alone."""
    if shape not in _sides:
        batch, fanout, _, scale, dim = SHAPES[shape]
        wl = Workload(scale=scale, edge_factor=8, dim=dim, n_seeds=max(700, 2 * batch + 50))
        cpu = CpuSide(wl, batch, fanout)
        lanes = GROUP if shape == "small" else 1             # the larger classes: lane 0 only
        want = [cpu.run(0, b, 0) for b in range(lanes)]
        cpu.close()
        _sides[shape] = (wl, want)
    return _sides[shape]


def _serve_and_compare(pipe, want, ctx, first=0, bf16=False):
    from legion_amd import engine
    sl = pipe.submit(first, 0)
    pipe.wait(sl)
    for lane, w in enumerate(want):
        got = engine.read_batch(pipe.pools[sl][lane])
        if bf16:
            w = dict(w)
            rows = got.pop("float_features")
            assert np.array_equal(rows, bf16_bits(w.pop("float_features"))), f"{ctx}lane {lane}: bf16 rows"
        compare_batches(got, w, f"{ctx}lane {lane}: ")
    assert all(pool.error() == 0 for pool in pipe.pools[sl])


@pytest.mark.parametrize("chunk_mb", [None, "0"], ids=["scattered", "plain"])
@pytest.mark.parametrize("shape,col_slots,out_dtype", [("small", "1", "float32"), ("small", "0", "float32"), ("small", "1", "bfloat16"),
                                                       ("2^19", "1", "float32"), ("2^19+", "1", "float32"), ("2^22+", "1", "float32")])
def test_arena_pipelines_across_the_plan(hip, monkeypatch, chunk_mb, shape, col_slots, out_dtype):
    """Every bucket class, column slots on and off, bf16 rows; shuffled chunks (the private block exists: creation checks each lane
    against its plan) and LEGION_ARENA_SCATTER_MB=0 (no block: every array a plain allocation, freed one by one).  Created and closed
    twice: the second pipeline re-uses what the first released."""
    from legion_amd import engine
    if chunk_mb is not None:
        monkeypatch.setenv("LEGION_ARENA_SCATTER_MB", chunk_mb)
    monkeypatch.setenv("LEGION_COL_SLOTS", col_slots)
    batch, fanout, n_buckets, _, _ = SHAPES[shape]
    wl, want = _side(shape)
    gpu = GpuSide(wl, batch, fanout)
    for rep in range(2):
        pipe = engine.Pipeline(gpu.graph, gpu.feature, gpu.cache, 0, batch, fanout, GROUP, gpu.pools[0].num_ids, True, SLOTS, weave=True, arena=True,
                               feature_out_dtype=out_dtype)
        assert pipe.pools[0][0].lds_buckets() == n_buckets
        _serve_and_compare(pipe, want, f"{shape} col_slots {col_slots} {out_dtype} ({chunk_mb}) rep {rep} ", bf16=out_dtype == "bfloat16")
        pipe.close()
    gpu.close()


def test_a_lane_with_edge_ids_inside_an_arena_pipeline(hip):
    """The edge-id arrays stay outside the plan: plain allocations of the pool, made when the mode is turned on.  close() frees those
    two and none of the lane's carved arrays."""
    from legion_amd import engine
    batch, fanout = SHAPES["small"][:2]
    wl, _ = _side("small")
    gpu = GpuSide(wl, batch, fanout)
    pipe = engine.Pipeline(gpu.graph, gpu.feature, gpu.cache, 0, batch, fanout, GROUP, gpu.pools[0].num_ids, True, SLOTS, weave=True, arena=True)
    pipe.set_edge_ids(True)
    sl = pipe.submit(0, 0)
    pipe.wait(sl)
    ids, labels = wl.sets[(0, 0)]
    for lane in range(GROUP):
        got = engine.read_batch(pipe.pools[sl][lane])
        want = edge_ids_ref.run_batch(wl.indptr, wl.col, ids, labels, batch, lane, fanout, True)
        compare_batches(got, want, f"edge ids lane {lane}: ")
        assert np.array_equal(got["agg_edge_ids"], want["agg_edge_ids"]), f"lane {lane}: agg_edge_ids"
        edge_ids_ref.check_edge_ids(wl.indptr, wl.col, got)
    pipe.close()
    gpu.close()


def test_interleaved_pipelines_on_one_thread(hip):
    """A created, B created, A submits, B submits, A closed, B submits again: each pipeline's pools know their own arena and block."""
    from legion_amd import engine
    batch, fanout = SHAPES["small"][:2]
    wl, want = _side("small")
    gpu = GpuSide(wl, batch, fanout)

    def make():
        return engine.Pipeline(gpu.graph, gpu.feature, gpu.cache, 0, batch, fanout, GROUP, gpu.pools[0].num_ids, True, SLOTS, weave=True, arena=True)
    a = make()
    b = make()
    _serve_and_compare(a, want, "A ")
    _serve_and_compare(b, want, "B ")
    a.close()
    _serve_and_compare(b, want, "B after A closed ")
    b.close()
    gpu.close()
