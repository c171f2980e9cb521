"""What the GPU must produce for one batch under any combination of the opt-in modes (the draw: with replacement, without, or
weighted; edge ids; bfloat16 feature storage; bfloat16 rows to the trainer), composed from the references the suite already has:

  ids, labels, counters, COO (helpers.KEYS_EXACT)   replace=True: the oracle (gpu_harness.CpuSide); replace=False: distinct_ref;
                                                    weighted: weighted_ref (which tests/test_mode_ref_cpu.py holds equal to the
                                                    oracle under unit weights)
  agg_edge_ids                                      edge_ids_ref (which tests/test_mode_ref_cpu.py holds equal to the first two);
                                                    weighted: weighted_ref's own
  rows                                              table[sampled_ids], the table being the float32 features or, for a bf16 storage,
                                                    torch's CPU rounding of them; for bf16 rows out the same rounding once more (a
                                                    no-op on a rounded table)

Every path is a copy or one round to nearest even, so everything is compared as bit patterns.  A helper of the tests, not a test
file."""
import collections
import copy
import itertools

import numpy as np
import torch

from tests import distinct_ref, edge_ids_ref, weighted_ref
from tests.gpu_harness import CpuSide
from tests.helpers import compare_batches

# replace x edge_ids x storage x out, indexed 0..15; then the weighted draw (with replacement: the library refuses weighted and
# distinct together) x edge_ids x storage x out, indexed 16..23.  "draw" names the draw: replace / distinct / weighted
COMBOS = [dict(replace=r, edge_ids=e, storage=s, out=o, draw="replace" if r else "distinct")
          for r, e, s, o in itertools.product((True, False), (False, True), ("float32", "bfloat16"), ("float32", "bfloat16"))]
COMBOS += [dict(replace=True, edge_ids=e, storage=s, out=o, draw="weighted")
           for e, s, o in itertools.product((False, True), ("float32", "bfloat16"), ("float32", "bfloat16"))]


def combo_name(c):
    return f"{c['draw']}{'+eids' if c['edge_ids'] else ''} storage {c['storage']} out {c['out']}"


# a case's per-edge weights and the prefix-sum table the graph builds from them
EdgeWeights = collections.namedtuple("EdgeWeights", "w table")
SPECIAL_WEIGHTS = np.array([0.0, -1.0, np.nan, np.inf, -0.0], dtype=np.float32)        # each counts as 0


def case_weights(indptr, seed):
    """The weights of the case `seed` over the CSR indptr: multiples of 1/8 (weighted_ref.hash_weights: a fifth of them zero), so
    every prefix sum is exact and the table is weighted_ref.cdf's bit for bit; about 5 % of the entries one of the values that
    are sanitised to 0; and every weight of a few rows of positive degree 0 (such a row yields no edge)."""
    indptr = np.asarray(indptr, dtype=np.int64)
    E = int(indptr[-1])
    rng = np.random.RandomState(6000 + seed)
    w = weighted_ref.hash_weights(E, seed=seed)
    odd = rng.rand(E) < 0.05
    w[odd] = rng.choice(SPECIAL_WEIGHTS, int(odd.sum()))
    rows = np.nonzero(np.diff(indptr) > 0)[0]
    for v in rng.choice(rows, min(3 + rows.size // 64, rows.size), replace=False):
        w[indptr[v]:indptr[v + 1]] = 0
    return EdgeWeights(w, weighted_ref.cdf(indptr, w))


def unit_weights(indptr):
    """Weight 1 on every edge: the weighted draw is then the uniform one."""
    w = np.ones(int(indptr[-1]), np.float32)
    return EdgeWeights(w, weighted_ref.cdf(indptr, w))


def rounded(f):
    """The float32 table as a bf16 storage serves it: torch's rounding, widened back (exact)."""
    return torch.from_numpy(np.ascontiguousarray(f)).to(torch.bfloat16).float().numpy()


def bf16_bits(rows):
    """torch's bf16 of float32 rows, as uint16 bits."""
    return torch.from_numpy(np.ascontiguousarray(rows)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def served_table(wl, storage):
    """float32[N, D]: the rows a storage of this dtype serves."""
    return rounded(wl.features) if storage == "bfloat16" else wl.features


def cpu_side(wl, batch, fanout, storage="float32"):
    """The oracle over the table the storage serves (its ids and counters do not depend on the table)."""
    wl_c = copy.copy(wl)
    wl_c.features = served_table(wl, storage)
    return CpuSide(wl_c, batch, fanout)


def expected_rows(wl, sampled_ids, storage, out):
    """Bit patterns [n, D] of the rows of sampled_ids: uint32 for float32 rows, uint16 for bf16 rows."""
    ids = np.asarray(sampled_ids, dtype=np.int64)
    assert np.all(ids >= 0)                  # (dead column entries are dropped, and a batch never reads past its seed set)
    rows = np.ascontiguousarray(served_table(wl, storage)[ids])
    return bf16_bits(rows) if out == "bfloat16" else rows.view(np.uint32)


def expected_batch(wl, dev, it, mode, batch, fanout, *, replace, edge_ids, storage, out, draw=None, weights=None, serve=True,
                   edge_access=None, node_access=None, cpu=None):
    """The batch `it` of partition dev's seed set `mode`: KEYS_EXACT, "agg_edge_ids" (int64) if edge_ids, and -- for a served batch
    -- "rows".  serve=False is a PreSC batch (no gathers); edge_access / node_access: uint64[N] hotness counts of the partition,
    added to in place.  draw: COMBOS' (None: by replace); weights: the EdgeWeights of a weighted draw.  cpu: the CpuSide the oracle
    runs through when replace=True (a throw-away one otherwise; the weighted draw does not use it)."""
    ids, labels = wl.sets[(dev, mode)]
    weighted = draw == "weighted"
    assert draw in (None, "weighted", "replace" if replace else "distinct") and (replace or not weighted)
    if weighted:
        want = weighted_ref.run_batch(wl.indptr, wl.col, weights.table, ids, labels, batch, it, fanout, serve, edge_access, node_access)
        weighted_ref.check_edges(wl.indptr, wl.col, weights.w, want)
        if not edge_ids:
            del want["agg_edge_ids"]
    elif replace:
        side = cpu if cpu is not None else cpu_side(wl, batch, fanout, storage)
        if node_access is not None:
            side.node_access[dev] = node_access
        if edge_access is not None:
            side.edge_access[dev] = edge_access
        want = side.run(dev, it, mode, is_presc=not serve)
        want.pop("float_features", None)
        want.pop("cache_search_buffer", None)
        if cpu is None:
            side.close()
    else:
        want = distinct_ref.run_batch(wl.indptr, wl.col, ids, labels, batch, it, fanout, serve, edge_access, node_access)
    if edge_ids and not weighted:
        e = edge_ids_ref.run_batch(wl.indptr, wl.col, ids, labels, batch, it, fanout, replace)
        for k in ("sampled_ids", "agg_src_ids", "agg_dst_ids"):      # the same edges, so the ids line up (counters differ in PreSC)
            assert np.array_equal(e[k], want[k]), f"the references disagree on {k}"
        edge_ids_ref.check_edge_ids(wl.indptr, wl.col, e)
        want["agg_edge_ids"] = e["agg_edge_ids"]
    if serve and wl.D > 0:
        want["rows"] = expected_rows(wl, want["sampled_ids"], storage, out)
    return want


def compare_mode_batch(got, want, wl, ctx):
    """got: engine.read_batch / GpuSide.run of a pool in the modes `want` was made for."""
    got = dict(got)
    rows = got.pop("float_features", None)
    compare_batches(got, want, ctx)
    assert ("agg_edge_ids" in got) == ("agg_edge_ids" in want), f"{ctx}agg_edge_ids present: {'agg_edge_ids' in got}"
    if "agg_edge_ids" in want:
        g, w = got["agg_edge_ids"], want["agg_edge_ids"]
        assert g.dtype == np.int64 and g.shape == w.shape, f"{ctx}agg_edge_ids: {g.dtype} {g.shape} != int64 {w.shape}"
        if not np.array_equal(g, w):
            bad = np.nonzero(g != w)[0]
            raise AssertionError(f"{ctx}agg_edge_ids: {bad.size} mismatches, first at {bad[0]}: got {g[bad[0]]} want {w[bad[0]]}")
        edge_ids_ref.check_edge_ids(wl.indptr, wl.col, got)
    if "rows" in want:
        w = want["rows"]
        assert rows is not None, f"{ctx}no rows"
        assert rows.dtype == (np.uint16 if w.dtype == np.uint16 else np.float32), f"{ctx}rows are {rows.dtype}"
        g = rows if rows.dtype == np.uint16 else rows.view(np.uint32)
        assert g.shape == w.shape, f"{ctx}rows shape {g.shape} != {w.shape}"
        if not np.array_equal(g, w):
            bad = np.nonzero((g != w).any(axis=1))[0]
            raise AssertionError(f"{ctx}{bad.size} rows differ, first {bad[:5]} (ids {want['sampled_ids'][bad[:5]]}): "
                                 f"got {g[bad[0]][:8]} want {w[bad[0]][:8]}")


def hop_frontiers(want, hops):
    """The frontier of every hop of a reference batch: the seeds, then each hop's sampled neighbours."""
    nc, ec = want["node_counter"], want["edge_counter"]
    out = [want["sampled_ids"][:max(int(nc[9]), 0)]]
    for h in range(1, hops):
        out.append(want["agg_src_ids"][int(ec[9 + h - 1]):int(ec[9 + h])])
    return out


def _carried_picks_matter(q, f, D, super_tile):
    """Entry q (D > f, slots across a super-tile boundary) without replacement: does a slot of the later super tile draw a position
    that one of the EARLIER tile's slots took?  Only then do the picks depend on the prefix the sampler carries over."""
    k = np.arange(f, dtype=np.int64)
    t = distinct_ref.draw(q * f + k, D - f + k + 1).tolist()
    first = int(super_tile - (q * f) % super_tile)                 # the first slot of the later super tile
    picks = []
    for kk in range(f):
        picks.append(t[kk] if t[kk] not in picks else int(D - f + kk))
    return any(t[kk] in picks[:first] for kk in range(first, f))


def row_weight_counts(indptr, w):
    """int64[N]: per row, how many of its entries have a (sanitised) weight > 0."""
    below = np.concatenate([[0], np.cumsum(weighted_ref.sanitise(w) > 0)]).astype(np.int64)
    indptr = np.asarray(indptr, dtype=np.int64)
    return below[indptr[1:]] - below[indptr[:-1]]


def batch_stats(wl, want, fanout, super_tile=1024, distinct=False, weights=None):
    """What a reference batch exercised, for the conditions that keep a fuzz from passing vacuously -- from the reference alone:
    frontier entries with D > f and with D = 0, entries with D > f whose f slots q*f .. q*f + f - 1 straddle a multiple of the
    sampler's super tile, (distinct=True: and, of these, the entries whose later picks depend on the earlier super tile's: "carry"), sampled
    dead column entries (slots that drew col < 0: every slot k < min(f, D) gives an edge otherwise), and whether the batch is the
    empty one.  weights (the EdgeWeights of a weighted batch): also the frontier entries with D > 0 whose row total is 0
    ("zero_total": none of their slots draws) and the frontier rows that hold a zero-weight entry beside positive ones ("mixed")."""
    ec = want["edge_counter"]
    deg = np.diff(wl.indptr)
    s = dict(over=0, zero=0, straddle=0, carry=0, dead=0, empty=int(want["sampled_ids"].size == 0 and int(want["node_counter"][9]) <= 0))
    positive = None
    if weights is not None:
        positive = row_weight_counts(wl.indptr, weights.w)
        s.update(zero_total=0, mixed=0)
    for h, (f, fr) in enumerate(zip(fanout, hop_frontiers(want, len(fanout)))):
        fr = np.asarray(fr, dtype=np.int64)
        D = np.where(fr >= 0, deg[np.maximum(fr, 0)], 0)
        if positive is not None:
            n_pos = np.where(fr >= 0, positive[np.maximum(fr, 0)], 0)
            s["zero_total"] += int(((D > 0) & (n_pos == 0)).sum())
            s["mixed"] += int(((n_pos > 0) & (n_pos < D)).sum())
        q = np.arange(fr.size, dtype=np.int64)
        s["over"] += int((D > f).sum())
        s["zero"] += int((D == 0).sum())
        across = (D > f) & ((q * f) // super_tile != (q * f + f - 1) // super_tile)
        s["straddle"] += int(across.sum())
        if distinct:
            s["carry"] += sum(_carried_picks_matter(int(i), f, int(D[i]), super_tile) for i in np.nonzero(across)[0])
        drawing = D if positive is None else np.where(n_pos > 0, D, 0)                # (a row whose total is 0 draws nothing)
        s["dead"] += int(np.minimum(drawing, f).sum()) - (int(ec[9 + h + 1]) - int(ec[9 + h]))
    return s


def add_stats(total, s):
    for k, v in s.items():
        total[k] = total.get(k, 0) + v
    return total


def with_dead_columns(col, seed, share=0.05):
    """A copy of the column array with `share` of its entries set to -1 (dead: no edge, no id)."""
    col = col.copy()
    if col.size:
        col[np.random.RandomState(5000 + seed).rand(col.size) < share] = -1
    return col
