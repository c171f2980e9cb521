#!/usr/bin/env python3
"""The rates of the link-prediction seed ops (GraphStorage.find_edges, negative_sample, engine.unique_ids, edge_prediction_seeds) on the
bench.py graph, each beside its composition from torch's library kernels on the same GPU and inputs, in a fresh process.

    python tools/link_rate.py [--scale 26] [--edge-factor 16] [--eids 1048576] [--k 5] [--launches 7] [--arms a,b,..] [--out FILE]

Graph, event timing and medians are those of tools/node2vec_rate.py (RMAT, seed 20231; rows sorted here if they are not; --launches
timed launches after one untimed, the median counts).  Arms:
  find_edges       2^20 edge ids, uniform over [0, E)        | torch.searchsorted(indptr, eids, right=True) - 1 and col[eids]
  negative(0)      k negatives per row, no exclusion         | torch.randint(0, N, (n, k))
  negative(1..3)   the exclusions (no torch counterpart: the time beside negative(0)'s)
  unique_ids       the first 2^20 ids a batch concatenates   | torch.unique(return_inverse=True)  (sorted, not first-appearance)
  seeds            edge_prediction_seeds of 2^20 // (2 + k) seed edges: the three ops chained, concatenation and scratch included
Every hand-written result is checked against the torch composition where the two compute the same thing (find_edges: equal; unique_ids:
the same set, the same count, local indices that give the ids back).  The arms named .../abi time the C ABI call alone over buffers
allocated once: the Python method's allocations and checks sit between the two events otherwise, which at these sizes is a tenth of
the time.  LEGION_HIP_LIB=<another build> times that build (how the find_edges variants of DESIGN.md 4.14 were
timed: --arms find_edges).  bench.py is not involved and is not changed."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(call, launches):
    import torch
    out = call()                                         # untimed: first touch of everything
    torch.cuda.synchronize()
    ms = []
    for _ in range(launches):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = call()
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1))
    return out, {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "ms": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=26)
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--eids", type=int, default=1 << 20)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--launches", type=int, default=7)
    ap.add_argument("--arms", type=str, default="find_edges,negative,unique_ids,seeds")
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    arms = set(args.arms.split(","))
    sys.path.insert(0, ROOT)
    import torch
    from legion_amd import engine, lib, synth
    from tools.node2vec_rate import sort_rows

    dev = "cuda:0"
    indptr, col = synth.rmat_csr_device(args.scale, args.edge_factor, 20231, dev)
    N, E = indptr.numel() - 1, col.numel()
    graph = engine.GraphStorage(1, indptr, col)
    was_sorted = graph.rows_sorted()
    print(f"the bench graph's rows are {'sorted' if was_sorted else 'NOT sorted: sorting them here, before anything is timed'}", flush=True)
    if not was_sorted:
        graph.close()
        col = sort_rows(indptr, col)
        torch.cuda.synchronize()
        graph = engine.GraphStorage(1, indptr, col)
        assert graph.rows_sorted(), "rows unsorted after the sort"
    n, k = args.eids, args.k
    gen = torch.Generator(device=dev)
    gen.manual_seed(20231)
    eids = torch.randint(0, E, (n,), dtype=torch.int64, device=dev, generator=gen)
    report = {"command": " ".join(["python", "tools/link_rate.py"] + sys.argv[1:]), "device": torch.cuda.get_device_name(0),
              "library": os.path.relpath(lib.LIB_PATH, ROOT), "graph": f"RMAT-{args.scale}, N={N}, E={E}", "rows_were_sorted": bool(was_sorted), "eids": n, "k": k,
              "launches": args.launches, "arms": {}}

    L = lib.load()
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    S = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def record(name, ours, theirs, items, unit, **more):
        arm = dict(ours=ours, per_second=items / ours["ms_median"] * 1e3, **more)
        line = f"{name:18s} {ours['ms_median']:8.3f} ms  {items / ours['ms_median'] * 1e-6:9.3f} G {unit}/s"
        if theirs is not None:
            arm["torch"] = theirs
            arm["ours_over_torch"] = ours["ms_median"] / theirs["ms_median"]
            line += f"   torch {theirs['ms_median']:8.3f} ms   ours / torch {arm['ours_over_torch']:.3f}"
        report["arms"][name] = arm
        print(line, flush=True)

    row, c = graph.find_edges(eids)
    if "find_edges" in arms:
        (row, c), ours = timed(lambda: graph.find_edges(eids), args.launches)
        (t_row, t_col), theirs = timed(lambda: (torch.searchsorted(indptr, eids, right=True) - 1, col[eids]), args.launches)
        same = bool(torch.equal(row.long(), torch.where(t_col >= 0, t_row, -1)) and torch.equal(c, torch.where(t_col >= 0, t_col, -1)))
        record("find_edges", ours, theirs, n, "edges", matches_torch=same)
        _, abi = timed(lambda: L.legion_find_edges(S(), graph.handle, P(eids), n, P(row), P(c)), args.launches)
        record("find_edges/abi", abi, theirs, n, "edges")
        assert same, "find_edges differs from searchsorted"
        del t_row, t_col
    neg = graph.negative_sample(row, k, exclude_self=False, exclude_edges=False)
    if "negative" in arms:
        _, theirs = timed(lambda: torch.randint(0, N, (n, k), dtype=torch.int32, device=dev), args.launches)
        for exclude in range(4):
            kw = dict(exclude_self=bool(exclude & 1), exclude_edges=bool(exclude & 2))
            out, ours = timed(lambda: graph.negative_sample(row, k, **kw), args.launches)
            record(f"negative({exclude})", ours, theirs if exclude == 0 else None, n * k, "negatives",
                   unfilled_slots=int((out < 0).sum().item()))
        neg = out
        for exclude in (0, 3):
            _, abi = timed(lambda: L.legion_negative_sample(S(), graph.handle, P(row), n, k, exclude, 256, 0, P(neg)), args.launches)
            record(f"negative({exclude})/abi", abi, theirs if exclude == 0 else None, n * k, "negatives")
    m = min(n, engine.UNIQUE_MAX_IDS)
    B = m // (2 + k)
    ids = torch.cat([row[:B], c[:B], neg[:B].reshape(-1)]).contiguous()
    if "unique_ids" in arms:
        (unique, local, count), ours = timed(lambda: engine.unique_ids(ids), args.launches)
        (t_unique, t_inverse), theirs = timed(lambda: torch.unique(ids, return_inverse=True), args.launches)
        U = int(count.item())
        live = ids >= 0
        same = bool(U == int((t_unique >= 0).sum().item()) and torch.equal(torch.sort(unique[:U]).values, t_unique[t_unique >= 0]) and
                    torch.equal(unique[local[live].long()], ids[live]) and bool((local[~live] == -1).all()) and bool((unique[U:] == -1).all()))
        record("unique_ids", ours, theirs, ids.numel(), "ids", ids=int(ids.numel()), distinct=U, matches_torch=same)
        assert same, "unique_ids differs from torch.unique"
        nbytes = int(L.legion_unique_ids_scratch_bytes(ids.numel()))
        scratch = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
        _, abi = timed(lambda: L.legion_unique_ids(S(), P(ids), ids.numel(), P(unique), P(local), P(count), P(scratch), nbytes), args.launches)
        record("unique_ids/abi", abi, theirs, ids.numel(), "ids")
    if "seeds" in arms:
        out, ours = timed(lambda: graph.edge_prediction_seeds(eids[:B], k), args.launches)

        def composed():
            r, cc = torch.searchsorted(indptr, eids[:B], right=True) - 1, col[eids[:B]]
            ng = torch.randint(0, N, (B, k), dtype=torch.int32, device=dev)
            return torch.unique(torch.cat([r.int(), cc, ng.reshape(-1)]), return_inverse=True)
        _, theirs = timed(composed, args.launches)
        record("seeds", ours, theirs, B, "seed edges", seed_edges=B, distinct=int(out[1].item()),
               note="torch's arm draws without any exclusion; ours excludes the row and its entries")
    graph.close()
    text = json.dumps(report, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
