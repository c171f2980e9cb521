#!/usr/bin/env python3
"""The rates of metapath walks and of PinSAGE over a metapath (legion_metapath_walk, legion_pinsage_metapath_neighbors) on the bench.py
graph, beside the library's own untyped ops on the same seeds, in a fresh process.

    python tools/metapath_rate.py [--scale 26] [--edge-factor 16] [--walks 1048576] [--length 16] [--types 1,4,64] [--launches 7]
                                  [--path A,B] [--out FILE]

Graph, seed lists (`uniform`: vertices drawn uniformly; `by-degree`: the rows of uniformly drawn edges, the hub list), edge types,
event timing and medians are those of tools/etype_rate.py.  Arms per T and list, L = 2 (the first and the last type in turn):
  walk      legion_metapath_walk, --walks walks of --length steps, without and with edge ids; yardstick legion_random_walk unweighted
  pinsage   legion_pinsage_metapath_neighbors, R = 16 walks of Q = --length / 2 traversals, k = 10, on the first --walks / 16 seeds;
            yardstick legion_pinsage_neighbors with walk_length = Q * 2: the same number of steps
  first step  (lists `short rows`, `long rows`: vertices of 1 .. 16 and of more than 16 entries) one step of legion_metapath_walk
            against one of legion_random_walk: the short class and the long class apart
and the share of steps taken from rows of at most 16 entries (the short class) among the reference walk's steps.  At T = 1 a metapath
walk IS the yardstick's walk, so ours / yardstick there is the cost of the segment step.  Ratios above 1 are slower than the yardstick.
This sets no pass mark.  bench.py is not involved and is not changed."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=26)
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--walks", type=int, default=1 << 20)
    ap.add_argument("--length", type=int, default=16)
    ap.add_argument("--types", type=str, default="1,4,64")
    ap.add_argument("--launches", type=int, default=7)
    ap.add_argument("--path", type=str, default="", help="the two types of the metapath, e.g. 1,2 (default: 0 and T - 1)")
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from legion_amd import engine, lib, synth
    from tools.link_rate import timed

    dev = "cuda:0"
    indptr, col = synth.rmat_csr_device(args.scale, args.edge_factor, 20231, dev)
    N, E = indptr.numel() - 1, col.numel()
    graph = engine.GraphStorage(1, indptr, col)
    gen = torch.Generator(device=dev)
    gen.manual_seed(20231)
    n, length = args.walks, args.length
    uniform = torch.randint(0, N, (n,), dtype=torch.int32, device=dev, generator=gen)
    edges = torch.randint(0, E, (n,), dtype=torch.int64, device=dev, generator=gen)
    by_degree = (torch.searchsorted(indptr, edges, right=True) - 1).int()
    u = torch.rand(E, device=dev, generator=gen)
    row = torch.repeat_interleave(torch.arange(N, device=dev), indptr[1:] - indptr[:-1], output_size=E)
    degree = indptr[1:] - indptr[:-1]
    pick = lambda rows: rows[torch.randint(0, rows.numel(), (n,), device=dev, generator=gen)].int()
    short_rows, long_rows = pick(torch.nonzero((degree > 0) & (degree <= 16)).flatten()), pick(torch.nonzero(degree > 16).flatten())
    command = (f"python tools/metapath_rate.py --scale {args.scale} --edge-factor {args.edge_factor} --walks {args.walks} "
               f"--length {args.length} --types {args.types} --launches {args.launches}" +
               (f" --path {args.path}" if args.path else ""))                           # what was measured, not where it was written
    report = {"command": command, "device": torch.cuda.get_device_name(0),
              "library": os.path.relpath(lib.LIB_PATH, ROOT), "graph": f"RMAT-{args.scale}, N={N}, E={E}", "launches": args.launches,
              "walks": n, "length": length, "types": {}}
    L = lib.load()
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    S = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    traces = torch.empty((n, length + 1), dtype=torch.int32, device=dev)
    eids = torch.empty((n, length), dtype=torch.int64, device=dev)
    R, Q, K = 16, length // 2, 10
    ns = n // R
    nb, ct = torch.empty((ns, K), dtype=torch.int32, device=dev), torch.empty((ns, K), dtype=torch.int32, device=dev)
    for T in [int(x) for x in args.types.split(",")]:
        etype = (torch.sort(row * 64 + (u * u * u * T).long().clamp(max=T - 1)).values % 64).to(torch.uint8)
        graph.set_edge_types(etype, T)
        path = (ctypes.c_uint8 * 2)(*([int(x) for x in args.path.split(",")] if args.path else [0, T - 1]))
        per_list = {}
        for name, seeds in (("uniform", uniform), ("by-degree", by_degree)):
            arms = {}
            for ids in (False, True):
                e = P(eids) if ids else None
                rc, theirs = timed(lambda: L.legion_random_walk(S(), graph.handle, P(seeds), n, length, 0, 0.0, 0, P(traces), e), args.launches)
                assert rc == 0
                rc, ours = timed(lambda: L.legion_metapath_walk(S(), graph.handle, P(seeds), n, path, 2, length, 0.0, 0, P(traces), e), args.launches)
                assert rc == 0
                left = traces[:, :-1][traces[:, 1:] >= 0].long()                       # the vertices our walks stepped from
                deg = indptr[left + 1] - indptr[left]
                arms[f"walk edge_ids={int(ids)}"] = dict(
                    ours=ours, yardstick=theirs, yardstick_op="legion_random_walk", walks_per_second=n / ours["ms_median"] * 1e3,
                    steps_taken=int(left.numel()), steps_per_second=left.numel() / ours["ms_median"] * 1e3,
                    short_row_share=float((deg <= 16).float().mean().item()) if left.numel() else 0.0,
                    ours_over_yardstick=ours["ms_median"] / theirs["ms_median"])
                print(f"T {T:2d} {name:10s} walk ids {int(ids)}: {ours['ms_median']:8.3f} ms {n / ours['ms_median'] * 1e-3:8.2f} M walks/s, {left.numel()} steps, "
                      f"short rows {arms[f'walk edge_ids={int(ids)}']['short_row_share']:.3f}   legion_random_walk {theirs['ms_median']:8.3f} ms   "
                      f"ours / yardstick {ours['ms_median'] / theirs['ms_median']:.3f}", flush=True)
            rc, theirs = timed(lambda: L.legion_pinsage_neighbors(S(), graph.handle, P(seeds), ns, R, Q * 2, K, 0, 0.5, 0, P(nb), P(ct)), args.launches)
            assert rc == 0
            rc, ours = timed(lambda: L.legion_pinsage_metapath_neighbors(S(), graph.handle, P(seeds), ns, path, 2, R, Q, K, 0.5, 0, P(nb), P(ct)), args.launches)
            assert rc == 0
            arms["pinsage"] = dict(ours=ours, yardstick=theirs, yardstick_op=f"legion_pinsage_neighbors R={R} T={Q * 2}", seeds=ns, R=R, Q=Q, k=K,
                                   seeds_per_second=ns / ours["ms_median"] * 1e3, ours_over_yardstick=ours["ms_median"] / theirs["ms_median"])
            print(f"T {T:2d} {name:10s} pinsage R {R} Q {Q}: {ours['ms_median']:8.3f} ms   legion_pinsage_neighbors R {R} T {Q * 2} {theirs['ms_median']:8.3f} ms   "
                  f"ours / yardstick {ours['ms_median'] / theirs['ms_median']:.3f}", flush=True)
            per_list[name] = arms
        first = torch.empty((n, 2), dtype=torch.int32, device=dev)                    # the split: ONE step from rows of one class
        for name, seeds in (("short rows", short_rows), ("long rows", long_rows)):
            rc, theirs = timed(lambda: L.legion_random_walk(S(), graph.handle, P(seeds), n, 1, 0, 0.0, 0, P(first), None), args.launches)
            assert rc == 0
            rc, ours = timed(lambda: L.legion_metapath_walk(S(), graph.handle, P(seeds), n, path, 2, 1, 0.0, 0, P(first), None), args.launches)
            assert rc == 0
            per_list[name] = {"first step": dict(ours=ours, yardstick=theirs, yardstick_op="legion_random_walk", steps_taken=int((first[:, 1] >= 0).sum().item()),
                                                 ours_over_yardstick=ours["ms_median"] / theirs["ms_median"])}
            print(f"T {T:2d} {name:10s} first step: {ours['ms_median']:8.3f} ms   legion_random_walk {theirs['ms_median']:8.3f} ms   "
                  f"ours / yardstick {ours['ms_median'] / theirs['ms_median']:.3f}", flush=True)
        report["types"][str(T)] = per_list
    graph.close()
    text = json.dumps(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
