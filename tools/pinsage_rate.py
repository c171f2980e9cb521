#!/usr/bin/env python3
"""What GraphStorage.pinsage_neighbors costs on the bench.py graph, beside the walks alone and beside today's user path, in a fresh
process.

    python tools/pinsage_rate.py [--scale 26] [--edge-factor 16] [--seeds 262144] [--launches 7] [--shapes R,T,k,p ...] [--out FILE]

Builds the graph bench.py builds (RMAT, seed 20231) and, per shape (default: DGL's PinSAGE example 10,2,3,0.5 and the cap of visits per
seed 64,16,10 at termination 0.5 and 0), times with HIP events --launches launches after one untimed; the median counts.  Arms:
  fused       pinsage_neighbors: walks, counting and top-k in one launch;
  walks       a floor: this build's random_walk alone over the same n * R walks of T steps, restart_prob = the termination probability
              (its first step takes the restart draw too, so with p > 0 it walks LESS than the fused call: steps_taken says how much);
  walks_p0    the same with restart_prob = 0: every load the fused call can make, and more;
  user_path   today's way: random_walk at restart_prob = p, then torch: sort, unique_consecutive, a second sort by (seed, count, id),
              top-k into the same two arrays.  (A user cannot skip the first step's restart draw: at p > 0 these are fewer steps
              than the fused call takes.)
At p = 0 the user path's result is compared with the fused one before anything is timed.  bench.py is not involved and not changed."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def user_path(torch, graph, seeds, R, T, k, p):
    """(neighbors, counts) as pinsage_neighbors orders them, from random_walk's traces with torch alone."""
    n = seeds.numel()
    traces = graph.random_walk(seeds.repeat_interleave(R), T, restart_prob=p)
    vis = traces[:, 1:].reshape(n, R * T).to(torch.int64)
    row = torch.arange(n, device=vis.device, dtype=torch.int64).unsqueeze(1).expand_as(vis)
    live = vis >= 0
    flat = (row[live] << 31) | vis[live]                                   # (seed, vertex)
    flat, _ = torch.sort(flat)
    pair, c = torch.unique_consecutive(flat, return_counts=True)
    seed, v = pair >> 31, pair & 0x7FFFFFFF
    key, _ = torch.sort((seed << 42) | ((1024 - c) << 31) | v)             # seed, count descending, vertex ascending
    seed, c, v = key >> 42, 1024 - ((key >> 31) & 0x7FF), key & 0x7FFFFFFF
    first = torch.searchsorted(seed, torch.arange(n, device=seed.device, dtype=torch.int64))
    rank = torch.arange(seed.numel(), device=seed.device, dtype=torch.int64) - first[seed]
    keep = rank < k
    nb = torch.full((n, k), -1, dtype=torch.int32, device=seed.device)
    ct = torch.zeros((n, k), dtype=torch.int32, device=seed.device)
    nb[seed[keep], rank[keep]] = v[keep].to(torch.int32)
    ct[seed[keep], rank[keep]] = c[keep].to(torch.int32)
    return nb, ct


def timed(torch, fn, launches):
    fn()                                                                   # untimed: first touch of everything
    torch.cuda.synchronize()
    ms = []
    for _ in range(launches):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1))
        del out
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "ms": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=26)
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--seeds", type=int, default=1 << 18)
    ap.add_argument("--launches", type=int, default=7)
    ap.add_argument("--shapes", nargs="*", default=["10,2,3,0.5", "64,16,10,0.5", "64,16,10,0"])
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from legion_amd import engine, synth

    dev = "cuda:0"
    indptr, col = synth.rmat_csr_device(args.scale, args.edge_factor, 20231, dev)
    N, E = indptr.numel() - 1, col.numel()
    graph = engine.GraphStorage(1, indptr, col)
    all_seeds = torch.from_numpy(synth.seed_ids(N, args.seeds, 11)).to(dev)
    if all_seeds.numel() < args.seeds:                   # (a graph smaller than the seed count: seeds repeat)
        all_seeds = all_seeds.repeat((args.seeds + all_seeds.numel() - 1) // all_seeds.numel())[:args.seeds].contiguous()
    report = {"command": " ".join(["python", "tools/pinsage_rate.py"] + sys.argv[1:]), "device": torch.cuda.get_device_name(0),
              "graph": f"RMAT-{args.scale}, N={N}, E={E}", "launches": args.launches, "shapes": []}
    for text in args.shapes:
        R, T, k, p = text.split(",")
        R, T, k, p = int(R), int(T), int(k), float(p)
        n = min(args.seeds, (2 ** 31 - 1) // (R * T))    # the draw index bounds n * R * T
        seeds = all_seeds[:n].contiguous()
        rep = seeds.repeat_interleave(R)
        entry = {"R": R, "T": T, "k": k, "termination_prob": p, "seeds": n, "walks": n * R, "arms": {}}
        nb, ct = graph.pinsage_neighbors(seeds, R, T, k, termination_prob=p)
        torch.cuda.synchronize()
        entry["visits_in_the_top_k"] = int(ct.sum().item())
        entry["rows_full"] = int((ct[:, -1] > 0).sum().item())
        if p == 0.0:
            unb, uct = user_path(torch, graph, seeds, R, T, k, 0.0)
            torch.cuda.synchronize()
            entry["user_path_equals_fused"] = bool(torch.equal(unb, nb) and torch.equal(uct, ct))
            del unb, uct
        del nb, ct
        arms = entry["arms"]
        arms["fused"] = timed(torch, lambda: graph.pinsage_neighbors(seeds, R, T, k, termination_prob=p), args.launches)
        arms["walks"] = timed(torch, lambda: graph.random_walk(rep, T, restart_prob=p), args.launches)
        arms["walks_p0"] = arms["walks"] if p == 0.0 else timed(torch, lambda: graph.random_walk(rep, T), args.launches)
        arms["user_path"] = timed(torch, lambda: user_path(torch, graph, seeds, R, T, k, p), args.launches)
        for name, restart in (("walks", p), ("walks_p0", 0.0)):
            traces = graph.random_walk(rep, T, restart_prob=restart)
            arms[name] = dict(arms[name], steps_taken=int((traces[:, 1:] >= 0).sum().item()))
            del traces
        f = arms["fused"]["ms_median"]
        entry["fused_over_walks"] = f / arms["walks"]["ms_median"]
        entry["fused_over_walks_p0"] = f / arms["walks_p0"]["ms_median"]
        entry["user_path_over_fused"] = arms["user_path"]["ms_median"] / f
        entry["seeds_per_sec_fused"] = n / f * 1e3
        print(f"R={R} T={T} k={k} p={p} n={n}: fused {f:.3f} ms, walks {arms['walks']['ms_median']:.3f} ms, walks at p=0 "
              f"{arms['walks_p0']['ms_median']:.3f} ms, user path {arms['user_path']['ms_median']:.3f} ms", flush=True)
        report["shapes"].append(entry)
        del rep, seeds
        torch.cuda.empty_cache()
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
