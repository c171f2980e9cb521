#!/usr/bin/env python3
"""The rate of GraphStorage.random_walk on the bench.py graph, unweighted and weighted, in a fresh process.

    python tools/random_walk_rate.py [--scale 26] [--edge-factor 16] [--walks 1048576] [--length 16] [--launches 7] [--out FILE]

Builds the graph bench.py builds (RMAT, seed 20231), gives it hash-derived positive float32 weights in (0, 1] (the weights of
tools/sample_weighted_ab.py), and times --launches launches of --walks walks of --length steps from seeded vertices with HIP events,
restart_prob = 0, after one untimed launch; the median counts.  Per arm (unweighted, weighted, each without and with edge ids) the
report gives steps/s over the steps walks took (an ended walk takes none) and the achieved rate of random requests: per step one
16-byte row-pointer pair and one column entry, and per weighted step the row total and the ceil(log2(D + 1)) probes of its search.
bench.py is not involved and is not changed."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=26)
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--walks", type=int, default=1 << 20)
    ap.add_argument("--length", type=int, default=16)
    ap.add_argument("--launches", type=int, default=7)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from legion_amd import engine, synth

    dev = "cuda:0"
    indptr, col = synth.rmat_csr_device(args.scale, args.edge_factor, 20231, dev)
    N, E = indptr.numel() - 1, col.numel()
    graph = engine.GraphStorage(1, indptr, col)
    e = torch.arange(E, dtype=torch.int64, device=dev)
    w = (((e * 2654435761) % (1 << 20)) + 1).to(torch.float32) / float(1 << 20)
    del e
    graph.set_edge_weights(w)
    torch.cuda.synchronize()
    del w
    seeds = torch.from_numpy(synth.seed_ids(N, args.walks, 11)).to(dev)
    if seeds.numel() < args.walks:                       # (a graph smaller than the walk count: seeds repeat)
        seeds = seeds.repeat((args.walks + seeds.numel() - 1) // seeds.numel())[:args.walks].contiguous()
    report = {"command": " ".join(["python", "tools/random_walk_rate.py"] + sys.argv[1:]), "device": torch.cuda.get_device_name(0),
              "graph": f"RMAT-{args.scale}, N={N}, E={E}", "walks": args.walks, "length": args.length, "launches": args.launches, "arms": {}}
    for weighted in (False, True):
        for eids in (False, True):
            out = graph.random_walk(seeds, args.length, weighted=weighted, return_eids=eids)      # untimed: first touch of everything
            torch.cuda.synchronize()
            ms = []
            for _ in range(args.launches):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                out = graph.random_walk(seeds, args.length, weighted=weighted, return_eids=eids)
                t1.record()
                torch.cuda.synchronize()
                ms.append(t0.elapsed_time(t1))
            traces = out[0] if eids else out
            frm = traces[:, :-1].reshape(-1).to(torch.int64)
            frm = frm[frm >= 0]                          # every step a walk attempted: it read the row-pointer pair
            deg = indptr[frm + 1] - indptr[frm]
            deg = deg[deg > 0]                           # ... and, with a row, the column entry (and the table when weighted)
            taken = int((traces[:, 1:] >= 0).sum().item())
            requests = int(frm.numel()) + int(deg.numel())
            if weighted:
                requests += int(deg.numel()) + int(torch.ceil(torch.log2(deg.to(torch.float64) + 1.0)).sum().item())
            med = statistics.median(ms)
            arm = ("weighted" if weighted else "unweighted") + ("+eids" if eids else "")
            report["arms"][arm] = {"ms_median": med, "ms_min": min(ms), "ms_max": max(ms), "ms": ms, "steps_taken": taken,
                                   "steps_per_sec": taken / med * 1e3, "random_requests": requests,
                                   "random_requests_per_sec": requests / med * 1e3,
                                   "walks_alive_at_the_end": int((traces[:, -1] >= 0).sum().item())}
            print(f"{arm:16s} {med:8.3f} ms  {taken / med * 1e-6:8.2f} G steps/s  {requests / med * 1e-6:8.2f} G requests/s", flush=True)
            del out, traces, frm, deg
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
