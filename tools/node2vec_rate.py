#!/usr/bin/env python3
"""The rate of GraphStorage.node2vec_random_walk on the bench.py graph beside random_walk on the same walks, in a fresh process.

    python tools/node2vec_rate.py [--scale 26] [--edge-factor 16] [--walks 1048576] [--length 16] [--launches 7] [--out FILE]

Graph, weights, seeds, event timing and medians are those of tools/random_walk_rate.py (RMAT, seed 20231; hash-derived weights in
(0, 1]; --launches timed launches after one untimed, the median counts).  node2vec searches rows, so they must be sorted: the tool asks
GraphStorage.rows_sorted(), says what it found and, if need be, sorts every row's entries (one device sort of (row, entry) keys) before
anything is timed -- random_walk is timed on the same sorted graph.  Arms: random_walk; node2vec at (p, q) = (1, 1), (0.5, 2), (2, 0.5)
and (4, 0.25), each without and with edge ids; one weighted arm, (0.5, 2).  Per arm: ms, steps taken per second (an ended walk takes
none), and -- from a restatement of the rule in torch on the device, whose traces must equal the kernel's -- the mean tries per step
and the share of tries whose class only the search of the previous row could decide.  bench.py is not involved and is not changed."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M31 = 2 ** 31 - 1


def _mulmod(a, b):
    return (a * b) % M31                                 # int64: both below 2^31


def minstd(k):
    """48271^k mod (2^31 - 1) for an int64 tensor of exponents, by squaring."""
    import torch
    out = torch.ones_like(k)
    sq = torch.full_like(k, 48271)
    for bit in range(33):
        out = torch.where((k >> bit) & 1 == 1, _mulmod(out, sq), out)
        sq = _mulmod(sq, sq)
    return out


def unit_of(x):
    import torch
    return (x - 1).to(torch.float64) / 2147483646.0


def restate(indptr, col, seeds, length, p, q, table=None, max_tries=256, base=0):
    """legion_node2vec_walk's rule (include/legion_hip.h) in torch, every walk at once, try by try: (traces, tries, searched tries).
    The counterpart of tests/node2vec_ref.py on whatever device the tensors live on."""
    import torch
    dev = col.device
    n, node_num = seeds.numel(), indptr.numel() - 1
    a, b = 1.0 / float(torch.tensor(p, dtype=torch.float32)), 1.0 / float(torch.tensor(q, dtype=torch.float32))
    mx, lo_w, hi_w = max(a, 1.0, b), min(1.0, b), max(1.0, b)
    rows = torch.repeat_interleave(torch.arange(node_num, dtype=torch.int64, device=dev), indptr[1:] - indptr[:-1])
    keys = (rows << 32) | (col.to(torch.int64) + 1)      # increasing: the rows are sorted
    del rows
    traces = torch.full((n, length + 1), -1, dtype=torch.int32, device=dev)
    traces[:, 0] = seeds
    v = seeds.to(torch.int64)
    t = torch.full_like(v, -1)
    idx = base + torch.arange(n, dtype=torch.int64, device=dev) * length
    tries = searched = 0
    for j in range(1, length + 1):
        nxt = torch.full_like(v, -1)
        at = torch.nonzero((v >= 0) & (v < node_num)).flatten()
        s = indptr[v[at]]
        D = indptr[v[at] + 1] - s
        at, s, D = at[D > 0], s[D > 0], D[D > 0]
        T = None
        if table is not None:
            T = table[s + D - 1].to(torch.float64)
            at, s, D, T = at[T > 0], s[T > 0], D[T > 0], T[T > 0]
        x = minstd(idx[at] + j)                          # the draw index base + w * length + (j - 1), plus one
        step23, step22 = minstd(torch.tensor([1 << 23, 1 << 22], dtype=torch.int64, device=dev))
        for i in range(max_tries):
            if at.numel() == 0:
                break
            tries += int(at.numel())
            r = unit_of(x)
            if table is None:
                pick = (r * D.to(torch.float64)).to(torch.int64)
            else:
                target = r * T
                lo, hi = torch.zeros_like(D), D.clone()      # #{e : cdf[s + e] <= target} by bisection
                while True:
                    open_ = lo < hi
                    if not bool(open_.any()):
                        break
                    mid = (lo + hi) // 2
                    le = table[s + torch.minimum(mid, D - 1)].to(torch.float64) <= target
                    lo, hi = torch.where(open_ & le, mid + 1, lo), torch.where(open_ & ~le, mid, hi)
                pick = torch.minimum(lo, D - 1)
            u = col[s + pick].to(torch.int64)
            dead = u < 0
            if j == 1 or i == max_tries - 1:
                accept = ~dead
            else:
                tt = t[at]
                key = (tt << 32) | (u + 1)
                pos = torch.clamp(torch.searchsorted(keys, key), max=keys.numel() - 1)
                member = keys[pos] == key
                z = unit_of(_mulmod(x, step22)) * mx
                wt = torch.full_like(z, b)
                wt[member] = 1.0
                wt[u == tt] = a
                accept = (z < wt) & ~dead
                searched += int((~dead & (u != tt) & (z >= lo_w) & (z < hi_w)).sum())
            nxt[at[accept]] = u[accept]
            go = ~accept & ~dead
            at, s, D, x = at[go], s[go], D[go], _mulmod(x[go], step23)
            if T is not None:
                T = T[go]
        t = torch.where(nxt >= 0, v, t)
        v = nxt
        traces[:, j] = v.to(torch.int32)
    return traces, tries, searched


def sort_rows(indptr, col):
    """col with every row's entries in non-decreasing order (as int32)."""
    import torch
    rows = torch.repeat_interleave(torch.arange(indptr.numel() - 1, dtype=torch.int64, device=col.device), indptr[1:] - indptr[:-1])
    keys = (rows << 32) | (col.to(torch.int64) + (1 << 31))
    del rows
    keys = torch.sort(keys).values
    return ((keys & 0xFFFFFFFF) - (1 << 31)).to(torch.int32)


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
    was_sorted = graph.rows_sorted()
    print(f"the bench graph's rows are {'sorted' if was_sorted else 'NOT sorted: sorting them here, before anything is timed'}", flush=True)
    if not was_sorted:
        graph.close()
        col = sort_rows(indptr, col)
        torch.cuda.synchronize()
        graph = engine.GraphStorage(1, indptr, col)
        assert graph.rows_sorted(), "rows unsorted after the sort"
    e = torch.arange(E, dtype=torch.int64, device=dev)
    w = (((e * 2654435761) % (1 << 20)) + 1).to(torch.float32) / float(1 << 20)
    del e
    graph.set_edge_weights(w)
    torch.cuda.synchronize()
    del w
    seeds = torch.from_numpy(synth.seed_ids(N, args.walks, 11)).to(dev)
    if seeds.numel() < args.walks:                       # (a graph smaller than the walk count: seeds repeat)
        seeds = seeds.repeat((args.walks + seeds.numel() - 1) // seeds.numel())[:args.walks].contiguous()
    report = {"command": " ".join(["python", "tools/node2vec_rate.py"] + sys.argv[1:]), "device": torch.cuda.get_device_name(0),
              "graph": f"RMAT-{args.scale}, N={N}, E={E}", "rows_were_sorted": bool(was_sorted), "walks": args.walks, "length": args.length,
              "launches": args.launches, "arms": {}}
    arms = [("random_walk", None, False)] + [(f"node2vec({p:g},{q:g})", (p, q), False) for p, q in ((1, 1), (0.5, 2), (2, 0.5), (4, 0.25))] + \
           [("node2vec(0.5,2) weighted", (0.5, 2), True)]
    for name, pq, weighted in arms:
        stats = None
        for eids in (False, True):
            if pq is None:
                call = lambda: graph.random_walk(seeds, args.length, weighted=weighted, return_eids=eids)
            else:
                call = lambda: graph.node2vec_random_walk(seeds, pq[0], pq[1], args.length, weighted=weighted, return_eids=eids)
            out = call()                                 # untimed: first touch of everything
            torch.cuda.synchronize()
            ms = []
            for _ in range(args.launches):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                out = call()
                t1.record()
                torch.cuda.synchronize()
                ms.append(t0.elapsed_time(t1))
            traces = out[0] if eids else out
            taken = int((traces[:, 1:] >= 0).sum().item())
            if pq is not None and stats is None:         # (the walks do not depend on the edge ids: counted once per (p, q))
                want, tries, searched = restate(indptr, col, seeds, args.length, pq[0], pq[1], table=graph.edge_cdf() if weighted else None)
                stats = {"restatement_matches": bool(torch.equal(want, traces)), "tries": tries, "tries_per_step": tries / max(taken, 1),
                         "searched_share_of_tries": searched / max(tries, 1)}
                del want
            med = statistics.median(ms)
            arm = name + ("+eids" if eids else "")
            report["arms"][arm] = dict({"ms_median": med, "ms_min": min(ms), "ms_max": max(ms), "ms": ms, "steps_taken": taken,
                                        "steps_per_sec": taken / med * 1e3,
                                        "walks_alive_at_the_end": int((traces[:, -1] >= 0).sum().item())}, **(stats or {}))
            extra = f"  {stats['tries_per_step']:.3f} tries/step  {stats['searched_share_of_tries'] * 100:5.1f} % searched  " \
                    f"restatement {'==' if stats['restatement_matches'] else '!='} kernel" if stats else ""
            print(f"{arm:30s} {med:8.3f} ms  {taken / med * 1e-6:8.3f} G steps/s{extra}", flush=True)
            del out, traces
    base = report["arms"]["random_walk"]["ms_median"]
    report["unbiased_over_random_walk"] = report["arms"]["node2vec(1,1)"]["ms_median"] / base
    report["unbiased_over_random_walk_eids"] = report["arms"]["node2vec(1,1)+eids"]["ms_median"] / report["arms"]["random_walk+eids"]["ms_median"]
    print(f"node2vec(1,1) / random_walk: {report['unbiased_over_random_walk']:.3f} (with edge ids {report['unbiased_over_random_walk_eids']:.3f})")
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
