#!/usr/bin/env python3
"""The rates of the per-row selection (legion_row_topk: GraphStorage.select_topk and sample_distinct) on the bench.py graph, each beside
its composition from torch's library kernels on the same GPU and inputs, in a fresh process.

    python tools/topk_rate.py [--scale 26] [--edge-factor 16] [--seeds 1048576] [--hub-seeds 65536] [--max-slots 67108864]
                              [--ks 10,25] [--launches 7] [--out FILE]

Graph, seed lists (`uniform`, `by-degree`), the cut to --max-slots, event timing and medians are those of tools/labor_rate.py; the
weights are eighths in [0, 4] drawn once, a tenth of them zero.  Arms per list, k and mode (largest, smallest, sample):
  abi        legion_row_topk over buffers allocated once, with edge ids and counts
  torch      in_edges' composition (repeat_interleave, gathers of indptr and col), the keys in torch (the float order in int64 ops; E by
             the contract's formula in float64 ops, one operation per call, the hash in int64 ops with logical shifts by masks), a stable
             sort by key and then by dst, and the filter rank-in-row < k
The hand-written result is compared with the composition and must be equal: the same entries of every row in the same order.  Rates:
sampled edges per second (the picks written) and scanned entries per second (the entries of the rows).  This sets no pass mark.
bench.py is not involved and is not changed."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {"largest": 0, "smallest": 1, "sample": 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=26)
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--seeds", type=int, default=1 << 20)
    ap.add_argument("--hub-seeds", type=int, default=1 << 16)
    ap.add_argument("--max-slots", type=int, default=1 << 26)
    ap.add_argument("--ks", type=str, default="10,25")
    ap.add_argument("--launches", type=int, default=7)
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
    uniform = torch.randint(0, N, (args.seeds,), dtype=torch.int32, device=dev, generator=gen)
    edges = torch.randint(0, E, (args.hub_seeds,), dtype=torch.int64, device=dev, generator=gen)
    by_degree = (torch.searchsorted(indptr, edges, right=True) - 1).int()
    w = torch.randint(0, 33, (E,), device=dev, generator=gen).float() / 8
    w[torch.rand(E, device=dev, generator=gen) < 0.1] = 0
    report = {"command": " ".join(["python", "tools/topk_rate.py"] + sys.argv[1:]), "device": torch.cuda.get_device_name(0),
              "library": os.path.relpath(lib.LIB_PATH, ROOT), "graph": f"RMAT-{args.scale}, N={N}, E={E}", "launches": args.launches,
              "lists": {}}
    L = lib.load()
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    S = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    SALT = 7

    def cut(rows, limit):
        """The longest prefix of rows whose entries are at most limit."""
        total = torch.cumsum(indptr[rows.long() + 1] - indptr[rows.long()], 0)
        return rows[:int((total <= limit).sum().item())].contiguous()

    def lsr(x, k):
        return (x >> k) & ((1 << (64 - k)) - 1)

    def splitmix(x):
        x = x + (-0x61C8864680B583EB)                              # 0x9E3779B97F4A7C15 as an int64
        x = (x ^ lsr(x, 30)) * (-0x40A7B892E31B1A47)               # 0xBF58476D1CE4E5B9
        x = (x ^ lsr(x, 27)) * (-0x6B2FB644ECCEEE15)               # 0x94D049BB133111EB
        return x ^ lsr(x, 31)

    def t_exp(e):
        x = splitmix(splitmix(torch.tensor([SALT], dtype=torch.int64, device=dev)) ^ e)
        u = (lsr(x, 12) * 2 + 1).double() * 2.0 ** -53
        m, ex = torch.frexp(u)
        low = m < 0.7071067811865476
        m = torch.where(low, 2.0 * m, m)
        ex = torch.where(low, ex - 1, ex)
        s = (m - 1.0) / (m + 1.0)
        z = s * s
        p = torch.full_like(z, 1.0 / 21.0)
        for t in range(9, -1, -1):
            p = p * z
            p = p + 1.0 / (2 * t + 1)
        a = ex.double() * 0.6931471805599453
        return -(a + (2.0 * s) * p)

    def t_keys(mode, e, src, we):
        """(key int64, eligible)"""
        if mode == 2:
            ok = (src >= 0) & torch.isfinite(we) & (we > 0)
            return (t_exp(e) / torch.where(ok, we, torch.ones_like(we)).double()).view(torch.int64), ok
        b = we.view(torch.int32).long() & 0xFFFFFFFF
        b = torch.where(b == 0x80000000, torch.zeros_like(b), b)
        o = torch.where((b & 0x80000000) != 0, b ^ 0xFFFFFFFF, b | 0x80000000)
        return (0xFFFFFFFF - o if mode == 0 else o), (src >= 0) & ~torch.isnan(we)

    def t_topk(rows, k, mode):
        """(dst, src, eid) of the picks, row by row, best first"""
        r = rows.long()
        deg = indptr[r + 1] - indptr[r]
        offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(deg, 0)])
        M = int(offsets[-1].item())
        dst = torch.repeat_interleave(torch.arange(rows.numel(), device=dev), deg, output_size=M)
        e = indptr[r[dst]] + (torch.arange(M, device=dev) - offsets[dst])
        src = col[e]
        key, ok = t_keys(mode, e, src, w[e])
        dst, e, src, key = dst[ok], e[ok], src[ok], key[ok]
        order = torch.sort(key, stable=True).indices              # (e ascends inside a row: a stable sort keeps the tie rule)
        order = order[torch.sort(dst[order], stable=True).indices]
        dst, e, src = dst[order], e[order], src[order]
        first = torch.searchsorted(dst, torch.arange(rows.numel(), device=dev))
        keep = torch.arange(dst.numel(), device=dev) - first[dst] < k
        return dst[keep], src[keep], e[keep]

    ks = [int(x) for x in args.ks.split(",")]
    for name, rows in (("uniform", cut(uniform, args.max_slots)), ("by-degree", cut(by_degree, args.max_slots))):
        n = rows.numel()
        M = int(graph.row_offsets(rows)[-1].item())
        nbytes = int(L.legion_row_topk_scratch_bytes(n))
        scratch = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
        per_k = {}
        for k in ks:
            src = torch.empty((n, k), dtype=torch.int32, device=dev)
            eid = torch.empty((n, k), dtype=torch.int64, device=dev)
            cnt = torch.empty((n,), dtype=torch.int32, device=dev)
            arms = {}
            for mode_name, mode in MODES.items():
                (t_dst, t_src, t_eid), theirs = timed(lambda: t_topk(rows, k, mode), args.launches)
                call = lambda: L.legion_row_topk(S(), graph.handle, P(rows), n, k, mode, P(w), SALT, P(src), P(eid), P(cnt), P(scratch), nbytes)
                rc, ours = timed(call, args.launches)
                assert rc == 0
                took = src >= 0
                same = bool(torch.equal(torch.nonzero(took)[:, 0], t_dst) and torch.equal(src[took], t_src) and torch.equal(eid[took], t_eid)
                            and torch.equal(took.sum(1).int(), cnt))
                assert same, f"legion_row_topk differs from the torch composition ({name}, k {k}, {mode_name})"
                picks = int(t_dst.numel())
                arms[mode_name] = dict(ours=ours, torch=theirs, picks=picks, sampled_edges_per_second=picks / ours["ms_median"] * 1e3,
                                       scanned_entries_per_second=M / ours["ms_median"] * 1e3,
                                       ours_over_torch=ours["ms_median"] / theirs["ms_median"], matches_torch=same)
                print(f"{name:10s} k {k:3d} {mode_name:9s} {ours['ms_median']:8.3f} ms  {picks / ours['ms_median'] * 1e-6:8.3f} G picks/s "
                      f"{M / ours['ms_median'] * 1e-6:8.3f} G entries/s   torch {theirs['ms_median']:9.3f} ms   ours / torch "
                      f"{ours['ms_median'] / theirs['ms_median']:.4f}", flush=True)
                del t_dst, t_src, t_eid
            per_k[str(k)] = arms
        report["lists"][name] = dict(rows=n, slots=M, ks=per_k)
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
