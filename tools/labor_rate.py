#!/usr/bin/env python3
"""The rates of layer-neighbour sampling (legion_labor_count, legion_labor_edges, GraphStorage.labor_edges, labor_block) on the bench.py
graph, each beside its composition from torch's library kernels on the same GPU and inputs, in a fresh process; and the figure that
motivates the op: the input nodes of two LABOR layers beside the distinct vertices per-seed sampling needs for the same seeds.

    python tools/labor_rate.py [--scale 26] [--edge-factor 16] [--seeds 1048576] [--hub-seeds 65536] [--max-slots 268435456]
                               [--fanouts 10,25] [--launches 7] [--out FILE]

Graph, seed lists (`uniform`, `by-degree`), the cut to --max-slots, event timing and medians are those of tools/in_edges_rate.py.  Arms
per list and fan-out:
  count/abi     legion_labor_count over buffers allocated once      | in_edges' composition (repeat_interleave, gathers of indptr and
  edges/abi     legion_labor_edges with edge ids, cap = K           |   col), splitmix64 and the compare in torch int64 ops (logical
  pair/abi      both calls                                          |   shifts by masks), then a boolean mask over dst, src and eid
  labor_edges   the Python method: offsets, two reads, allocation   |
  labor_block   over the longest prefix of distinct seeds with n + M <= 2^20 | the composition, then torch.unique(return_inverse=True)
Every hand-written result is compared with the torch composition and must be equal.  Then, record only: for 1 024 and 8 000 uniformly
drawn distinct seeds, two layers at fan-outs 25 then 10 -- the input nodes of the LABOR blocks with one salt for both layers and with a
salt per layer, beside the distinct vertices of per-seed uniform sampling (fan-out draws with replacement per seed, the neighbour
sampler's default mode, composed in torch).  bench.py is not involved and is not changed."""
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
    ap.add_argument("--seeds", type=int, default=1 << 20)
    ap.add_argument("--hub-seeds", type=int, default=1 << 16)
    ap.add_argument("--max-slots", type=int, default=1 << 28)
    ap.add_argument("--fanouts", type=str, default="10,25")
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
    report = {"command": " ".join(["python", "tools/labor_rate.py"] + sys.argv[1:]), "device": torch.cuda.get_device_name(0),
              "library": os.path.relpath(lib.LIB_PATH, ROOT), "graph": f"RMAT-{args.scale}, N={N}, E={E}", "launches": args.launches,
              "lists": {}, "layers": {}}
    L = lib.load()
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    S = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

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

    def t_keep(src, d, fanout, salt):
        key = splitmix(torch.tensor([salt], dtype=torch.int64, device=dev))
        h = lsr(splitmix(key ^ src.long()), 32)
        return (h * (d >> 32) + lsr(h * (d & 0xFFFFFFFF), 32) < fanout) & (src >= 0)

    def t_labor(rows, fanout, salt):
        r = rows.long()
        deg = indptr[r + 1] - indptr[r]
        offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(deg, 0)])
        M = int(offsets[-1].item())
        dst = torch.repeat_interleave(torch.arange(rows.numel(), device=dev), deg, output_size=M)
        e = indptr[r[dst]] + (torch.arange(M, device=dev) - offsets[dst])
        src = col[e]
        keep = t_keep(src, deg[dst], fanout, salt)
        return dst[keep], src[keep], e[keep]

    fanouts = [int(x) for x in args.fanouts.split(",")]
    for name, rows in (("uniform", cut(uniform, args.max_slots)), ("by-degree", cut(by_degree, args.max_slots))):
        n = rows.numel()
        off = graph.row_offsets(rows)
        M = int(off[-1].item())
        per_fanout = {}
        for fanout in fanouts:
            arms = {}

            def record(arm, ours, theirs, slots=M, **more):
                out = dict(ours=ours, slots=slots, slots_per_second=slots / ours["ms_median"] * 1e3, torch=theirs,
                           ours_over_torch=ours["ms_median"] / theirs["ms_median"], **more)
                arms[arm] = out
                print(f"{name:10s} fanout {fanout:3d} {arm:12s} {ours['ms_median']:8.3f} ms  {out['slots_per_second'] * 1e-9:7.3f} G slots/s"
                      f"   torch {theirs['ms_median']:8.3f} ms   ours / torch {out['ours_over_torch']:.3f}", flush=True)

            (t_dst, t_src, t_eid), theirs = timed(lambda: t_labor(rows, fanout, 7), args.launches)
            K = int(t_dst.numel())
            nbytes = int(L.legion_labor_scratch_bytes(M))
            scratch = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
            count = torch.zeros(1, dtype=torch.int64, device=dev)
            dst, src = (torch.empty(max(K, 1), dtype=torch.int32, device=dev) for _ in range(2))
            eid = torch.empty(max(K, 1), dtype=torch.int64, device=dev)
            c_count = lambda: L.legion_labor_count(S(), graph.handle, P(rows), n, P(off), M, fanout, 7, P(count), P(scratch), nbytes)
            c_edges = lambda: L.legion_labor_edges(S(), graph.handle, P(rows), n, P(off), M, fanout, 7, P(scratch), nbytes, K, P(dst), P(src),
                                                   P(eid))
            _, t_c = timed(c_count, args.launches)
            assert int(count.item()) == K, "legion_labor_count differs from the torch composition"
            _, t_e = timed(c_edges, args.launches)
            same = bool(torch.equal(dst[:K].long(), t_dst) and torch.equal(src[:K], t_src) and torch.equal(eid[:K], t_eid))
            assert same, "legion_labor_edges differs from the torch composition"
            record("count/abi", t_c, theirs, kept=K)
            record("edges/abi", t_e, theirs, matches_torch=same)
            _, t_p = timed(lambda: (c_count(), c_edges()), args.launches)
            record("pair/abi", t_p, theirs)
            got, ours = timed(lambda: graph.labor_edges(rows, fanout, salt=7, return_eids=True), args.launches)
            same = bool(torch.equal(got[0].long(), t_dst) and torch.equal(got[1], t_src) and torch.equal(got[2], t_eid))
            assert same, "labor_edges differs from the torch composition"
            record("labor_edges", ours, theirs, matches_torch=same)
            del dst, src, eid, got, t_dst, t_src, t_eid
            seeds = torch.unique(rows.long(), sorted=False).int()
            seeds = seeds[torch.randperm(seeds.numel(), device=dev, generator=gen)]
            total = torch.cumsum(indptr[seeds.long() + 1] - indptr[seeds.long()], 0) + torch.arange(1, seeds.numel() + 1, device=dev)
            seeds = seeds[:int((total <= engine.UNIQUE_MAX_IDS).sum().item())].contiguous()
            if seeds.numel():
                blk, ours = timed(lambda: graph.labor_block(seeds, fanout, salt=7), args.launches)

                def composed():
                    d, s, _ = t_labor(seeds, fanout, 7)
                    return torch.unique(torch.cat([seeds, s]), return_inverse=True), d, s
                ((t_unique, _), t_d, t_s), theirs_b = timed(composed, args.launches)
                same = bool(torch.equal(torch.sort(blk[0]).values, t_unique) and torch.equal(blk[0][:seeds.numel()], seeds) and
                            torch.equal(blk[1].long(), t_d) and torch.equal(blk[0][blk[2].long()], t_s))
                assert same, "labor_block differs from the torch composition"
                record("labor_block", ours, theirs_b, slots=int(total[seeds.numel() - 1].item()) - int(seeds.numel()),
                       seeds=int(seeds.numel()), kept=int(blk[1].numel()), distinct=int(blk[0].numel()), matches_torch=same)
            per_fanout[str(fanout)] = dict(kept=K, arms=arms)
        report["lists"][name] = dict(rows=n, slots=M, fanouts=per_fanout)

    # the motivating figure, record only
    for count_seeds in (1024, 8000):
        seeds = torch.randperm(N, device=dev, generator=gen)[:count_seeds].int()

        def per_seed(s, fanout):
            """distinct vertices of s and of fanout uniform draws with replacement from each row of s that has entries"""
            r = s.long()
            deg = indptr[r + 1] - indptr[r]
            has = deg > 0
            u = torch.rand((int(has.sum().item()), fanout), device=dev, generator=gen)
            e = indptr[r[has]][:, None] + (u * deg[has][:, None]).long().clamp(max=E - 1)
            picked = col[e.reshape(-1)]
            return torch.unique(torch.cat([r, picked[picked >= 0].long()])).int()

        one = graph.labor_block(graph.labor_block(seeds, 25, salt=1)[0], 10, salt=1)[0]
        inner = graph.labor_block(seeds, 25, salt=1)[0]
        two = graph.labor_block(inner, 10, salt=2)[0]
        sampled1 = per_seed(seeds, 25)
        sampled2 = per_seed(sampled1, 10)
        row = dict(seeds=count_seeds, fanouts=[25, 10], labor_layer1_input_nodes=int(inner.numel()),
                   labor_one_salt_input_nodes=int(one.numel()), labor_salt_per_layer_input_nodes=int(two.numel()),
                   per_seed_layer1_distinct=int(sampled1.numel()), per_seed_distinct=int(sampled2.numel()))
        print(row, flush=True)
        report["layers"][str(count_seeds)] = row
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
