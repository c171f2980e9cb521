#!/usr/bin/env python3
"""The rates of the full-neighbour ops (GraphStorage.row_offsets, in_edges, full_neighbor_block) on the bench.py graph, each beside its
composition from torch's library kernels on the same GPU and inputs, in a fresh process.

    python tools/in_edges_rate.py [--scale 26] [--edge-factor 16] [--seeds 1048576] [--hub-seeds 65536] [--max-slots 268435456]
                                  [--launches 7] [--out FILE]

Graph, event timing and medians are those of tools/link_rate.py (RMAT, seed 20231; --launches timed launches after one untimed, the
median counts).  Two seed lists: `uniform`, --seeds vertices drawn uniformly, and `by-degree`, --hub-seeds rows of uniformly drawn edges
(the hub-heavy case); each is cut to the longest prefix whose entries fit --max-slots.  Arms per list:
  offsets       row_offsets                                   | indptr[rows + 1] - indptr[rows], cumsum
  expand        in_edges with edge ids, the offsets given     | repeat_interleave(arange(n), deg), arange(M) - offsets[dst],
  expand/no-eids                                              |   indptr[rows[dst]] + j, col[e]
  in_edges      the Python method: offsets, the read of M, allocation, expand
  .../abi       the C call alone over buffers allocated once
  block         full_neighbor_block over the longest prefix of distinct seeds with n + M <= 2^20 | the composition, then
                torch.unique(return_inverse=True) (sorted, not seeds-first)
Every hand-written result is checked against the torch composition.  GB/s counts the algorithmic bytes: 4 + 4 (+ 8) written and 4 read
per slot.  LEGION_HIP_LIB=<another build> times that build (how the two forms of the expansion of DESIGN.md 4.17 were timed).  bench.py
is not involved and is not changed."""
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
    report = {"command": " ".join(["python", "tools/in_edges_rate.py"] + sys.argv[1:]), "device": torch.cuda.get_device_name(0),
              "library": os.path.relpath(lib.LIB_PATH, ROOT), "graph": f"RMAT-{args.scale}, N={N}, E={E}", "launches": args.launches,
              "lists": {}}
    L = lib.load()
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    S = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def cut(rows, limit):
        """The longest prefix of rows whose entries are at most limit."""
        total = torch.cumsum(indptr[rows.long() + 1] - indptr[rows.long()], 0)
        return rows[:int((total <= limit).sum().item())].contiguous()

    def t_offsets(rows):
        r = rows.long()
        deg = indptr[r + 1] - indptr[r]
        return torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(deg, 0)]), deg

    def t_expand(rows, offsets, deg, M):
        dst = torch.repeat_interleave(torch.arange(rows.numel(), device=dev), deg, output_size=M)
        e = indptr[rows.long()[dst]] + (torch.arange(M, device=dev) - offsets[dst])
        return dst, col[e], e

    for name, rows in (("uniform", cut(uniform, args.max_slots)), ("by-degree", cut(by_degree, args.max_slots))):
        n = rows.numel()
        arms = {}

        def record(arm, ours, theirs, slots, bytes_per_slot, **more):
            out = dict(ours=ours, slots_per_second=slots / ours["ms_median"] * 1e3, GB_per_second=slots * bytes_per_slot / ours["ms_median"] * 1e-6,
                       **more)
            line = f"{name:10s} {arm:16s} {ours['ms_median']:8.3f} ms  {out['slots_per_second'] * 1e-9:7.3f} G slots/s  {out['GB_per_second']:7.1f} GB/s"
            if theirs is not None:
                out["torch"] = theirs
                out["ours_over_torch"] = ours["ms_median"] / theirs["ms_median"]
                line += f"   torch {theirs['ms_median']:8.3f} ms   ours / torch {out['ours_over_torch']:.3f}"
            arms[arm] = out
            print(line, flush=True)

        (t_off, deg), their_off = timed(lambda: t_offsets(rows), args.launches)
        M = int(t_off[-1].item())
        off, our_off = timed(lambda: graph.row_offsets(rows), args.launches)
        assert torch.equal(off, t_off), "row_offsets differs from the cumsum"
        record("offsets", our_off, their_off, n, 12)
        nbytes = int(L.legion_row_offsets_scratch_bytes(n))
        scratch = torch.empty(max(nbytes // 8, 1), dtype=torch.int64, device=dev)
        _, abi = timed(lambda: L.legion_row_offsets(S(), graph.handle, P(rows), n, P(off), P(scratch), nbytes), args.launches)
        record("offsets/abi", abi, their_off, n, 12)
        (t_dst, t_src, t_eid), their_exp = timed(lambda: t_expand(rows, t_off, deg, M), args.launches)
        dst, src = (torch.empty(M, dtype=torch.int32, device=dev) for _ in range(2))
        eid = torch.empty(M, dtype=torch.int64, device=dev)
        _, abi = timed(lambda: L.legion_in_edges(S(), graph.handle, P(rows), n, P(off), M, P(dst), P(src), P(eid)), args.launches)
        same = bool(torch.equal(dst.long(), t_dst) and torch.equal(src, t_src) and torch.equal(eid, t_eid))
        record("expand/abi", abi, their_exp, M, 20, matches_torch=same)
        assert same, "in_edges differs from the torch composition"
        _, abi = timed(lambda: L.legion_in_edges(S(), graph.handle, P(rows), n, P(off), M, P(dst), P(src), None), args.launches)
        record("expand/no-eids/abi", abi, their_exp, M, 12)
        del dst, src, eid, t_dst, t_src, t_eid
        _, whole = timed(lambda: t_expand(rows, *t_offsets(rows), M), args.launches)
        _, ours = timed(lambda: graph.in_edges(rows, return_eids=True), args.launches)
        record("in_edges", ours, whole, M, 20, note="torch's arm is given M; ours reads it back")
        # the block: distinct seeds, n + M within unique_ids' reach
        seeds = torch.unique(rows.long(), sorted=False).int()
        seeds = seeds[torch.randperm(seeds.numel(), device=dev, generator=gen)]
        total = torch.cumsum(indptr[seeds.long() + 1] - indptr[seeds.long()], 0) + torch.arange(1, seeds.numel() + 1, device=dev)
        seeds = seeds[:int((total <= engine.UNIQUE_MAX_IDS).sum().item())].contiguous()
        if seeds.numel():
            blk, ours = timed(lambda: graph.full_neighbor_block(seeds), args.launches)

            def composed():
                o, d = t_offsets(seeds)
                m = int(o[-1].item())
                dd, ss, _ = t_expand(seeds, o, d, m)
                return torch.unique(torch.cat([seeds, ss]), return_inverse=True), dd
            ((t_unique, _), _), theirs = timed(composed, args.launches)
            live = blk[2] >= 0
            same = bool(torch.equal(torch.sort(blk[0]).values, t_unique[t_unique >= 0]) and torch.equal(blk[0][:seeds.numel()], seeds) and
                        torch.equal(blk[0][blk[2][live].long()], col[(indptr[seeds.long()[blk[1].long()]] +
                                                                     (torch.arange(blk[1].numel(), device=dev) - blk[3][blk[1].long()]))][live]))
            record("block", ours, theirs, int(blk[1].numel()), 12, seeds=int(seeds.numel()), distinct=int(blk[0].numel()), matches_torch=same)
            assert same, "full_neighbor_block differs from the torch composition"
        report["lists"][name] = dict(rows=n, slots=M, largest_row=int(deg.max().item()), rows_without_entries=int((deg == 0).sum().item()),
                                     arms=arms)
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
