#!/usr/bin/env python3
"""The time of the reverse CSR (GraphStorage.reverse: legion_graph_build_reverse) on the bench.py graph beside its composition from
torch's library kernels on the same GPU and arrays, and of out_edges beside the torch expansion over the same reverse arrays, in a fresh
process.

    python tools/reverse_rate.py [--scale 26] [--edge-factor 16] [--builds 7] [--nodes 65536] [--max-slots 268435456] [--out FILE]

Graph and event timing are those of tools/link_rate.py (RMAT, seed 20231).  A build is timed on a fresh graph object, --builds times after
one untimed; the median counts.  The torch composition: the live column entries, a stable torch.sort of them with its indices, bincount
and cumsum for the row pointers, repeat_interleave over the forward degrees for the rows.  Every hand-written result is compared with it
and must be equal.  Per-kernel times (count, scan, scatter, each class of the sort) are the kernel statistics of a profiler run of this
script: the build's kernels are the ones named reverse_* and scan_*.  LEGION_HIP_LIB=<another build> times that build.  bench.py is not
involved and is not changed."""
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
    ap.add_argument("--builds", type=int, default=7)
    ap.add_argument("--nodes", type=int, default=1 << 16)
    ap.add_argument("--max-slots", type=int, default=1 << 28)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from legion_amd import engine, lib, synth
    from tools.link_rate import timed

    dev = "cuda:0"
    indptr, col = synth.rmat_csr_device(args.scale, args.edge_factor, 20231, dev)
    N, E = indptr.numel() - 1, col.numel()
    report = {"command": " ".join(["python", "tools/reverse_rate.py"] + sys.argv[1:]), "device": torch.cuda.get_device_name(0),
              "library": os.path.relpath(lib.LIB_PATH, ROOT), "graph": f"RMAT-{args.scale}, N={N}, E={E}", "builds": args.builds}

    def t_reverse():
        e = torch.nonzero((col >= 0) & (col < N)).reshape(-1)
        u, order = torch.sort(col[e], stable=True)
        reid = e[order]
        rindptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(torch.bincount(u, minlength=N), 0)])
        rows = torch.repeat_interleave(torch.arange(N, dtype=torch.int32, device=dev), indptr[1:] - indptr[:-1], output_size=E)
        return rindptr, rows[reid], reid

    want, theirs = timed(t_reverse, args.builds)
    want = [x.clone() for x in want]
    torch.cuda.empty_cache()
    ms, graph = [], None
    for i in range(args.builds + 1):                  # the first build untimed
        if graph is not None:
            graph.close()
        graph = engine.GraphStorage(1, indptr, col)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        rev = graph.reverse()
        t1.record()
        torch.cuda.synchronize()
        if i > 0:
            ms.append(t0.elapsed_time(t1))
        same = bool(torch.equal(rev.indptr, want[0]) and torch.equal(rev.col, want[1]) and torch.equal(rev.eids, want[2]))
        assert same, "the reverse differs from the torch composition"
    ours = {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "ms": ms}
    lengths = want[0][1:] - want[0][:-1]
    report["reverse"] = dict(ours=ours, torch=theirs, ours_over_torch=ours["ms_median"] / theirs["ms_median"], matches_torch=True,
                             live_entries=int(want[2].numel()), longest_row=int(lengths.max().item()),
                             rows_wave=int(((lengths >= 2) & (lengths <= 64)).sum().item()),
                             rows_tile=int(((lengths > 64) & (lengths <= 4096)).sum().item()), rows_long=int((lengths > 4096).sum().item()),
                             entries_long=int(lengths[lengths > 4096].sum().item()))
    print(f"reverse   ours {ours['ms_median']:9.3f} ms   torch {theirs['ms_median']:9.3f} ms   ours / torch {report['reverse']['ours_over_torch']:.3f}",
          flush=True)

    # out_edges against the torch expansion over the same reverse arrays
    gen = torch.Generator(device=dev)
    gen.manual_seed(20231)
    nodes = torch.randint(0, N, (args.nodes,), dtype=torch.int32, device=dev, generator=gen)
    total = torch.cumsum(lengths[nodes.long()], 0)
    nodes = nodes[:int((total <= args.max_slots).sum().item())].contiguous()
    rindptr, rcol, reid = want

    def t_out_edges():
        r = nodes.long()
        deg = rindptr[r + 1] - rindptr[r]
        offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(deg, 0)])
        M = int(offsets[-1].item())
        src = torch.repeat_interleave(torch.arange(nodes.numel(), device=dev), deg, output_size=M)
        at = rindptr[r[src]] + (torch.arange(M, device=dev) - offsets[src])
        return src, rcol[at], reid[at]

    (t_src, t_dst, t_eid), theirs = timed(t_out_edges, args.builds)
    (src, dst, eid), ours = timed(lambda: graph.out_edges(nodes, return_eids=True), args.builds)
    same = bool(torch.equal(src.long(), t_src) and torch.equal(dst, t_dst) and torch.equal(eid, t_eid))
    assert same, "out_edges differs from the torch expansion"
    report["out_edges"] = dict(ours=ours, torch=theirs, ours_over_torch=ours["ms_median"] / theirs["ms_median"], matches_torch=same,
                               nodes=int(nodes.numel()), edges=int(eid.numel()))
    print(f"out_edges ours {ours['ms_median']:9.3f} ms   torch {theirs['ms_median']:9.3f} ms   ours / torch {report['out_edges']['ours_over_torch']:.3f}",
          flush=True)
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
