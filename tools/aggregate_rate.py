#!/usr/bin/env python3
"""The time of the fused neighbour aggregation (FeatureStorage.aggregate: legion_aggregate_rows) over full neighbourhoods of the bench.py
graph beside the composition available without it on the same GPU and arrays: legion_gather_rows_fmt into an M x D float32 buffer, then
torch.segment_reduce over it, in a fresh process.

    python tools/aggregate_rate.py [--scale 26] [--edge-factor 16] [--dim 128] [--rows 65536] [--max-slots 16777216] [--launches 7]
                                   [--out FILE]

Graph and event timing are those of tools/link_rate.py (RMAT, seed 20231).  Two row lists: uniform (random vertices) and hub-heavy (the
vertices of highest degree), each cut so that its neighbourhoods hold at most --max-slots entries; float32 and bf16 storage; reduce =
mean.  The edge list (row_offsets + in_edges) is built once, outside both timings.  Each side runs once untimed, then --launches times;
the median counts.  The fused result is compared with the composition's within the bound of a float32 sum in any order.  Bytes: the fused
op reads M stored rows and writes n x D; the composition also writes and reads M x D float32.  LEGION_HIP_LIB=<another build> times that
build.  bench.py is not involved and is not changed."""
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
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--rows", type=int, default=1 << 16)
    ap.add_argument("--max-slots", type=int, default=1 << 24)
    ap.add_argument("--launches", type=int, default=7)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from legion_amd import engine, lib, synth
    from tools.link_rate import timed

    dev = "cuda:0"
    L = lib.load()
    indptr, col = synth.rmat_csr_device(args.scale, args.edge_factor, 20231, dev)
    N, E, D = indptr.numel() - 1, col.numel(), args.dim
    graph = engine.GraphStorage(1, indptr, col)
    gen = torch.Generator(device=dev)
    gen.manual_seed(20231)
    X = torch.randn((N, D), dtype=torch.float32, device=dev, generator=gen)
    report = {"command": " ".join(["python", "tools/aggregate_rate.py"] + sys.argv[1:]), "device": torch.cuda.get_device_name(0),
              "library": os.path.relpath(lib.LIB_PATH, ROOT), "graph": f"RMAT-{args.scale}, N={N}, E={E}", "dim": D,
              "launches": args.launches, "cases": []}
    deg = indptr[1:] - indptr[:-1]
    lists = {"uniform": torch.randint(0, N, (args.rows,), dtype=torch.int32, device=dev, generator=gen),
             "hub-heavy": torch.argsort(deg, descending=True)[:args.rows].to(torch.int32)}
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    for storage in ("float32", "bfloat16"):
        feature = engine.FeatureStorage(1, X, feature_dtype=storage)
        table = L.legion_feature_table(feature.handle)
        tables = torch.tensor([table], dtype=torch.int64, device=dev)
        for name, rows in lists.items():
            total = torch.cumsum(deg[rows.long()], 0)
            rows = rows[:int((total <= args.max_slots).sum().item())].contiguous()
            offsets, _, src = graph.in_edges(rows)
            n, M = rows.numel(), src.numel()
            lengths = offsets[1:] - offsets[:-1]
            buf = torch.zeros((M, D), dtype=torch.float32, device=dev)        # (the gather leaves the row of a dead entry as it is)
            cidx = torch.empty((M,), dtype=torch.int32, device=dev)
            rng = torch.tensor([0, M], dtype=torch.int32, device=dev)

            def composed():
                s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
                rc = L.legion_gather_rows_fmt(s, engine.FEATURE_DTYPES[storage], 0, table, P(tables), None, 0, D, N, P(src), None, P(cidx),
                                              P(rng), P(buf), M, M, 0, 1, None)
                assert rc == 0
                return torch.segment_reduce(buf, "mean", lengths=lengths, initial=0.0, unsafe=True)

            theirs_out, theirs = timed(composed, args.launches)
            theirs_out = theirs_out.clone()
            ours_out, ours = timed(lambda: feature.aggregate(offsets, src, reduce="mean"), args.launches)
            # dead column entries are skipped by both sides' sums but counted by the composition's mean: compare the sums
            live = torch.segment_reduce((src >= 0).float(), "sum", lengths=lengths, initial=0.0)[:, None]
            mass = torch.segment_reduce(buf.abs(), "sum", lengths=lengths, initial=0.0)
            err = (ours_out.double() * live - theirs_out.double() * lengths[:, None]).abs()
            bound = 2 * (lengths[:, None] + 2) * 2.0 ** -24 * mass.double()
            assert bool((err <= bound).all()), "the fused result differs from the composition's by more than two float32 sums may"
            row_bytes = feature.row_bytes
            case = dict(storage=storage, rows=name, n=n, M=M, longest=int(lengths.max().item()), ours=ours, composed=theirs,
                        ours_over_composed=ours["ms_median"] / theirs["ms_median"],
                        ours_bytes=M * (row_bytes + 4) + n * (D * 4 + 8), composed_bytes=M * (row_bytes + 4 + 8 * D) + n * (D * 4 + 8))
            case["ours_gbps"] = case["ours_bytes"] / ours["ms_median"] / 1e6
            case["composed_gbps"] = case["composed_bytes"] / theirs["ms_median"] / 1e6
            report["cases"].append(case)
            print(f"{storage:9s} {name:10s} n {n:6d} M {M:9d}  ours {ours['ms_median']:8.3f} ms ({case['ours_gbps']:6.0f} GB/s)   "
                  f"gather + segment_reduce {theirs['ms_median']:8.3f} ms   ours / composed {case['ours_over_composed']:.3f}", flush=True)
            del buf, cidx, theirs_out, ours_out, mass, err, bound
        feature.close()
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
