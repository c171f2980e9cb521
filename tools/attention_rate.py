#!/usr/bin/env python3
"""The time of the fused attention aggregation (FeatureStorage.attention: legion_attention_rows) over neighbour lists of an RMAT graph
beside two yardsticks on the same GPU and lists, in a fresh process:
  * the floor: FeatureStorage.aggregate(reduce="sum", weights=), which reads the same rows once and does no dot, no exponential;
  * the composition available without it, in torch: index_select into M x D, einsum for the logits, a segment softmax
    (segment_reduce max and sum) and segment_reduce over the M x H x D weighted rows.

    python tools/attention_rate.py [--scale 24] [--edge-factor 16] [--dim 128] [--heads 1,4] [--rows 65536] [--fanout 25]
                                   [--max-slots 2097152] [--launches 9] [--out FILE]

Graph and event timing are those of tools/link_rate.py (RMAT, seed 20231).  Three lists: the full neighbourhoods of uniform rows and of
the rows of highest degree, each cut to at most --max-slots entries, and --fanout random neighbours of every uniform row (-1 for a row
without any).  float32 and bf16 storage for the fused call and the floor; the composition reads the float32 rows.  The lists are built
once, outside every timing.  Each side runs once untimed, then --launches times: the median counts and min / max are kept beside it.  The
fused result is compared with the composition's.  bench.py is not involved and is not changed."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=24)
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--heads", type=str, default="1,4")
    ap.add_argument("--rows", type=int, default=1 << 16)
    ap.add_argument("--fanout", type=int, default=25)
    ap.add_argument("--max-slots", type=int, default=1 << 21)
    ap.add_argument("--launches", type=int, default=9)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from legion_amd import engine, lib, synth
    from tools.link_rate import timed

    dev = "cuda:0"
    indptr, col = synth.rmat_csr_device(args.scale, args.edge_factor, 20231, dev)
    N, E, D = indptr.numel() - 1, col.numel(), args.dim
    graph = engine.GraphStorage(1, indptr, col)
    gen = torch.Generator(device=dev)
    gen.manual_seed(20231)
    X = torch.randn((N, D), dtype=torch.float32, device=dev, generator=gen)
    report = {"command": " ".join(["python", "tools/attention_rate.py"] + sys.argv[1:]), "device": torch.cuda.get_device_name(0),
              "library": os.path.relpath(lib.LIB_PATH, ROOT), "graph": f"RMAT-{args.scale}, N={N}, E={E}", "dim": D,
              "launches": args.launches, "cases": []}
    deg = indptr[1:] - indptr[:-1]
    uniform = torch.randint(0, N, (args.rows,), dtype=torch.int32, device=dev, generator=gen)
    lists = {}
    for name, rows in (("uniform", uniform), ("hub-heavy", torch.argsort(deg, descending=True)[:args.rows].to(torch.int32))):
        rows = rows[:int((torch.cumsum(deg[rows.long()], 0) <= args.max_slots).sum().item())].contiguous()
        offsets, _, src = graph.in_edges(rows)
        lists[name] = (offsets, src)
    k, d_u = args.fanout, deg[uniform.long()][:, None]
    at = indptr[uniform.long()][:, None] + (torch.rand((args.rows, k), device=dev, generator=gen) * d_u).long()
    drawn = torch.where(d_u > 0, col[at.clamp(max=E - 1)], torch.full_like(at, -1, dtype=torch.int32))
    lists[f"fanout-{k}"] = (torch.arange(args.rows + 1, dtype=torch.int64, device=dev) * k, drawn.reshape(-1).contiguous())

    features = {storage: engine.FeatureStorage(1, X, feature_dtype=storage) for storage in ("float32", "bfloat16")}
    for name, (offsets, src) in lists.items():
        n, M = offsets.numel() - 1, src.numel()
        lengths = offsets[1:] - offsets[:-1]
        seg = torch.repeat_interleave(torch.arange(n, device=dev), lengths)
        dead = (src < 0)[:, None]
        weights = torch.rand((M,), dtype=torch.float32, device=dev, generator=gen)
        for H in [int(h) for h in args.heads.split(",")]:
            q = torch.randn((n, H, D), dtype=torch.float32, device=dev, generator=gen)

            def composed():
                rows = X.index_select(0, src.clamp(min=0).long())
                s = (torch.einsum("mhd,md->mh", q[seg], rows) * D ** -0.5).masked_fill(dead, float("-inf"))
                top = torch.segment_reduce(s, "max", lengths=lengths, unsafe=True)
                p = torch.exp(s - top[seg])
                a = p / torch.segment_reduce(p, "sum", lengths=lengths, unsafe=True)[seg]
                return torch.segment_reduce((a[:, :, None] * rows[:, None, :]).reshape(M, H * D), "sum", lengths=lengths, unsafe=True)

            theirs_out, theirs = timed(composed, args.launches)
            theirs_out = theirs_out.reshape(n, H, D).clone()
            for storage, feature in features.items():
                _, floor = timed(lambda: feature.aggregate(offsets, src, reduce="sum", weights=weights), args.launches)
                ours_out, ours = timed(lambda: feature.attention(offsets, src, queries=q), args.launches)
                some = torch.isfinite(theirs_out).all(dim=2).all(dim=1)                  # (the composition gives NaN without a live entry)
                err = float((ours_out[some] - theirs_out[some]).abs().max().item())
                assert err <= (1e-3 if storage == "float32" else 0.25), err              # (bf16 rows: other logits; plumbing only)
                case = dict(storage=storage, rows=name, heads=H, n=n, M=M, longest=int(lengths.max().item()), ours=ours, floor=floor,
                            composed_float32=theirs, ours_over_floor=ours["ms_median"] / floor["ms_median"],
                            ours_over_composed=ours["ms_median"] / theirs["ms_median"], max_abs_difference=err,
                            ours_bytes=M * (feature.row_bytes + 4) + n * H * D * 8 + n * 8)
                case["ours_gbps"] = case["ours_bytes"] / ours["ms_median"] / 1e6
                report["cases"].append(case)
                print(f"{storage:9s} {name:10s} H {H} n {n:6d} M {M:8d}  ours {ours['ms_median']:7.3f} ms [{ours['ms_min']:.3f}, {ours['ms_max']:.3f}] "
                      f"({case['ours_gbps']:5.0f} GB/s)  floor {floor['ms_median']:7.3f} ms [{floor['ms_min']:.3f}, {floor['ms_max']:.3f}]  "
                      f"torch {theirs['ms_median']:8.3f} ms  ours / floor {case['ours_over_floor']:.2f}  ours / torch "
                      f"{case['ours_over_composed']:.3f}", flush=True)
            del theirs_out, q
            torch.cuda.empty_cache()
    for feature in features.values():
        feature.close()
    graph.close()
    text = json.dumps(report, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
