#!/usr/bin/env python3
"""The time of the backward pass of the fused attention aggregation (FeatureStorage.attention_backward:
legion_attention_rows_backward) over neighbour lists of an RMAT graph beside two yardsticks on the same GPU and lists, in a fresh
process:
  * the forward: FeatureStorage.attention(return_lse=True) at the same shape, which reads the same rows once;
  * the composition available without it, in torch: the forward of tools/attention_rate.py (index_select into M x D, einsum, a segment
    softmax, segment_reduce) under autograd, and torch.autograd.grad for the queries and the gathered rows.  Forward and backward are
    timed together and the forward alone; the backward's share is the difference of the medians.

    python tools/attention_backward_rate.py [--scale 24] [--edge-factor 16] [--dim 128] [--heads 1,4] [--rows 65536] [--fanout 25]
                                            [--max-slots 2097152] [--launches 9] [--out FILE]

Graph, lists and event timing are those of tools/attention_rate.py (RMAT, seed 20231; float32 rows).  Each side runs once untimed,
then --launches times: the median counts and min / max are kept beside it.  The fused gradients are compared with autograd's.
bench.py is not involved and is not changed."""
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
    report = {"command": " ".join(["python", "tools/attention_backward_rate.py"] + sys.argv[1:]), "device": torch.cuda.get_device_name(0),
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

    feature = engine.FeatureStorage(1, X)
    for name, (offsets, src) in lists.items():
        n, M = offsets.numel() - 1, src.numel()
        lengths = offsets[1:] - offsets[:-1]
        seg = torch.repeat_interleave(torch.arange(n, device=dev), lengths)
        dead = (src < 0)[:, None]
        some = torch.segment_reduce((~dead[:, 0]).float(), "sum", lengths=lengths, unsafe=True) > 0      # (the composition gives NaN without a live entry)
        for H in [int(h) for h in args.heads.split(",")]:
            q = torch.randn((n, H, D), dtype=torch.float32, device=dev, generator=gen)
            dO = torch.randn((n, H, D), dtype=torch.float32, device=dev, generator=gen) * some[:, None, None]

            def composed(backward):
                qa = q.detach().requires_grad_(backward)
                rows = X.index_select(0, src.clamp(min=0).long()).requires_grad_(backward)
                s = (torch.einsum("mhd,md->mh", qa[seg], rows) * D ** -0.5).masked_fill(dead, float("-inf"))
                top = torch.segment_reduce(s.detach(), "max", lengths=lengths, unsafe=True)
                p = torch.exp(s - torch.where(some[:, None], top, 0.0)[seg])
                a = p / torch.segment_reduce(p, "sum", lengths=lengths, unsafe=True).clamp_min(1e-30)[seg]
                out = torch.segment_reduce((a[:, :, None] * rows[:, None, :]).reshape(M, H * D), "sum", lengths=lengths, unsafe=True)
                return torch.autograd.grad(out, (qa, rows), dO.reshape(n, H * D)) if backward else out

            (their_q, their_r), both = timed(lambda: composed(True), args.launches)
            _, forward_only = timed(lambda: composed(False), args.launches)
            (out, lse), forward = timed(lambda: feature.attention(offsets, src, queries=q, return_lse=True), args.launches)
            (our_q, _, our_r), ours = timed(lambda: feature.attention_backward(offsets, src, dO, out, lse, queries=q), args.launches)
            err = max(float((our_q - their_q).abs().max().item()), float((our_r - their_r).abs().max().item()))
            assert err <= 1e-2, err                                                     # (plumbing only: tests hold the bound)
            torch_ms = both["ms_median"] - forward_only["ms_median"]
            case = dict(rows=name, heads=H, n=n, M=M, longest=int(lengths.max().item()), ours=ours, forward=forward, composed_forward_and_backward=both,
                        composed_forward=forward_only, composed_backward_ms=torch_ms, ours_over_forward=ours["ms_median"] / forward["ms_median"],
                        ours_over_composed_backward=ours["ms_median"] / torch_ms, max_abs_difference=err,
                        ours_bytes=M * (feature.row_bytes + 4 + 4 * D + 4 * H) + n * H * D * 16 + n * 8)      # rows, ids, grad_rows, grad_bias; q, dO, out, grad_queries
            case["ours_gbps"] = case["ours_bytes"] / ours["ms_median"] / 1e6
            report["cases"].append(case)
            print(f"{name:10s} H {H} n {n:6d} M {M:8d}  backward {ours['ms_median']:7.3f} ms [{ours['ms_min']:.3f}, {ours['ms_max']:.3f}] "
                  f"({case['ours_gbps']:5.0f} GB/s)  forward {forward['ms_median']:7.3f} ms [{forward['ms_min']:.3f}, {forward['ms_max']:.3f}]  "
                  f"torch backward {torch_ms:8.3f} ms  backward / forward {case['ours_over_forward']:.2f}  backward / torch "
                  f"{case['ours_over_composed_backward']:.4f}", flush=True)
            del their_q, their_r, our_q, our_r, q, dO, out, lse
            torch.cuda.empty_cache()
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
