#!/usr/bin/env python3
"""The time of the sparse row update (FeatureStorage.update_rows: legion_row_update) beside the composition available without it on the
same GPU and arrays: torch.unique(return_inverse, return_counts), index_add_ into a [U, D] buffer, and the same Adagrad step in torch
over the rows of the unique ids, in a fresh process.

    python tools/update_rate.py [--scale 24] [--edge-factor 16] [--dim 128] [--ids 1048576,4194304] [--launches 7] [--out FILE]

The table has N = 2^scale rows.  Two id lists: uniform (random vertices, few duplicates) and degree-proportional (the column entries of
random edges of the bench.py RMAT graph, seed 20231, as walk contexts are: many duplicates).  Event timing is tools/link_rate.py's:
each side runs once untimed, then --launches times; the median counts.  Every timed call is one more optimizer step on the same
table and state, for both sides alike.  The two sides start from equal tables; after their first step their Adagrad states (g^2) are compared
within the bound of two float32 sums in any order.  Bytes: the update reads m x D gradients and reads and writes U rows of the table and of the
state; its sort moves 2 x passes x 8 m bytes.  LEGION_HIP_LIB=<another build> times that build.  bench.py is not involved and is not
changed."""
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
    ap.add_argument("--ids", type=str, default="1048576,4194304")
    ap.add_argument("--launches", type=int, default=7)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from legion_amd import engine, lib, synth
    from tools.link_rate import timed

    dev = "cuda:0"
    indptr, col = synth.rmat_csr_device(args.scale, args.edge_factor, 20231, dev)
    N, E, D = indptr.numel() - 1, col.numel(), args.dim
    del indptr
    gen = torch.Generator(device=dev)
    gen.manual_seed(20231)
    X = torch.randn((N, D), dtype=torch.float32, device=dev, generator=gen)
    lr, eps = 0.01, 1e-10
    report = {"command": " ".join(["python", "tools/update_rate.py"] + sys.argv[1:]), "device": torch.cuda.get_device_name(0),
              "library": os.path.relpath(lib.LIB_PATH, ROOT), "table": f"N={N}, D={D}, float32", "graph": f"RMAT-{args.scale}, E={E}",
              "optimizer": "adagrad, combine=mean", "launches": args.launches, "cases": []}

    for m in [int(x) for x in args.ids.split(",")]:
        lists = {"uniform": torch.randint(0, N, (m,), dtype=torch.int32, device=dev, generator=gen),
                 "degree-proportional": col[torch.randint(0, E, (m,), device=dev, generator=gen)].to(torch.int32)}
        grads = torch.randn((m, D), dtype=torch.float32, device=dev, generator=gen)
        for name, ids in lists.items():
            ours_table, theirs_table = X.clone(), X.clone()
            feature = engine.FeatureStorage(1, ours_table)
            state = {}
            theirs_state = torch.zeros((N, D), dtype=torch.float32, device=dev)

            def composed():
                uniq, inverse, counts = torch.unique(ids, return_inverse=True, return_counts=True)
                g = torch.zeros((uniq.numel(), D), dtype=torch.float32, device=dev).index_add_(0, inverse, grads)
                g /= counts[:, None]
                rows = uniq.long()
                s = theirs_state[rows] + g * g
                theirs_state[rows] = s
                theirs_table[rows] -= lr * g / (s.sqrt() + eps)
                return uniq

            def ours():
                return feature.update_rows(ids, grads, optimizer="adagrad", lr=lr, combine="mean", state=state, eps=eps)

            # the first step of each side, from equal tables: compared, then the timed steps go on from there
            uniq = composed()
            ours()
            torch.cuda.synchronize()
            rows = uniq.long()
            counts = torch.bincount(ids.long(), minlength=N)[rows]
            mass = torch.zeros((N, D), dtype=torch.float32, device=dev).index_add_(0, ids.long(), grads.abs())[rows]
            # each side's g is a float32 sum of `count` terms over the count: they differ by at most dg, their squares s by
            # 2 (|g| + dg) dg and the roundings of s.  (The step itself is no yardstick: w moves by lr g / (|g| + eps), which flips
            # with the sign of a g that is all rounding.)
            dg = 2 * (counts[:, None] + 2) * 2.0 ** -24 * mass.double() / counts[:, None]
            want = theirs_state[rows].double()
            err = (state["state1"][rows].double() - want).abs()
            bound = 2 * (want.sqrt() + dg) * dg + 2.0 ** -22 * want
            assert bool((err <= bound).all()), f"the two sides' sums of squares differ by more than two float32 sums may: {float((err - bound).max())}"
            del dg, want, mass, err, bound
            _, theirs = timed(composed, args.launches)
            _, mine = timed(ours, args.launches)
            U, passes = int(uniq.numel()), -(-N.bit_length() // 8)
            case = dict(m=m, ids=name, distinct=U, most_duplicates=int(counts.max().item()), ours=mine, composed=theirs,
                        ours_over_composed=mine["ms_median"] / theirs["ms_median"],
                        ours_bytes=m * (D * 4 + 4) + 4 * U * D * 4 + 2 * passes * 8 * m)
            case["ours_gbps"] = case["ours_bytes"] / mine["ms_median"] / 1e6
            report["cases"].append(case)
            print(f"m {m:8d} {name:20s} distinct {U:8d}  ours {mine['ms_median']:8.3f} ms ({case['ours_gbps']:6.0f} GB/s)   "
                  f"unique + index_add_ + torch step {theirs['ms_median']:8.3f} ms   ours / composed {case['ours_over_composed']:.3f}", flush=True)
            feature.close()
            del ours_table, theirs_table, theirs_state, state, feature
            torch.cuda.empty_cache()
    text = json.dumps(report, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
