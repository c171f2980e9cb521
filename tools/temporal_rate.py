#!/usr/bin/env python3
"""The rates of temporal neighbour sampling (legion_temporal_sample_count, legion_temporal_sample_edges) on the bench.py graph, beside
per-edge-type sampling with one type on the same rows, in a fresh process.

    python tools/temporal_rate.py [--scale 26] [--edge-factor 16] [--seeds 1048576] [--hub-seeds 65536] [--max-slots 67108864]
                                  [--launches 7] [--out FILE]

Graph, seed lists (`uniform`, `by-degree`), the cut to --max-slots, event timing and medians are those of tools/etype_rate.py.  An
edge's time is its position in its row (class `sorted`); the same times shuffled inside every row give class `scan`.  A row's bound is
its median time: half its entries are candidates.  Arms per class and list, all at fan-out 10, count and edges over buffers allocated
once, with edge ids and times -- the two calls a capturing caller makes: `uniform replace=0`, `uniform replace=1`, and `last` (sorted
only).  The yardstick, measured in the same run: legion_etype_sample_count + legion_etype_sample_edges with T = 1 at fan-out 10 on the
same rows, the same output shape without a time filter.  Ratios above 1 are slower than the yardstick.  This sets no pass mark.
bench.py is not involved and is not changed."""
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
    ap.add_argument("--max-slots", type=int, default=1 << 26)
    ap.add_argument("--launches", type=int, default=7)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from legion_amd import engine, lib, synth
    from tools.link_rate import timed

    dev = "cuda:0"
    FAN, SALT = 10, 7
    indptr, col = synth.rmat_csr_device(args.scale, args.edge_factor, 20231, dev)
    N, E = indptr.numel() - 1, col.numel()
    graph = engine.GraphStorage(1, indptr, col)
    gen = torch.Generator(device=dev)
    gen.manual_seed(20231)
    uniform = torch.randint(0, N, (args.seeds,), dtype=torch.int32, device=dev, generator=gen)
    edges = torch.randint(0, E, (args.hub_seeds,), dtype=torch.int64, device=dev, generator=gen)
    by_degree = (torch.searchsorted(indptr, edges, right=True) - 1).int()
    deg = indptr[1:] - indptr[:-1]
    row = torch.repeat_interleave(torch.arange(N, device=dev), deg, output_size=E)
    pos = torch.arange(E, device=dev) - indptr[row]                   # the sorted class: a row's times are 0 .. D - 1
    order = torch.argsort((row << 32) | torch.randint(0, 1 << 32, (E,), device=dev, generator=gen))
    shuffled = pos[order]                                             # the scan class: the same times, shuffled inside the row
    del row, order
    graph.set_edge_types(torch.zeros(E, dtype=torch.uint8, device=dev), 1)
    report = {"command": " ".join(["python", "tools/temporal_rate.py"] + sys.argv[1:]), "device": torch.cuda.get_device_name(0),
              "library": os.path.relpath(lib.LIB_PATH, ROOT), "graph": f"RMAT-{args.scale}, N={N}, E={E}", "launches": args.launches,
              "fanout": FAN, "lists": {}}
    L = lib.load()
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    S = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def cut(rows, limit):
        total = torch.cumsum(deg[rows.long()], 0)
        return rows[:int((total <= limit).sum().item())].contiguous()

    for name, rows in (("uniform", cut(uniform, args.max_slots)), ("by-degree", cut(by_degree, args.max_slots))):
        n = rows.numel()
        bounds = (deg[rows.long()] // 2).contiguous()
        entries = int(deg[rows.long()].sum().item())
        nbytes = int(L.legion_temporal_sample_scratch_bytes(n))
        scratch = torch.empty(max(nbytes // 8, 1), dtype=torch.int64, device=dev)
        off, cand = torch.empty(n + 1, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int64, device=dev)
        c_fan = (ctypes.c_int32 * 1)(FAN)
        assert L.legion_etype_sample_count(S(), graph.handle, P(rows), n, c_fan, 0, P(off), P(scratch), nbytes) == 0
        M = int(off[n].item())
        out = [torch.empty(M, dtype=dt, device=dev) for dt in (torch.int32, torch.int32, torch.int64, torch.uint8)]

        def yard():
            rc = L.legion_etype_sample_count(S(), graph.handle, P(rows), n, c_fan, 0, P(off), P(scratch), nbytes)
            return rc | L.legion_etype_sample_edges(S(), graph.handle, P(rows), n, c_fan, 0, SALT, P(off), M, *[P(x) for x in out])

        rc, theirs = timed(yard, args.launches)
        assert rc == 0
        del out
        arms = {"yardstick": dict(op="legion_etype_sample_count + _edges, T=1, fan-out 10, replace=0", slots=M, **theirs)}
        for cls, times in (("sorted", pos), ("scan", shuffled)):
            graph.set_edge_times(times)
            assert graph.edge_times_sorted == (cls == "sorted")
            for arm, strategy, replace in (("uniform replace=0", 0, 0), ("uniform replace=1", 0, 1), ("last", 1, 0))[:3 if cls == "sorted" else 2]:
                head = (graph.handle, P(rows), P(bounds), n, FAN, strategy, replace)
                assert L.legion_temporal_sample_count(S(), *head, P(cand), P(off), P(scratch), nbytes) == 0
                M = int(off[n].item())
                out = [torch.empty(M, dtype=dt, device=dev) for dt in (torch.int32, torch.int32, torch.int64, torch.int64)]

                def ours_call():
                    rc = L.legion_temporal_sample_count(S(), *head, P(cand), P(off), P(scratch), nbytes)
                    return rc | L.legion_temporal_sample_edges(S(), *head, SALT, P(cand), P(off), M, *[P(x) for x in out])

                rc, ours = timed(ours_call, args.launches)
                assert rc == 0 and bool((cand == bounds).all()) and bool((out[3] < bounds[out[0].long()]).all())
                ratio = ours["ms_median"] / theirs["ms_median"]
                arms[f"{cls} {arm}"] = dict(ours=ours, slots=M, slots_per_second=M / ours["ms_median"] * 1e3, ours_over_yardstick=ratio)
                print(f"{name:10s} {cls:6s} {arm:18s}: {ours['ms_median']:8.3f} ms {M / ours['ms_median'] * 1e-6:7.3f} G slots/s   yardstick "
                      f"{theirs['ms_median']:8.3f} ms   ours / yardstick {ratio:.3f}", flush=True)
                del out
        report["lists"][name] = dict(rows=n, entries=entries, time_bytes=8 * entries, arms=arms)
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
