#!/usr/bin/env python3
"""The rates of per-edge-type sampling (legion_etype_degrees, legion_etype_sample_count, legion_etype_sample_edges) on the bench.py
graph, beside the library's own untyped ops on the same rows, in a fresh process.

    python tools/etype_rate.py [--scale 26] [--edge-factor 16] [--seeds 1048576] [--hub-seeds 65536] [--max-slots 67108864]
                               [--types 4,64] [--launches 7] [--out FILE]

Graph, seed lists (`uniform`, `by-degree`), the cut to --max-slots, event timing and medians are those of tools/topk_rate.py.  An edge's
type is floor(T u^3) of a uniform u drawn once (skewed: half the edges in the first eighth of the types), and every row is sorted by
type.  Arms per list, T, fan-out vector (`ten`: 10 for every type; `mix`: the same with -1 for type 0) and replace:
  etype      count and edges over buffers allocated once, with edge ids and types: the two calls a capturing caller makes
  yardstick  the untyped op at the same total fan-out: legion_row_topk in SAMPLE mode without weights at min(64, 10 T) for `ten`, and
             legion_row_offsets + legion_in_edges for `mix`, whose take-all type is the bulk of its output
and legion_etype_degrees beside the time a plain device copy of the rows' type bytes would take at the rate torch copies etype.
Ratios above 1 are slower than the yardstick.  This sets no pass mark.  bench.py is not involved and is not changed."""
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
    ap.add_argument("--types", type=str, default="4,64")
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
    u = torch.rand(E, device=dev, generator=gen)
    row = torch.repeat_interleave(torch.arange(N, device=dev), indptr[1:] - indptr[:-1], output_size=E)
    report = {"command": " ".join(["python", "tools/etype_rate.py"] + sys.argv[1:]), "device": torch.cuda.get_device_name(0),
              "library": os.path.relpath(lib.LIB_PATH, ROOT), "graph": f"RMAT-{args.scale}, N={N}, E={E}", "launches": args.launches, "types": {}}
    L = lib.load()
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    S = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    SALT = 7

    def cut(rows, limit):
        total = torch.cumsum(indptr[rows.long() + 1] - indptr[rows.long()], 0)
        return rows[:int((total <= limit).sum().item())].contiguous()

    lists = (("uniform", cut(uniform, args.max_slots)), ("by-degree", cut(by_degree, args.max_slots)))
    for T in [int(x) for x in args.types.split(",")]:
        etype = (torch.sort(row * 64 + (u * u * u * T).long().clamp(max=T - 1)).values % 64).to(torch.uint8)
        graph.set_edge_types(etype, T)
        _, copy = timed(lambda: etype.clone(), args.launches)
        copy_rate = E / copy["ms_median"]                             # type bytes per ms, read and written once each
        per_list = {}
        for name, rows in lists:
            n = rows.numel()
            offsets = graph.row_offsets(rows)
            entries = int(offsets[-1].item())
            deg = torch.empty((n, T), dtype=torch.int64, device=dev)
            rc, t_deg = timed(lambda: L.legion_etype_degrees(S(), graph.handle, P(rows), n, P(deg)), args.launches)
            assert rc == 0 and int(deg.sum().item()) == entries
            arms = {"etype_degrees": dict(ours=t_deg, rows_per_second=n / t_deg["ms_median"] * 1e3, stream_ms=entries / copy_rate,
                                          ours_over_stream=t_deg["ms_median"] / (entries / copy_rate))}
            nbytes = int(L.legion_etype_sample_scratch_bytes(n))
            scratch = torch.empty(max(nbytes // 8, 1), dtype=torch.int64, device=dev)
            off = torch.empty(n + 1, dtype=torch.int64, device=dev)
            for fan_name, fan in (("ten", [10] * T), ("mix", [-1] + [10] * (T - 1))):
                c_fan = (ctypes.c_int32 * T)(*fan)
                for replace in (0, 1):
                    assert L.legion_etype_sample_count(S(), graph.handle, P(rows), n, c_fan, replace, P(off), P(scratch), nbytes) == 0
                    M = int(off[n].item())
                    out = [torch.empty(M, dtype=dt, device=dev) for dt in (torch.int32, torch.int32, torch.int64, torch.uint8)]

                    def ours_call():
                        rc = L.legion_etype_sample_count(S(), graph.handle, P(rows), n, c_fan, replace, P(off), P(scratch), nbytes)
                        return rc | L.legion_etype_sample_edges(S(), graph.handle, P(rows), n, c_fan, replace, SALT, P(off), M, *[P(x) for x in out])

                    rc, ours = timed(ours_call, args.launches)
                    assert rc == 0 and bool((out[3] < T).all()) and bool((out[0] >= 0).all())
                    if fan_name == "ten":
                        k = min(64, 10 * T)
                        src, eid, cnt = (torch.empty((n, k), dtype=torch.int32, device=dev), torch.empty((n, k), dtype=torch.int64, device=dev),
                                         torch.empty(n, dtype=torch.int32, device=dev))
                        tb = int(L.legion_row_topk_scratch_bytes(n))
                        ts = torch.empty(tb // 4, dtype=torch.int32, device=dev)
                        what = f"legion_row_topk SAMPLE k={k}"
                        yard = lambda: L.legion_row_topk(S(), graph.handle, P(rows), n, k, 2, None, SALT, P(src), P(eid), P(cnt), P(ts), tb)
                    else:
                        d2, s2, e2 = (torch.empty(entries, dtype=torch.int32, device=dev), torch.empty(entries, dtype=torch.int32, device=dev),
                                      torch.empty(entries, dtype=torch.int64, device=dev))
                        rb = int(L.legion_row_offsets_scratch_bytes(n))
                        rs = torch.empty(max(rb // 8, 1), dtype=torch.int64, device=dev)
                        what = "legion_row_offsets + legion_in_edges"

                        def yard():
                            rc = L.legion_row_offsets(S(), graph.handle, P(rows), n, P(offsets), P(rs), rb)
                            return rc | L.legion_in_edges(S(), graph.handle, P(rows), n, P(offsets), entries, P(d2), P(s2), P(e2))
                    rc, theirs = timed(yard, args.launches)
                    assert rc == 0
                    arms[f"{fan_name} replace={replace}"] = dict(ours=ours, yardstick=theirs, yardstick_op=what, slots=M,
                                                                 slots_per_second=M / ours["ms_median"] * 1e3,
                                                                 ours_over_yardstick=ours["ms_median"] / theirs["ms_median"])
                    print(f"T {T:2d} {name:10s} {fan_name} replace {replace}: {ours['ms_median']:8.3f} ms {M / ours['ms_median'] * 1e-6:7.3f} G slots/s   "
                          f"{what} {theirs['ms_median']:8.3f} ms   ours / yardstick {ours['ms_median'] / theirs['ms_median']:.3f}", flush=True)
                    del out
            print(f"T {T:2d} {name:10s} etype_degrees {t_deg['ms_median']:8.3f} ms; streaming the rows' {entries} type bytes {entries / copy_rate:8.3f} ms",
                  flush=True)
            per_list[name] = dict(rows=n, entries=entries, arms=arms)
        report["types"][str(T)] = per_list
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
