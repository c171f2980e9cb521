#!/usr/bin/env python3
"""The rates of seed-edge exclusion (legion_reverse_edge_ids, legion_edge_set_build, legion_edge_filter_count / _edges) on the bench.py
graph, each beside its composition from torch's library kernels on the same GPU and inputs, in a fresh process.

    python tools/exclude_rate.py [--scale 26] [--edge-factor 16] [--eids 1048576] [--edges 1048576] [--launches 7] [--out FILE]

Graph, event timing and medians are those of tools/link_rate.py: the median of --launches timed calls after one untimed call.
  reverse ids   on the REVERSE of the bench graph, whose rows are sorted, so that both search paths run on one graph: via 0 (its own
                rows), via 1 (the reverse of the reverse), find_edges on the same ids (the op's own first half), and the torch
                composition it replaces -- the packed (row, col) keys of all E' entries, an E'-sized int64 temporary, and two
                searchsorted -- timed with the keys built per call and with the keys built before.  On the bench graph itself
                (unsorted rows) via 1 alone.
  filter        legion_edge_set_build + count + edges at a batch's sizes, 1 024 and 8 000 seed edges with their reverses against
                --edges sampled edges | torch.isin plus three masked selects; and count + edges alone over a set built before.
Every hand-written result is compared with the torch composition before it is timed and must be equal.  bench.py is not involved and is
not changed."""
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
    ap.add_argument("--eids", type=int, default=1 << 20)
    ap.add_argument("--edges", type=int, default=1 << 20)
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
    rev = graph.reverse()
    assert rev.rows_sorted()
    rev.reverse()
    E1 = rev.edge_num
    gen = torch.Generator(device=dev)
    gen.manual_seed(20231)
    L = lib.load()
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    S = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    report = {"command": " ".join(["python", "tools/exclude_rate.py"] + sys.argv[1:]), "device": torch.cuda.get_device_name(0),
              "library": os.path.relpath(lib.LIB_PATH, ROOT), "graph": f"RMAT-{args.scale}, N={N}, E={E}, live {E1}", "launches": args.launches,
              "bench_graph_rows_sorted": bool(graph.rows_sorted()), "arms": {}}

    def record(arm, ours, theirs, items, unit, **more):
        out = dict(ours=ours, items=items, unit=unit, per_second=items / ours["ms_median"] * 1e3, **more)
        line = f"{arm:28s} {ours['ms_median']:9.3f} ms  {out['per_second'] * 1e-9:7.3f} G {unit}/s"
        if theirs is not None:
            out.update(torch=theirs, ours_over_torch=ours["ms_median"] / theirs["ms_median"])
            line += f"   torch {theirs['ms_median']:9.3f} ms   ours / torch {out['ours_over_torch']:.3f}"
        report["arms"][arm] = out
        print(line, flush=True)

    # ---- reverse ids -------------------------------------------------------------------------------------------------------------
    n = args.eids
    eids = torch.randint(0, E1, (n,), dtype=torch.int64, device=dev, generator=gen)
    out = torch.empty(n, dtype=torch.int64, device=dev)
    row, c = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)

    def t_keys():
        rows = torch.repeat_interleave(torch.arange(N, dtype=torch.int64, device=dev), rev.indptr[1:] - rev.indptr[:-1])
        return rows * N + rev.col                                  # ascending: the rows are sorted

    def t_reverse(keys=None):
        keys = t_keys() if keys is None else keys
        v = torch.searchsorted(rev.indptr, eids, right=True) - 1
        want = rev.col[eids].long() * N + v
        pos = torch.searchsorted(keys, want).clamp(max=E1 - 1)
        return torch.where(keys[pos] == want, pos, -1)

    keys = t_keys()
    want = t_reverse(keys)
    for via in (0, 1):
        assert L.legion_reverse_edge_ids(S(), rev.handle, P(eids), n, via, P(out)) == 0
        assert torch.equal(out, want), f"legion_reverse_edge_ids via {via} differs from the torch composition"
    found = int((want >= 0).sum().item())
    _, theirs_all = timed(lambda: t_reverse(), args.launches)
    _, theirs_pre = timed(lambda: t_reverse(keys), args.launches)
    _, fe = timed(lambda: L.legion_find_edges(S(), rev.handle, P(eids), n, P(row), P(c)), args.launches)
    record("find_edges (first half)", fe, None, n, "ids")
    for via in (0, 1):
        _, ours = timed(lambda: L.legion_reverse_edge_ids(S(), rev.handle, P(eids), n, via, P(out)), args.launches)
        record(f"reverse_ids via {via}", ours, theirs_all, n, "ids", found=found, torch_keys_prebuilt=theirs_pre, torch_temporary_bytes=8 * E1,
               over_find_edges=ours["ms_median"] / fe["ms_median"], over_torch_keys_prebuilt=ours["ms_median"] / theirs_pre["ms_median"])
    del keys, want
    eids0 = torch.randint(0, E, (n,), dtype=torch.int64, device=dev, generator=gen)
    _, ours = timed(lambda: L.legion_reverse_edge_ids(S(), graph.handle, P(eids0), n, 1, P(out)), args.launches)
    record("reverse_ids via 1, bench graph", ours, None, n, "ids", found=int((out >= 0).sum().item()))
    torch.cuda.empty_cache()

    # ---- the filter --------------------------------------------------------------------------------------------------------------
    m = args.edges
    dst = torch.sort(torch.randint(0, max(m // 10, 1), (m,), dtype=torch.int32, device=dev, generator=gen)).values.contiguous()
    src = torch.randint(0, N, (m,), dtype=torch.int32, device=dev, generator=gen)
    eid = torch.randint(0, E, (m,), dtype=torch.int64, device=dev, generator=gen)
    nbytes = int(L.legion_edge_filter_scratch_bytes(m))
    scratch = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    o = [torch.empty(m, dtype=t, device=dev) for t in (torch.int32, torch.int32, torch.int64)]
    for seeds in (1024, 8000):
        seed_eids = eid[torch.randperm(m, device=dev, generator=gen)[:seeds]]      # seed edges that do occur among the sampled ones
        members = torch.cat([seed_eids, graph.reverse_edge_ids(seed_eids)]).contiguous()
        k = members.numel()
        set_bytes = int(L.legion_edge_set_bytes(k))
        table = torch.empty(set_bytes // 8, dtype=torch.int64, device=dev)

        def t_filter():
            keep = ~torch.isin(eid, members[members >= 0])
            return dst[keep], src[keep], eid[keep]

        head = (P(dst), P(src), P(eid), m, P(table), set_bytes, k)
        c_build = lambda: L.legion_edge_set_build(S(), P(members), k, P(table), set_bytes)
        c_count = lambda: L.legion_edge_filter_count(S(), *head, P(count), P(scratch), nbytes)
        c_edges = lambda: L.legion_edge_filter_edges(S(), *head, P(scratch), nbytes, m, P(o[0]), P(o[1]), P(o[2]))
        want = t_filter()
        assert (c_build(), c_count(), c_edges()) == (0, 0, 0)
        K = int(count.item())
        assert K == want[0].numel() and all(torch.equal(a[:K], b) for a, b in zip(o, want)), "the filter differs from the torch composition"
        _, theirs = timed(t_filter, args.launches)
        _, ours = timed(lambda: (c_build(), c_count(), c_edges()), args.launches)
        record(f"filter with build, {seeds} seeds", ours, theirs, m, "edges", set_ids=k, kept=K)
        _, ours = timed(lambda: (c_count(), c_edges()), args.launches)
        record(f"count + edges, {seeds} seeds", ours, None, m, "edges", set_ids=k, kept=K)
        _, ours = timed(c_build, args.launches)
        record(f"set build, {seeds} seeds", ours, None, k, "ids")
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
