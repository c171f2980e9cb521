#!/usr/bin/env python3
"""The rates of the vertex set and of induced subgraphs (legion_node_set_build, legion_node_set_lookup, legion_induced_count,
legion_induced_edges, GraphStorage.node_subgraph) on the bench.py graph, each beside its composition from torch's library kernels on the
same GPU and inputs, in a fresh process.

    python tools/induced_rate.py [--scale 26] [--edge-factor 16] [--nodes 1048576] [--hub-seeds 65536] [--lookups 16777216]
                                 [--max-slots 268435456] [--launches 7] [--out FILE]

Graph, event timing and medians are those of tools/in_edges_rate.py and tools/labor_rate.py.  Two node lists, each used as the rows and
as the set: `uniform`, --nodes vertices drawn uniformly and made distinct (nearly every slot is rejected), and `by-degree`, the distinct
rows of in_edges_rate's by-degree list (hub-heavy), each cut to the longest prefix with at most --max-slots entries.  The yardstick is
the composition a caller writes today: in_edges' own output (legion_in_edges), an N-entry int32 position map filled by a scatter,
pos[src], the mask, nonzero, three gathers (two without edge ids), and searchsorted for the row pointers.  Arms per list:
  build          legion_node_set_build                               | the position map: a fill of N entries and a scatter
  lookup         legion_node_set_lookup of --lookups uniform ids     | a gather from the position map
  edges/abi      build + count + edges, with edge ids, cap = K       | the composition without searchsorted
  edges-no-eids  the same without edge ids                           | the same with two gathers
  count+edges    the two calls alone over a set built before (record only: torch has no counterpart without its map)
  node_subgraph  the Python method: set, offsets, three reads        | GraphStorage.in_edges, the composition, searchsorted
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
    ap.add_argument("--nodes", type=int, default=1 << 20)
    ap.add_argument("--hub-seeds", type=int, default=1 << 16)
    ap.add_argument("--lookups", type=int, default=1 << 24)
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
    uniform = torch.randint(0, N, (args.nodes,), dtype=torch.int32, device=dev, generator=gen)
    edges = torch.randint(0, E, (args.hub_seeds,), dtype=torch.int64, device=dev, generator=gen)
    by_degree = (torch.searchsorted(indptr, edges, right=True) - 1).int()
    asked = torch.randint(0, N, (args.lookups,), dtype=torch.int32, device=dev, generator=gen)
    report = {"command": " ".join(["python", "tools/induced_rate.py"] + sys.argv[1:]), "device": torch.cuda.get_device_name(0),
              "library": os.path.relpath(lib.LIB_PATH, ROOT), "graph": f"RMAT-{args.scale}, N={N}, E={E}", "launches": args.launches,
              "lookups": args.lookups, "lists": {}}
    L = lib.load()
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    S = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def distinct(rows):
        """The distinct values of rows in order of first appearance."""
        values, inverse = torch.unique(rows, return_inverse=True)
        first = torch.full((values.numel(),), rows.numel(), dtype=torch.int64, device=dev)
        first.scatter_reduce_(0, inverse, torch.arange(rows.numel(), device=dev), reduce="amin")
        return values[torch.argsort(first)].contiguous()

    def cut(rows, limit):
        """The longest prefix of rows whose entries are at most limit."""
        total = torch.cumsum(indptr[rows.long() + 1] - indptr[rows.long()], 0)
        return rows[:int((total <= limit).sum().item())].contiguous()

    for name, nodes in (("uniform", cut(distinct(uniform), args.max_slots)), ("by-degree", cut(distinct(by_degree), args.max_slots))):
        k = n = nodes.numel()
        rows = nodes
        off = graph.row_offsets(rows)
        M = int(off[-1].item())
        arms = {}

        def record(arm, ours, theirs, items, unit, **more):
            out = dict(ours=ours, items=items, unit=unit, per_second=items / ours["ms_median"] * 1e3, **more)
            line = f"{name:10s} {arm:14s} {ours['ms_median']:9.3f} ms  {out['per_second'] * 1e-9:7.3f} G {unit}/s"
            if theirs is not None:
                out.update(torch=theirs, ours_over_torch=ours["ms_median"] / theirs["ms_median"])
                line += f"   torch {theirs['ms_median']:9.3f} ms   ours / torch {out['ours_over_torch']:.3f}"
            arms[arm] = out
            print(line, flush=True)

        # ---- the set -------------------------------------------------------------------------------------------------------------
        set_bytes = int(L.legion_node_set_bytes(k))
        table = torch.empty(set_bytes // 4, dtype=torch.int32, device=dev)
        count_distinct = torch.zeros(1, dtype=torch.int32, device=dev)
        order = torch.arange(k, dtype=torch.int32, device=dev)

        def t_map():
            pos = torch.full((N,), -1, dtype=torch.int32, device=dev)
            pos[nodes.long()] = order
            return pos

        c_build = lambda: L.legion_node_set_build(S(), P(nodes), k, P(table), set_bytes, P(count_distinct))
        pos_map, theirs = timed(t_map, args.launches)
        _, ours = timed(c_build, args.launches)
        assert int(count_distinct.item()) == k, "legion_node_set_build counts other distinct nodes than there are"
        record("build", ours, theirs, k, "nodes", table_bytes=set_bytes, map_bytes=4 * N)
        local = torch.empty(args.lookups, dtype=torch.int32, device=dev)
        c_lookup = lambda: L.legion_node_set_lookup(S(), P(table), set_bytes, k, P(asked), args.lookups, P(local))
        t_local, theirs = timed(lambda: pos_map[asked.long()], args.launches)
        c_lookup()
        same = bool(torch.equal(local, t_local))
        assert same, "legion_node_set_lookup differs from the position map"
        _, ours = timed(c_lookup, args.launches)
        record("lookup", ours, theirs, args.lookups, "ids", members=int((t_local >= 0).sum().item()), matches_torch=same)
        del local, t_local

        # ---- the edges -----------------------------------------------------------------------------------------------------------
        e_dst, e_src = (torch.empty(M, dtype=torch.int32, device=dev) for _ in range(2))
        e_eid = torch.empty(M, dtype=torch.int64, device=dev)

        def t_edges(with_eids, pointers=False):
            assert L.legion_in_edges(S(), graph.handle, P(rows), n, P(off), M, P(e_dst), P(e_src), P(e_eid) if with_eids else None) == 0
            pos = t_map()
            loc = torch.where(e_src >= 0, pos[e_src.clamp(min=0).long()], -1)      # a dead entry is -1: no index
            at = torch.nonzero(loc >= 0).reshape(-1)
            out = [e_dst[at], loc[at]] + ([e_eid[at]] if with_eids else [])
            if pointers:
                out.append(torch.searchsorted(out[0], torch.arange(k + 1, dtype=torch.int32, device=dev)))
            return out

        nbytes = int(L.legion_induced_scratch_bytes(M))
        scratch = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        want = t_edges(True)
        K = int(want[0].numel())
        dst, src = (torch.empty(max(K, 1), dtype=torch.int32, device=dev) for _ in range(2))
        eid = torch.empty(max(K, 1), dtype=torch.int64, device=dev)
        c_count = lambda: L.legion_induced_count(S(), graph.handle, P(rows), n, P(off), M, P(table), set_bytes, k, P(count), P(scratch), nbytes)
        c_edges = lambda e: L.legion_induced_edges(S(), graph.handle, P(rows), n, P(off), M, P(table), set_bytes, k, P(scratch), nbytes, K, P(dst),
                                                   P(src), P(e))
        assert (c_build(), c_count(), c_edges(eid)) == (0, 0, 0)
        same = bool(int(count.item()) == K and torch.equal(dst[:K], want[0]) and torch.equal(src[:K], want[1]) and torch.equal(eid[:K], want[2]))
        assert same, "legion_induced_count / _edges differ from the torch composition"
        del want
        for arm, e in (("edges/abi", eid), ("edges-no-eids", None)):
            _, theirs = timed(lambda: t_edges(e is not None), args.launches)
            _, ours = timed(lambda: (c_build(), c_count(), c_edges(e)), args.launches)
            record(arm, ours, theirs, M, "slots", kept=K, matches_torch=same)
        _, ours = timed(lambda: (c_count(), c_edges(eid)), args.launches)
        record("count+edges", ours, None, M, "slots", kept=K)
        del dst, src, eid, scratch

        # ---- node_subgraph end to end ----------------------------------------------------------------------------------------------
        def t_subgraph():
            _, d, s, e = graph.in_edges(rows, return_eids=True)
            pos = t_map()
            loc = torch.where(s >= 0, pos[s.clamp(min=0).long()], -1)
            at = torch.nonzero(loc >= 0).reshape(-1)
            kept = d[at]
            return torch.searchsorted(kept, torch.arange(k + 1, dtype=torch.int32, device=dev)), loc[at], e[at]

        want = t_subgraph()
        got = graph.node_subgraph(nodes, return_eids=True)
        same = bool(all(torch.equal(a, b) for a, b in zip(got, want)))
        assert same, "node_subgraph differs from the torch composition"
        del want, got
        _, theirs = timed(t_subgraph, args.launches)
        _, ours = timed(lambda: graph.node_subgraph(nodes, return_eids=True), args.launches)
        record("node_subgraph", ours, theirs, M, "slots", kept=K, matches_torch=same)
        del e_dst, e_src, e_eid, pos_map
        torch.cuda.empty_cache()
        report["lists"][name] = dict(nodes=k, slots=M, kept=K, arms=arms)
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
