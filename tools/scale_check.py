"""Reads the bench line(s) of an N > 1 run (the driver's SCALE_rNN.json, a file of JSON lines, or stdin) and checks that what ran is
what DESIGN.md section 6 says runs -- so that the first 8-GPU record can be judged the day it exists:

    python tools/scale_check.py SCALE_r05.json            # or:  python bench.py --gpus 2 --full ... | python tools/scale_check.py -

For every line with n_gpus > 1:
  * `collective.world_size_seen_by_all_reduce == n_gpus` and `collective.issued_by` names the library (RCCL issued by liblegion_hip,
    not a torch.distributed fallback);
  * per_rank has n_gpus entries on n_gpus DISTINCT PCI bus ids (one process per physical GPU);
  * headline leg (cache_agg_mode 0): no peer traffic expected -- the xGMI read deltas of the timed regions stay below 1 % of the
    bytes the gathers moved;
  * `striped` / `striped_replica` legs: every rank's measured xGMI read bytes per region within [0.7, 1.5] x the bytes the gather itself
    counted as read from OTHER members' stripes (rows x D x 4; the counters also see adjacency reads and protocol overhead);
  * `striped_bulk` leg: bytes pushed INTO a rank ~ its computed peer bytes of the striped leg (same rows, other transport);
  * the per-leg expectations of DESIGN.md section 6 (table "what N = 8 should cost") as pass / note lines.
Exit code 0 when every hard check holds, 1 otherwise; prints one line per check."""
import json
import sys

XGMI_LINK_GBPS = 153.0          # MI355X_MICROARCH.md: per link and direction; 7 links per GPU on an 8-GPU node
HBM_PEAK_GBPS = 8000.0


def lines_of(path):
    text = sys.stdin.read() if path == "-" else open(path).read()
    out = []
    try:
        obj = json.loads(text)
        cand = obj if isinstance(obj, list) else [obj]
    except ValueError:
        cand = []
        for ln in text.splitlines():
            ln = ln.strip()
            if ln.startswith("{"):
                try:
                    cand.append(json.loads(ln))
                except ValueError:
                    pass

    def walk(o):                      # the driver wraps the bench line ("parsed": {...}) per N
        if isinstance(o, dict):
            if "metric" in o and "n_gpus" in o:
                out.append(o)
            else:
                for v in o.values():
                    walk(v)
        elif isinstance(o, list):
            for v in o:
                walk(v)
    walk(cand)
    return out


class Report:
    def __init__(self):
        self.bad = 0

    def check(self, ok, what):
        print(("PASS  " if ok else "FAIL  ") + what)
        self.bad += 0 if ok else 1

    def note(self, what):
        print("note  " + what)


def check_leg(rep, name, leg, n, D, headline_value=None):
    col = leg.get("collective")
    if col:
        rep.check(col.get("world_size_seen_by_all_reduce") == n, f"{name}: all-reduce saw world size {col.get('world_size_seen_by_all_reduce')} (want {n})")
        rep.check("liblegion" in str(col.get("issued_by", "")), f"{name}: hotness all-reduce issued by {col.get('issued_by')!r} (want the library's RCCL call)")
        ms, nbytes = col.get("hotness_all_reduce_ms"), col.get("hotness_all_reduce_bytes")
        if ms and nbytes:
            # ring / direct reduce-scatter + all-gather: 2 (n-1)/n x bytes per GPU; bounded by one link direction at worst, seven at best
            moved = 2 * (n - 1) / n * nbytes
            lo, hi = moved / (7 * XGMI_LINK_GBPS * 1e6), moved / (XGMI_LINK_GBPS * 1e6)
            rep.note(f"{name}: hotness all-reduce {ms:.1f} ms for {nbytes / 1e9:.2f} GB; link-rate bounds {lo:.1f} .. {hi:.1f} ms"
                     + ("" if ms <= 3 * hi else "  <-- more than 3 x the one-link bound: look at the communicator's topology"))
    pr = leg.get("per_rank") or []
    rep.check(len(pr) == n, f"{name}: per_rank has {len(pr)} entries (want {n})")
    buses = {r.get("pci_bus_id") for r in pr}
    rep.check(len(buses) == n, f"{name}: {len(buses)} distinct PCI bus ids over {len(pr)} ranks (one process per physical GPU)")
    striped = "striped" in str(leg.get("parallelism", leg.get("config", {}).get("parallelism", "")))
    for r in pr:
        tag = f"{name} rank {r.get('rank')}"
        if "xgmi_read_bytes_per_region_measured" in r and "peer_bytes_per_region_computed" in r and striped and not leg.get("peer_gather"):
            m, c = r["xgmi_read_bytes_per_region_measured"], r["peer_bytes_per_region_computed"]
            rep.check(c > 0 and 0.7 <= m / c <= 1.5, f"{tag}: xGMI read {m / 1e9:.2f} GB per region vs {c / 1e9:.2f} GB of rows the gather read from peers (ratio {m / max(c, 1):.2f})")
            links = [b for b in r.get("xgmi_read_bytes_link", []) if b > 0]
            if links:
                rep.note(f"{tag}: {len(links)} links carried reads, max / min = {max(links) / max(min(links), 1):.2f} (striping t % Kg spreads rows evenly: ~1)")
        elif "xgmi_read_bytes" in r and not striped:
            moved = r.get("gather_roofline_frac", 0) * HBM_PEAK_GBPS * 1e9 * r.get("window_s", 0)
            rep.check(moved <= 0 or r["xgmi_read_bytes"] <= 0.01 * moved, f"{tag}: {r['xgmi_read_bytes'] / 1e6:.1f} MB over xGMI in the timed window (replicated caches: none expected)")
        if leg.get("peer_gather") == "bulk" and "bulk" in r:
            b = r["bulk"]
            rep.note(f"{tag}: bulk phase A {b['phase_a_s_per_group'] * 1e3:.2f} ms, phase B {b['phase_b_s_per_group'] * 1e3:.2f} ms, barriers {b['barriers_s_per_group'] * 1e3:.2f} ms per group; "
                     f"{b['bytes_pushed_into_me_per_region'] / 1e9:.2f} GB pushed into it per region, {b['push_GBps_out_of_me']:.0f} GB/s out of it")
    if headline_value and leg.get("value"):
        rep.note(f"{name}: {leg['value'] / 1e9:.2f} G edges/s = {leg['value'] / headline_value:.2f} x the replicated-cache leg of the same run")


def main():
    rep = Report()
    lines = [ln for ln in lines_of(sys.argv[1] if len(sys.argv) > 1 else "-")]
    if not lines:
        print("no bench line found")
        return 1
    by_n = {}
    for ln in lines:
        by_n[ln["n_gpus"]] = ln
    for n in sorted(by_n):
        ln = by_n[n]
        D = int(str(ln["config"]["workload"]).split("[N x ")[1].split("]")[0]) if "[N x " in str(ln["config"].get("workload", "")) else 128
        frac = (ln.get("roofline") or {}).get("frac")
        print(f"---- n_gpus = {n}: {ln['value'] / 1e9:.2f} G edges/s, " +
              (f"gather {frac:.3f} of the HBM peak" if frac is not None else "no roofline (a bench run without --full)"))
        if n == 1:
            continue
        rep.check(ln.get("scaling") == "weak", f"N={n}: scaling declared {ln.get('scaling')!r}")
        check_leg(rep, f"N={n} headline", ln, n, D)
        for leg in ("striped", "striped_replica", "striped_bulk"):
            if isinstance(ln.get(leg), dict):
                check_leg(rep, f"N={n} {leg}", ln[leg], n, D, ln["value"])
            else:
                rep.note(f"N={n}: no `{leg}` leg in the line" + (f" ({ln.get('extra_legs_error')})" if ln.get("extra_legs_error") else ""))
        # DESIGN.md section 6, "what N = 8 should cost": the striped leg is bound by the xGMI ingest of each GPU
        if isinstance(ln.get("striped"), dict) and ln["striped"].get("per_rank"):
            r0 = ln["striped"]["per_rank"][0]
            if "peer_bytes_per_region_computed" in r0 and ln["striped"].get("timed_region"):
                region_s = ln["striped"]["timed_region"]["median_s"]
                ingest = r0["peer_bytes_per_region_computed"] / region_s / 1e9
                peak = (n - 1) * XGMI_LINK_GBPS
                rep.note(f"N={n} striped: rank 0 ingests {ingest:.0f} GB/s of peer rows = {ingest / peak:.2f} of its {n - 1} links' {peak:.0f} GB/s; "
                         f"expected (DESIGN 6): direct peer loads reach 0.5-0.8 of that; below 0.4 the leg is latency-bound (look at striped_bulk)")
    if 1 in by_n:
        base = by_n[1]["value"]
        for n in sorted(by_n):
            if n > 1:
                eff = by_n[n]["value"] / (n * base)
                rep.check(eff >= 0.75, f"N={n}: {by_n[n]['value'] / base:.2f} x the N=1 value = {eff:.2f} per GPU (north_star: >= 6 x at N = 8, i.e. 0.75)")
    print("all hard checks hold" if rep.bad == 0 else f"{rep.bad} hard check(s) failed")
    return 0 if rep.bad == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
