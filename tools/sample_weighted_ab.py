#!/usr/bin/env python3
"""Weighted sampling (GraphStorage.set_edge_weights + MemoryPool / Pipeline weighted=True) off against on, on the bench.py workload,
alternated in fresh child processes.

    python tools/sample_weighted_ab.py [--arms off,on] [--repeats 3] [--timeout 900] [--out FILE] -- <bench.py arguments>

An arm is `off` (bench.py as it is: the uniform draw) or `on`: every GraphStorage gets hash-derived positive float32 weights in
(0, 1] right after it is made, and engine.MemoryPool / Pipeline default to weighted=True.  Each child runs bench.py unchanged;
children alternate the arms in the order given, --repeats times each; every child runs under its own time limit and the first failing
child ends the run.  Every arm runs with --full (for the sampler chain's time).  Pass --no-verify along for the `on` arm: bench.py
verifies against the uniform oracle, which a weighted batch is not.  Per arm the report gives ms/step and the sampler chain's time per
step (median, min, max): edges_per_step over bench.py's sampling_only.edges_per_sec, i.e. the timed region minus the HIP-event time of
every gather, over the step's sampled edges.  The `on` children also time the table build (the second of two calls, HIP events) next
to a device copy of E floats, which moves the same 8 E bytes."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARMS = {"off": False, "on": True}
TABLE_TAG = "weighted_table: "


def child(arm, bench_args):
    sys.path.insert(0, ROOT)
    from legion_amd import engine

    def default(cls, key, value):
        init = cls.__init__

        def patched(self, *a, **kw):
            kw.setdefault(key, value)
            init(self, *a, **kw)
        cls.__init__ = patched

    if ARMS[arm]:
        import torch
        graph_init = engine.GraphStorage.__init__

        def weighted_graph(self, *a, **kw):
            graph_init(self, *a, **kw)
            e = torch.arange(self.edge_num, dtype=torch.int64, device=self.col.device)
            w = (((e * 2654435761) % (1 << 20)) + 1).to(torch.float32) / float(1 << 20)
            del e
            self.set_edge_weights(w)                     # (the first call allocates the table)
            t0, t1, t2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            dst = torch.empty_like(w)
            dst.copy_(w)
            t0.record()
            self.set_edge_weights(w)
            t1.record()
            dst.copy_(w)
            t2.record()
            torch.cuda.synchronize()
            print(TABLE_TAG + json.dumps({"edges": self.edge_num, "rows": self.node_num, "build_ms": t0.elapsed_time(t1),
                                          "copy_8E_bytes_ms": t1.elapsed_time(t2)}), flush=True)
        engine.GraphStorage.__init__ = weighted_graph
        default(engine.MemoryPool, "weighted", True)
        default(engine.Pipeline, "weighted", True)
    sys.argv = [os.path.join(ROOT, "bench.py")] + bench_args
    import runpy
    runpy.run_path(sys.argv[0], run_name="__main__")


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        return child(sys.argv[2], sys.argv[4:] if sys.argv[3:4] == ["--"] else sys.argv[3:])
    argv = sys.argv[1:]
    split = argv.index("--") if "--" in argv else len(argv)
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", type=str, default="off,on", help="off and / or on, comma separated")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=900, help="seconds per child")
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args(argv[:split])
    arms = args.arms.split(",")
    for arm in arms:
        if arm not in ARMS:
            ap.error(f"--arms: {arm!r} is not one of {sorted(ARMS)}")
    bench_args = argv[split + 1:] + ["--full"]
    runs = {arm: [] for arm in arms}
    tables = []
    for rep in range(args.repeats):
        for arm in arms:
            cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", arm, "--"] + bench_args
            p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            line = next((ln for ln in reversed(p.stdout.splitlines()) if ln.startswith("{")), None)
            if p.returncode != 0 or line is None:
                print(f"{arm} run {rep}: exit {p.returncode}\n{p.stdout[-3000:]}", file=sys.stderr)
                return 1
            out = json.loads(line)
            tables += [json.loads(ln[len(TABLE_TAG):]) for ln in p.stdout.splitlines() if ln.startswith(TABLE_TAG)]
            sampler_ms = out["edges_per_step"] / out["sampling_only"]["edges_per_sec"] * 1e3
            runs[arm].append({"ms_per_step": out["ms_per_step"], "sampler_ms_per_step": sampler_ms,
                              "edges_per_step": out["edges_per_step"], "rows_per_step": out["rows_per_step"]})
            print(f"{arm:3s} run {rep}: {out['ms_per_step']:.4f} ms/step, sampler chain {sampler_ms:.4f} ms/step, "
                  f"{out['edges_per_step']:.0f} edges/step", flush=True)
    report = {"command": " ".join(["python", "tools/sample_weighted_ab.py"] + sys.argv[1:])}
    for arm, rs in runs.items():
        ms = [r["ms_per_step"] for r in rs]
        sm = [r["sampler_ms_per_step"] for r in rs]
        report[arm] = {"ms_per_step_median": statistics.median(ms), "ms_per_step_min": min(ms), "ms_per_step_max": max(ms),
                       "sampler_ms_median": statistics.median(sm), "sampler_ms_min": min(sm), "sampler_ms_max": max(sm), "runs": rs}
    f = report[arms[0]]
    report["over_" + arms[0]] = {arm: {"ms_per_step": report[arm]["ms_per_step_median"] / f["ms_per_step_median"],
                                       "sampler_ms": report[arm]["sampler_ms_median"] / f["sampler_ms_median"]}
                                 for arm in arms[1:]}
    if tables:
        report["table_build"] = tables
    text = json.dumps(report, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
