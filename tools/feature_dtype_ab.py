#!/usr/bin/env python3
"""Feature storage dtype x feature output dtype on the bench.py workload, alternated in fresh child processes.

    python tools/feature_dtype_ab.py [--arms f32:f32,bf16:f32] [--repeats 3] [--timeout 900] [--rows 0] [--out FILE] -- <bench.py arguments>

An arm is storage:out, each f32 or bf16: the dtype the feature table and caches hold (engine.FeatureStorage feature_dtype) and
the dtype of the rows handed over (engine.MemoryPool / Pipeline feature_out_dtype).  Each child runs bench.py unchanged, with
those constructors defaulting to the arm's dtypes (f32:f32 = bench.py as it is).  Children alternate the arms in the order
given, --repeats times each; every child runs under its own time limit and the first failing child ends the run.  bench.py's
own verification compares float32 rows with the float32 table, so every arm runs with --full --no-verify (the bf16 rows are covered
by tests/test_gpu_feature_bf16.py and tests/test_gpu_feature_out_bf16.py).  Per arm the report gives ms/step (median, min,
max), the last-hop gather's average launch time, and its algorithmic GB/s and fraction of the 8 TB/s peak at the arm's bytes
per row (P = D rounded up to 8): f32:f32 8 D + 8, bf16:f32 2 P + 4 D + 8, bf16:bf16 2 P + 2 D + 8, f32:bf16 6 D + 8.
--rows R: children of arms with a bf16 side run with LEGION_GATHER_ROWS=R (the gather's tile size; 0 = the library's choice)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_GBPS = 8000.0


DTYPES = {"f32": "float32", "bf16": "bfloat16"}


def child(arm, bench_args):
    sys.path.insert(0, ROOT)
    from legion_amd import engine
    storage, out = (DTYPES[x] for x in arm.split(":"))

    def default(cls, key, value):
        init = cls.__init__

        def patched(self, *a, **kw):
            kw.setdefault(key, value)
            init(self, *a, **kw)
        cls.__init__ = patched

    default(engine.FeatureStorage, "feature_dtype", storage)
    default(engine.MemoryPool, "feature_out_dtype", out)
    default(engine.Pipeline, "feature_out_dtype", out)
    sys.argv = [os.path.join(ROOT, "bench.py")] + bench_args
    import runpy
    runpy.run_path(sys.argv[0], run_name="__main__")


def bytes_per_row(arm, D):
    storage, out = arm.split(":")
    return (4 * D if storage == "f32" else 2 * ((D + 7) // 8 * 8)) + (4 * D if out == "f32" else 2 * D) + 8


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        return child(sys.argv[2], sys.argv[4:] if sys.argv[3:4] == ["--"] else sys.argv[3:])
    argv = sys.argv[1:]
    split = argv.index("--") if "--" in argv else len(argv)
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", type=str, default="f32:f32,bf16:f32", help="storage:out,... (f32 or bf16 each)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=900, help="seconds per child")
    ap.add_argument("--rows", type=int, default=0)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args(argv[:split])
    arms = args.arms.split(",")
    for arm in arms:
        if len(arm.split(":")) != 2 or any(x not in DTYPES for x in arm.split(":")):
            ap.error(f"--arms: {arm!r} is not storage:out with f32 or bf16 on each side")
    bench_args = argv[split + 1:] + ["--full", "--no-verify"]
    D = 128
    for i, a in enumerate(bench_args):
        if a == "--dim":
            D = int(bench_args[i + 1])
    runs = {arm: [] for arm in arms}
    for rep in range(args.repeats):
        for dtype in arms:
            env = dict(os.environ)
            if dtype != "f32:f32" and args.rows:
                env["LEGION_GATHER_ROWS"] = str(args.rows)
            cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", dtype, "--"] + bench_args
            p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            line = next((ln for ln in reversed(p.stdout.splitlines()) if ln.startswith("{")), None)
            if p.returncode != 0 or line is None:
                print(f"{dtype} run {rep}: exit {p.returncode}\n{p.stdout[-3000:]}", file=sys.stderr)
                return 1
            out = json.loads(line)
            roof = out["roofline"]
            us = roof["avg_launch_us"]
            gbps = roof["rows_per_launch"] * bytes_per_row(dtype, D) / (us * 1e-6) / 1e9 if us > 0 else 0.0
            runs[dtype].append({"ms_per_step": out["ms_per_step"], "last_gather_us": us, "gather_gbps": gbps,
                                "rows_per_launch": roof["rows_per_launch"]})
            print(f"{dtype:9s} run {rep}: {out['ms_per_step']:.4f} ms/step, last gather {us:.1f} us, {gbps:.0f} GB/s "
                  f"({gbps / PEAK_GBPS:.3f} of peak)", flush=True)
    report = {"command": " ".join(["python", "tools/feature_dtype_ab.py"] + sys.argv[1:]), "D": D, "peak_gbps": PEAK_GBPS,
              "bytes_per_row": {k: bytes_per_row(k, D) for k in runs}, "bf16_gather_rows": args.rows or "library default"}
    for dtype, rs in runs.items():
        ms = [r["ms_per_step"] for r in rs]
        us = [r["last_gather_us"] for r in rs]
        g = [r["gather_gbps"] for r in rs]
        report[dtype] = {"ms_per_step_median": statistics.median(ms), "ms_per_step_min": min(ms), "ms_per_step_max": max(ms),
                         "last_gather_us_median": statistics.median(us), "last_gather_us_min": min(us), "last_gather_us_max": max(us),
                         "gather_gbps_median": statistics.median(g), "gather_frac_of_peak_median": statistics.median(g) / PEAK_GBPS,
                         "runs": rs}
    f = report[arms[0]]
    report["over_" + arms[0]] = {arm: {"ms_per_step": report[arm]["ms_per_step_median"] / f["ms_per_step_median"],
                                       "last_gather_us": report[arm]["last_gather_us_median"] / f["last_gather_us_median"]}
                                 for arm in arms[1:]}
    text = json.dumps(report, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
