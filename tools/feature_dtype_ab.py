#!/usr/bin/env python3
"""float32 vs bfloat16 feature storage on the bench.py workload, alternated in fresh child processes.

    python tools/feature_dtype_ab.py [--repeats 3] [--timeout 900] [--rows 0] [--out FILE] -- <bench.py arguments>

Each child runs bench.py unchanged, with engine.FeatureStorage defaulting to the dtype under test (float32 = bench.py as it
is).  Children alternate float32, bfloat16, float32, ... --repeats times each; every child runs under its own time limit
and the first failing child ends the run.  bench.py's own verification compares rows with the float32 table, so both dtypes
run with --no-verify (the bf16 rows are covered by tests/test_gpu_feature_bf16.py).  Per dtype the report gives ms/step
(median, min, max), the last-hop gather's average launch time, and its algorithmic GB/s and fraction of the 8 TB/s peak at
8 D + 8 bytes per float32 row and 2 P + 4 D + 8 per bf16 row (P = D rounded up to 8).  --rows R: bf16 children run with
LEGION_GATHER_ROWS=R (the gather's tile size; 0 = the library's choice)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_GBPS = 8000.0


def child(dtype, bench_args):
    sys.path.insert(0, ROOT)
    from legion_amd import engine
    init = engine.FeatureStorage.__init__

    def patched(self, *a, feature_dtype=dtype, **kw):
        init(self, *a, feature_dtype=feature_dtype, **kw)

    engine.FeatureStorage.__init__ = patched
    sys.argv = [os.path.join(ROOT, "bench.py")] + bench_args
    import runpy
    runpy.run_path(sys.argv[0], run_name="__main__")


def bytes_per_row(dtype, D):
    return 8 * D + 8 if dtype == "float32" else 2 * ((D + 7) // 8 * 8) + 4 * D + 8


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        return child(sys.argv[2], sys.argv[4:] if sys.argv[3:4] == ["--"] else sys.argv[3:])
    argv = sys.argv[1:]
    split = argv.index("--") if "--" in argv else len(argv)
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=900, help="seconds per child")
    ap.add_argument("--rows", type=int, default=0)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args(argv[:split])
    bench_args = argv[split + 1:] + ["--no-verify"]
    D = 128
    for i, a in enumerate(bench_args):
        if a == "--dim":
            D = int(bench_args[i + 1])
    runs = {"float32": [], "bfloat16": []}
    for rep in range(args.repeats):
        for dtype in ("float32", "bfloat16"):
            env = dict(os.environ)
            if dtype == "bfloat16" and args.rows:
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
    f, b = report["float32"], report["bfloat16"]
    report["bf16_over_f32"] = {"ms_per_step": b["ms_per_step_median"] / f["ms_per_step_median"],
                               "last_gather_us": b["last_gather_us_median"] / f["last_gather_us_median"]}
    text = json.dumps(report, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
