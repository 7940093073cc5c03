#!/usr/bin/env python
"""A/B of two builds of libpps.so in one sitting, in the protocol of DESIGN.md section 8 1f / 1g / 1i: the parent commit's library against this
tree's, alternating, every GPU step a process of its own under its own time limit; the first step that fails, faults or runs out of time ends
the run (nothing more is started on the GPU).

  python tools/first_panel_ab.py PARENT_LIB OUTDIR [--parts trace,timeline,harness,headline,full] [--runs 8] [--full-runs 3]

  trace     PPS_TRACE=1 tools/trace_c2.py per library: the per-front phase stamps of k_band_factor_lean_trace (stderr of the library)
  timeline  rocprofv3 --kernel-trace of tools/timeline_c2.py, two passes per library: median, mean and range of the four kernels of a launch
            set and the launch-set period (factor start to factor start), per pass and pooled
  harness   rocprofv3 --kernel-trace of the one-front harness k_debug_front<NT, false, 4> (no counters, no other tracing): the six fronts of
            1g's table, 110 launches each, median us
  headline  `--runs` alternating runs per library of bench.py --gpus 1 --steps 20 --warmup 3
  full      `--full-runs` alternating runs per library of the same with --full --no-cpu-baseline and PPS_BENCH_MULTI_G=8,128
  c5        (only when named) `--runs` alternating runs per library with --full --no-cpu-baseline --no-c3 --no-concurrent and
            PPS_BENCH_MULTI_G=8: more samples of the C5 frame loop, a host-bound line on which identical libraries differ by 2 %

Every value of every run goes to OUTDIR/ab.json (raw result lines included), the timelines to OUTDIR/timeline_<build>.txt.
  python tools/first_panel_ab.py --harness-child          (the harness workload itself, run under rocprofv3 by the above)
"""
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = [(18, 0, 2), (13, 19, 2), (15, 33, 3), (27, 21, 3), (27, 24, 4), (47, 16, 4)]      # (p, b, tile rows): the fronts of 1g's table
HARNESS_REPS = 110
KERNELS = ("k_band_factor_all", "k_band_solve_all", "k_trial_lin", "k_hblocks2")


def harness_child():
    sys.path.insert(0, ROOT)
    import numpy as np
    import pop_up_slam_amd as P
    for p, b, nt in HARNESS:
        rng = np.random.default_rng(0); f = p + b
        M = rng.standard_normal((f, f + 20)); H = M @ M.T + f * np.eye(f)
        full = np.zeros((f + 1, f + 1)); full[:f, :f] = H; full[f, :f] = rng.standard_normal(f); full[f, f] = 7.0
        tri = np.concatenate([full[i, :i + 1] for i in range(f + 1)])
        for _ in range(HARNESS_REPS):
            P.debug_front_factor(tri, p, b, tiles=nt, width=4)
    print("ok")


class Failed(Exception):
    pass


def run(cmd, env, limit, log):
    """one step: its own process, its own time limit; anything but exit status 0 ends the whole run"""
    e = dict(os.environ); e.update(env)
    try:
        r = subprocess.run(cmd, env=e, cwd=ROOT, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        raise Failed("time limit of %d s: %s" % (limit, " ".join(cmd)))
    with open(log, "a") as f:
        f.write("$ %s   [%s]\n%s\n%s\n" % (" ".join(cmd), " ".join("%s=%s" % kv for kv in env.items()), r.stdout[-4000:], r.stderr[-8000:]))
    if r.returncode != 0:
        raise Failed("exit status %d: %s\n%s" % (r.returncode, " ".join(cmd), r.stderr[-1500:]))
    return r


def stat(v):
    return {"n": len(v), "median": statistics.median(v), "mean": statistics.fmean(v), "min": min(v), "max": max(v)} if v else {"n": 0}


def kernel_rows(d):
    f = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))[-1]
    rows = [(r["Kernel_Name"].split("(")[0].replace("pps::", "").replace("void ", ""), int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(open(f))]
    rows.sort(key=lambda r: r[1])
    return rows


def rocprof(cmd, env, limit, log):
    with tempfile.TemporaryDirectory() as td:
        run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", td, "--"] + cmd, env, limit, log)
        return kernel_rows(td)


def timeline_pass(env, log):
    rows = rocprof([sys.executable, "tools/timeline_c2.py", "run"], env, 240, log)
    out = {k: [(e - s) / 1e3 for n, s, e in rows if n == k] for k in KERNELS}
    st = [s for n, s, e in rows if n == "k_band_factor_all"]
    out["period"] = [(b - a) / 1e3 for a, b in zip(st, st[1:])]
    out["dispatches"] = len(rows)
    return out


def harness_pass(env, log):
    rows = [r for r in rocprof([sys.executable, "tools/first_panel_ab.py", "--harness-child"], env, 240, log) if r[0].startswith("k_debug_front")]
    if len(rows) != len(HARNESS) * HARNESS_REPS:
        raise Failed("harness: %d launches in the trace" % len(rows))
    return {"p%d_b%d_nt%d" % s: stat([(e - a) / 1e3 for _, a, e in rows[i * HARNESS_REPS:(i + 1) * HARNESS_REPS]]) for i, s in enumerate(HARNESS)}


def bench_line(env, extra, limit, log):
    r = run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "3"] + extra, env, limit, log)
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def main():
    if sys.argv[1] == "--harness-child":
        return harness_child()
    parent, outdir = os.path.abspath(sys.argv[1]), sys.argv[2]
    opt = dict(zip(sys.argv[3::2], sys.argv[4::2]))
    parts = opt.get("--parts", "trace,timeline,harness,headline,full").split(",")
    runs, full_runs = int(opt.get("--runs", 8)), int(opt.get("--full-runs", 3))
    os.makedirs(outdir, exist_ok=True)
    log = os.path.join(outdir, "steps.log")
    envs = {"parent": {"PPS_LIB": parent}, "this": {}}
    res = {"parts": parts, "failed": None}
    order = lambda k: ("parent", "this") if k % 2 == 0 else ("this", "parent")          # parent/this/this/parent ...

    def save():
        with open(os.path.join(outdir, "ab.json"), "w") as f:
            json.dump(res, f, indent=1)
    try:
        if "trace" in parts:
            for b in ("parent", "this"):
                r = run([sys.executable, "tools/trace_c2.py", "c2"], dict(envs[b], PPS_TRACE="1"), 180, log)
                with open(os.path.join(outdir, "phase_trace_%s.txt" % b), "w") as f:
                    f.write(r.stdout + r.stderr)
        if "timeline" in parts:
            tl = {"parent": [], "this": []}
            for k in range(2):
                for b in order(k):
                    tl[b].append(timeline_pass(envs[b], log))
                    res["kernel_timeline_us"] = {b_: {"passes": [{k_: stat(v) for k_, v in p.items() if k_ != "dispatches"} for p in tl[b_]],
                                                      "pooled": {k_: stat([x for p in tl[b_] for x in p[k_]]) for k_ in KERNELS + ("period",)},
                                                      "raw_k_band_factor_all": [p["k_band_factor_all"] for p in tl[b_]]} for b_ in tl if tl[b_]}
                    save()
            for b in tl:
                with open(os.path.join(outdir, "timeline_%s.txt" % b), "w") as f:
                    f.write("build: %s   (rocprofv3 --kernel-trace of tools/timeline_c2.py: two LM solves of the C2 graph per pass, %d passes, %d kernel dispatches)\n"
                            % (b, len(tl[b]), sum(p["dispatches"] for p in tl[b])))
                    for i, p in enumerate(tl[b] + [{k_: [x for q in tl[b] for x in q[k_]] for k_ in KERNELS + ("period",)}]):
                        f.write("pass %d\n" % (i + 1) if i < len(tl[b]) else "pooled\n")
                        for k_ in KERNELS + ("period",):
                            s = stat(p[k_])
                            f.write("%-36s n %4d   mean %7.2f us   median %7.2f   min %7.2f   max %7.2f\n"
                                    % ("launch-set period (factor to factor)" if k_ == "period" else k_, s["n"], s["mean"], s["median"], s["min"], s["max"]))
        if "harness" in parts:
            res["harness_us"] = {}
            for b in ("parent", "this"):
                res["harness_us"][b] = harness_pass(envs[b], log); save()
        if "headline" in parts:
            res["headline_runs"] = {"parent": [], "this": []}
            for k in range(runs):
                for b in order(k):
                    res["headline_runs"][b].append(bench_line(envs[b], [], 240, log)); save()
        if "full" in parts:
            res["full_runs"] = {"parent": [], "this": []}
            for k in range(full_runs):
                for b in order(k):
                    res["full_runs"][b].append(bench_line(dict(envs[b], PPS_BENCH_MULTI_G="8,128"), ["--full", "--no-cpu-baseline"], 600, log)); save()
        if "c5" in parts:
            res["c5_runs"] = {"parent": [], "this": []}
            for k in range(runs):
                for b in order(k):
                    res["c5_runs"][b].append(bench_line(dict(envs[b], PPS_BENCH_MULTI_G="8"), ["--full", "--no-cpu-baseline", "--no-c3", "--no-concurrent"], 400, log)); save()
    except Failed as e:
        res["failed"] = str(e); save()
        print("FAILED:", e)
        return 1
    save()
    print("ok:", ",".join(parts))
    return 0


if __name__ == "__main__":
    sys.exit(main())
