#!/usr/bin/env python
"""bench.py -- headline benchmark of the plane-SLAM graph solve on MI355X.

  python bench.py --gpus N --steps K --warmup W

One "step" = one full `pps_batch_optimize` (Levenberg-Marquardt to convergence, the reference's
Slam::batch_optimization) of the BASELINE.json config-2 graph -- synthetic corridor, 1 000 SE3 poses,
200 plane landmarks, 5 000 plane edges + 999 odometry edges + priors -- restarted from its initial
(dead-reckoned) estimate, which is restored from a device-resident snapshot.  Graph, measurements
and state are resident in HBM before the timed region starts.  value = LM iterations / second over
all ranks (one independent graph per GPU, no collective: SURVEY.md section 8(e)); ms_per_step = wall
milliseconds of one timed step.

A plain run sets up, warms up, times the --steps steps and prints the headline line.  --dump-outputs DIR
also writes what the last timed step computed (per graph: the optimised poses n x 7 and planes n x 4,
the final chi2 and the LM iteration count, float64) as DIR/<name>.npy.  Everything else is measured only
with --full; the objects it adds to the JSON line include:
  roofline      K1 (Jacobian sweep) inside the timed solves: algorithmic bytes per launch (392 B per
                plane edge, 840 B per odometry edge) / mean launch duration from HIP
                event pairs recorded on the solver's stream.  The single C2 graph (2.8 MB) lives in
                cache, so `roofline_batched` repeats the sweep over replicated edges (> 256 MB).
  cpu_baseline  the CPU oracle (oracle/pps_oracle.c, a "port": the reference itself cannot be built
                here) solving the same graph on one host core.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

B_PLANE_EDGE = 392   # 152 B read + 240 B written per pose-plane edge linearisation
B_ODO_EDGE = 840     # 216 B read + 624 B written per odometry edge
B_TRIAL_EDGE = 176   # K4: one edge's residual at a trial point
HBM_PEAK_GBS = 8000.0


N_SIMD, CLOCK_HZ = 1024, 2.4e9          # MI355X: 256 CUs x 4 SIMDs, 2.4 GHz peak engine clock (/opt/skills/guides/MI355X_MICROARCH.md)
K1_SOURCES = ("pps_k1.hip", "pps_k1_lanes.hip", "pps_k1_body.h", "pps_lin.h", "pps_geom.h")


def k1_source_hash():
    """hash of the sources that define the K1 kernels: a PMC record (profiles/r*_pmc_k1_sweep.json) is only quoted by a build
    of exactly these sources"""
    import hashlib
    h = hashlib.sha1()
    for name in K1_SOURCES:
        with open(os.path.join(ROOT, "pop_up_slam_amd", "csrc", name), "rb") as f:
            h.update(name.encode()); h.update(f.read())
    return h.hexdigest()[:16]


def load_pmc():
    """the newest PMC record of the batched K1 sweep whose source hash equals this tree's; ({}, reason) when there is none"""
    import glob
    want = k1_source_hash()
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_k1_sweep.json")), reverse=True)
    for path in files:
        try:
            with open(path) as f:
                js = json.load(f)
        except (OSError, ValueError):
            continue
        if js.get("k1_source_hash") == want:
            return js, os.path.basename(path)
    return {}, "no PMC record in profiles/ was taken on these K1 sources (hash %s): traffic not quoted" % want


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(spec, budget_s=12.0, optimised=False, threads=1, min_runs=5, max_runs=9):
    """Reference-faithful CPU path (numeric Jacobians, re-ordering every factorisation, 1 thread); `optimised`: the same
    solver with closed-form Jacobians and the ordering computed once (what a tuned CPU build of the reference could do);
    `threads` > 1: its Jacobian sweep on that many OpenMP threads (the sparse Cholesky stays sequential, as CHOLMOD's
    simplicial code is).  SURVEY 8(d): the process is pinned (one core for the 1-thread variants), the value is the MEDIAN
    over >= 5 full solves."""
    from oracle import oracle_py as O
    saved = None
    try:
        saved = os.sched_getaffinity(0)
        cores = sorted(saved)
        os.sched_setaffinity(0, set(cores[-threads:]) if threads > 1 else {cores[-1]})
    except (AttributeError, OSError):
        saved = None
    rates, iters, secs, chi2 = [], 0, 0.0, None
    phases = np.zeros(4)
    try:
        while len(rates) < min_runs or (secs < budget_s and len(rates) < max_runs):
            kw = dict(analytic=1, cache_ordering=1, threads=threads) if optimised else {}
            o = O.OracleGraph(**kw)
            spec.replay(o)
            t0 = time.perf_counter()
            it = o.batch_optimize()
            dt = time.perf_counter() - t0
            rates.append(it / dt)
            secs += dt
            iters += it
            chi2 = o.chi2()
            phases += o.timers()
    finally:
        if saved is not None:
            os.sched_setaffinity(0, saved)
    runs = len(rates)
    return {
        "value": float(np.median(rates)), "unit": "LM iters/s", "cores": threads, "kind": "port",
        "sample": f"median of {runs} full LM solves of the same C2 graph ({iters} iterations, {secs:.1f} s), oracle/pps_oracle.c -O3, "
                  + ("closed-form Jacobians + ordering computed once" + (f", Jacobian sweep on {threads} OpenMP threads" if threads > 1 else "")
                     if optimised else "numeric Jacobians + per-call re-ordering as the reference")
                  + (", process pinned" if saved is not None else ", pinning unavailable"),
        "min": float(np.min(rates)), "max": float(np.max(rates)), "runs": runs,
        "final_chi2": chi2, "host_cores_total": os.cpu_count(), "host_cpu": cpu_model(),
        "phase_split_s": {"linearise": phases[0] / runs, "factor_solve": phases[1] / runs,
                          "retract_chi2": phases[2] / runs, "ordering": phases[3] / runs},
    }


# C4 TIMING set: independently seeded C2-size graphs.  Seed 42 is BASELINE config 2; the others are the first generator
# seeds whose LM run is as short as seed 42's (55-79 trials to chi2 = 0.023) -- a balanced unit of work for a scaling
# curve.  PARITY on C4 is judged on SURVEY's seeds 100-107 (tests/test_gpu_solve.py::test_c4_survey_seeds_against_the_oracle),
# most of which zig-zag for 100-500 trials and half of which are chaotic even between two CPU builds of the oracle.
C4_SEEDS = [42, 135, 110, 143, 225, 154, 169, 185]


def multi_graph_bench(P, synth, device, mode, args, spec0, flops_per_factorisation, k1_bytes, torch, k3_bytes=0, g_list=None):
    """G in {1, 8, 64, 128} (g_list) C4 timing graphs (seeds cycle through C4_SEEDS) solved by pps_multi_optimize from their initial
    estimates; per graph the chi2 / iteration count must equal the single-handle solve of the same seed."""
    specs = {sd: synth.corridor(seed=sd) for sd in C4_SEEDS}
    single = {}
    for sd, sp in specs.items():
        g1 = P.Graph(device=device, jacobian_mode=mode); sp.replay(g1)
        single[sd] = (g1.batch_optimize(), g1.chi2()); g1.close()
    res = {}
    for G in (g_list or tuple(int(x) for x in os.environ.get("PPS_BENCH_MULTI_G", "1,8,64,128").split(","))):
        gs = []
        for k in range(G):
            gk = P.Graph(device=device, jacobian_mode=mode)
            specs[rank_seed(k)].replay(gk); gk.save_state()
            gs.append(gk)
        mm = P.Multi(gs)
        its, st = mm.optimize()                                          # analysis + upload + first solve: outside the clock
        same = all((int(its[k]), gs[k].chi2()) == single[rank_seed(k)] for k in range(G))
        same_iters = all(int(its[k]) == single[rank_seed(k)][0] for k in range(G))
        max_rel = max(abs(gs[k].chi2() - single[rank_seed(k)][1]) / single[rank_seed(k)][1] for k in range(G))
        reps = max(2, args.steps // (5 if G >= 64 else 4))
        torch.cuda.synchronize()
        t1 = time.perf_counter(); iters = 0
        for _ in range(reps):
            mm.restore_state()
            its, st = mm.optimize()
            iters += int(its.sum())
        torch.cuda.synchronize()
        el = time.perf_counter() - t1
        mm.set_profiling(1)
        mm.restore_state()
        mm.optimize()
        ph = mm.phase_times(); mm.set_profiling(0)
        ent = {"graphs": G, "graphs_per_sec": G * reps / el, "value": iters / el, "unit": "LM iters/s", "rounds": mm.rounds(),
               "timed_region": "pps_multi_restore_state (every graph back at its initial estimate, one launch) + pps_multi_optimize, %d repetitions" % reps,
               "ms_per_batch_solve": 1e3 * el / reps, "bit_identical_to_single_handle": bool(same), "same_iteration_counts": bool(same_iters),
               "max_rel_chi2_diff_vs_single_handle": max_rel,
               "device_seconds_per_phase": {k: ph[k] for k in ("linearize", "assemble", "factor", "backsolve", "trial")},
               "relinearisations": ph["n_relinearized"], "factorisations": ph["n_solves"]}
        if ph["factor"] > 0:
            tf = flops_per_factorisation * ph["n_solves"] / ph["factor"] / 1e12
            ent["roofline_k3"] = {"bound": "mfma", "kernel": "kb_level_factor2/3/4" if ph["level_form"] else "kb_band_factor", "achieved": tf, "peak": 78.6, "unit": "TFLOP/s", "frac": tf / 78.6,
                                  "us_per_factorisation_amortised": 1e6 * ph["factor"] / max(1, ph["n_solves"])}
            if k3_bytes:
                # a batch streams every graph's H entries, index lists, update matrices and factor panels through HBM once per
                # factorisation (1.6 GB of L / U sets at G = 128: far beyond the caches) -- the bound a large batch actually runs into
                gb3 = k3_bytes * ph["n_solves"] / ph["factor"] / 1e9
                ent["roofline_k3_hbm"] = {"bound": "hbm", "achieved": gb3, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gb3 / HBM_PEAK_GBS, "traffic": None,
                                          "algorithmic_bytes_per_factorisation": k3_bytes,
                                          "note": "bytes of one multifrontal factorisation of the C2 graph (seed 42): front-ordered H + targets 12 B per entry, children's "
                                                  "update matrices + targets 12 B per entry read and 8 B written, factor panels 8 B per entry written"}
        if ph["linearize"] > 0:
            gb = k1_bytes * ph["n_relinearized"] / ph["linearize"] / 1e9
            k1_name = ("kb_linearize<0,0,true> + kb_linearize<0,1,false> (thread per factor)" if ph["thread_form"] else "kb_linearize_lanes") if mode == P.JAC_NUMERIC else "kb_linearize<1,*>"
            ent["roofline_k1"] = {"bound": "hbm", "kernel": k1_name,
                                  "achieved": gb, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gb / HBM_PEAK_GBS, "traffic": None,
                                  "us_per_graph_amortised": 1e6 * ph["linearize"] / max(1, ph["n_relinearized"])}
        res[str(G)] = ent
        mm.close()
        for gk in gs:
            gk.close()
    return res


def factorisation_work(A):
    """flops of one multifrontal factorisation (right-looking partial Cholesky of every front incl. the rhs row) and its algorithmic
    bytes: front-ordered H + targets 12 B per entry, children's update matrices + targets 12 B per entry read and 8 B written,
    factor panels 8 B per entry written (SURVEY 8(d) / DESIGN section 5)"""
    fl = 0
    for p_, b_ in zip(A["f_p"].tolist(), A["f_b"].tolist()):
        fa = p_ + b_ + 1
        for k in range(p_):
            fl += (fa - k - 1) * (fa - k) + (fa - k - 1)
    nbytes = int(A["f_el_off"][-1]) * 12 + int(A["f_ea_off"][-1]) * 20 + int(A["L_size"]) * 8
    return fl, nbytes


def gather_objects(dist, obj, world):
    """every rank's object on every rank (outside any timed region; the data path has no collective)"""
    if dist is None:
        return [obj]
    out = [None] * world
    dist.all_gather_object(out, obj)
    return out


def rank_seed(rank):
    return C4_SEEDS[rank % len(C4_SEEDS)]


def aggregate(dist, elapsed, iters, device):
    """whole-job numbers: MAX of the per-rank wall time, SUM of the per-rank LM iterations"""
    if dist is None:
        return elapsed, float(iters)
    import torch
    t = torch.tensor([elapsed], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    it_t = torch.tensor([float(iters)], dtype=torch.float64, device=device)
    dist.all_reduce(it_t, op=dist.ReduceOp.SUM)
    return float(t.item()), float(it_t.item())


def dump_outputs(path, graphs, seeds, last_iters):
    """what the last timed step returned to its caller, per graph: the optimised estimate, chi2 and LM iterations; with several
    graphs per rank (N > 1) every name carries its graph's seed"""
    os.makedirs(path, exist_ok=True)
    for gk, sd, it in zip(graphs, seeds, last_iters):
        prefix = "" if len(graphs) == 1 else "seed%d_" % sd
        arrays = {"poses": gk.get_poses(), "planes": gk.get_planes(), "final_chi2": [gk.chi2()], "lm_iterations": [it]}
        for name, a in arrays.items():
            np.save(os.path.join(path, prefix + name + ".npy"), np.asarray(a, dtype=np.float64))


def cpu_dry_run(args, rank, world):
    """No GPU: every rank builds and analyses ITS graph (host logic only) and feeds synthetic timings
    through the same aggregation the real run uses."""
    import torch.distributed as dist
    import pop_up_slam_amd as P
    from pop_up_slam_amd import synth
    if world > 1:
        dist.init_process_group(backend="gloo")
    spec = synth.corridor(120, 26, seed=rank_seed(rank))
    g = P.Graph()
    spec.replay(g)
    g.analyze()
    st = g.stats()
    elapsed, iters = 0.1 * (rank + 1), 10 * (rank + 1)
    if world > 1:
        dist.barrier()
    elapsed, total = aggregate(dist if world > 1 else None, elapsed, iters, "cpu")
    if rank == 0:
        print(json.dumps({"dry_run": True, "n_gpus": world, "value": total / elapsed, "elapsed_max": elapsed,
                          "total_iters": total, "seed": rank_seed(rank), "fronts": st["n_fronts"], "scaling": "weak"}))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def self_launch(args):
    """`python bench.py --gpus N` (N > 1) outside any launcher: start the N ranks -- one process per GPU, RANK / LOCAL_RANK /
    WORLD_SIZE / MASTER_* in their environment, rendezvous on 127.0.0.1 -- exactly what `python -m torch.distributed.run --nnodes=1
    --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...` would start; rank 0's stdout (the JSON line) is
    this process' stdout.  Returns the first non-zero exit code of a rank."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), LOCAL_WORLD_SIZE=str(args.gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: what RCCL needs across processes on this driver
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=None if r == 0 else subprocess.DEVNULL))
    rc = 0
    try:
        for pr in procs:
            c = pr.wait()
            rc = rc or c
            if c != 0:                      # a rank died: the others would wait at a barrier for ever
                for q in procs:
                    if q.poll() is None:
                        q.terminate()
    finally:
        for q in procs:
            if q.poll() is None:
                q.kill()
    if rc:
        raise SystemExit(rc)
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mode", choices=["numeric", "analytic"], default="numeric",
                    help="Jacobian mode of the sweep (numeric = reference behaviour)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write what the last timed step computed to DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, measure everything else: rooflines, the other Jacobian mode, pps_multi, concurrent "
                         "handles, C3, C5 and the CPU baselines (the options below select among them)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-c5", action="store_true", help="skip the config-5 frame loop (1000 frames, ~2 s)")
    ap.add_argument("--no-c3", action="store_true", help="skip the config-3 graph (10 000 poses)")
    ap.add_argument("--no-concurrent", action="store_true",
                    help="skip the 8-host-thread section (rocprofv3 --kernel-trace of ROCm 7.2 crashes inside hipLaunchKernel when several "
                         "host threads launch at once; the profile in profiles/ is taken with this flag)")
    ap.add_argument("--batched-replicas", type=int, default=0, help="0 = auto (> 256 MB per sweep)")
    ap.add_argument("--cpu-dry-run", action="store_true",
                    help="CI only: gloo backend, no GPU work -- exercises the rank/seed/aggregation plumbing of the N>1 path")
    args = ap.parse_args()

    if args.gpus < 1:
        ap.error("--gpus must be >= 1")
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        return self_launch(args)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: launch exactly one rank per GPU "
                         f"(python bench.py --gpus N starts them itself)")
    import torch
    if not args.cpu_dry_run and os.environ.get("PPS_BENCH_SHARED_GPU") != "1" and args.gpus > torch.cuda.device_count():
        raise SystemExit(f"bench.py: --gpus {args.gpus} but {torch.cuda.device_count()} device(s) visible "
                         f"(PPS_BENCH_SHARED_GPU=1 puts every rank on device 0: validation on a one-GPU box only)")
    dist = None
    if args.cpu_dry_run:
        return cpu_dry_run(args, rank, world)
    # PPS_BENCH_SHARED_GPU=1 (validation on a one-GPU box only): all ranks use device 0 and meet over gloo
    shared = os.environ.get("PPS_BENCH_SHARED_GPU") == "1"
    if shared:
        local_rank = 0
    if world > 1:
        import torch.distributed as dist
        torch.cuda.set_device(local_rank)
        if shared:
            dist.init_process_group(backend="gloo")
        else:
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))
    assert torch.cuda.is_available(), "bench.py needs a GPU"

    import pop_up_slam_amd as P
    from pop_up_slam_amd import synth

    mode = P.JAC_NUMERIC if args.mode == "numeric" else P.JAC_ANALYTIC
    # N = 1: the C2 graph (seed 42).  N > 1: every rank holds the eight C4 timing graphs and a step solves all of them
    # once, rank r starting at graph r -- at any moment the GPUs work on different, independently seeded graphs, and every
    # rank does the same work per step (a fixed graph per rank would time the slowest seed: 55 vs 79 LM trials per solve).
    seeds = [rank_seed(0)] if world == 1 else [rank_seed((k + rank) % len(C4_SEEDS)) for k in range(len(C4_SEEDS))]
    graphs = []
    for sd in seeds:
        spec_k = synth.corridor(seed=sd)
        gk = P.Graph(device=local_rank, jacobian_mode=mode)
        spec_k.replay(gk)
        gk.save_state()
        graphs.append(gk)
    g = graphs[0]

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    for gk in graphs[1:]:                    # every handle analysed / uploaded / run once before the clock starts
        gk.restore_state(); gk.batch_optimize()

    def step():
        """N = 1: one LM solve of the C2 graph.  N > 1: this rank's eight C4 graphs solved once each, starting with graph
        `rank` -- every rank does exactly the same work in every step, whatever K is.  Returns the LM iterations per graph."""
        its = []
        for gk in graphs:
            gk.restore_state()
            its.append(gk.batch_optimize())
        return its

    for i in range(args.warmup):
        step()
    barrier()
    t0 = time.perf_counter()
    iters = 0
    for i in range(args.steps):
        last = step()
        iters += sum(last)
    barrier()
    elapsed = time.perf_counter() - t0
    solves = args.steps * len(graphs)
    chi2 = g.chi2()
    st = g.stats()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, graphs, seeds, last)

    elapsed, total_iters = aggregate(dist, elapsed, iters, "cpu" if shared else "cuda")
    out = {
        "metric": "graph-solve iters/sec + final chi2, 1k-pose/5k-edge plane graph",
        "value": total_iters / elapsed, "unit": "LM iters/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "config": {"workload": "C2 synthetic corridor: 1000 SE3 poses, 200 planes, 5000 plane edges, 999 odometry edges "
                               "(BASELINE.json configs[1], seed 42)" + ("" if world == 1 else
                               "; N > 1 = config 4: eight independently seeded C2 graphs per rank (timing seeds %s: the "
                               "short, balanced LM runs; parity on SURVEY's seeds 100-107 is a test, not a bench line), one "
                               "step = all eight solved once, rank r starting at graph r, no collective" % C4_SEEDS),
                   "jacobian_mode": args.mode, "lm_solves_per_step": len(graphs), "lm_iterations_per_solve": iters / solves,
                   "graphs_per_sec": world * solves / elapsed, "total_lm_iterations": total_iters, "total_lm_solves": world * solves},
        "final_chi2": chi2, "chi2_initial": st["chi2_initial"],
        "fronts": st["n_fronts"], "levels": st["n_levels"], "max_front": st["max_front"],
    }
    if not args.full:
        if rank == 0:
            print(json.dumps(out))
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        return None

    # --full: everything below runs after the headline's measurement and does not change it
    spec = synth.corridor(seed=seeds[0])
    # one more solve of this rank's first graph with an event pair around every K1 launch
    g.restore_state(); g.set_profiling(1); g.batch_optimize(); g.set_profiling(0)
    st = g.stats()
    k1_time, k1_launches = st["t_linearize"], st["n_linearize"]

    # N > 1 (BASELINE config 4 / north_star: "graphs/sec and achieved-HBM-fraction at 1/2/4/8 GPUs"): every rank also runs the
    # many-graphs-per-launch form on ITS device -- G = 8 (config 4's size) and G = 128 (where one GPU saturates) -- and rank 0
    # adds the graphs/s up and reports the per-rank roofline fractions.  No collective on the data path: the ranks meet at a
    # barrier before and after, and exchange their result dictionaries afterwards.
    multi_ranks = None
    if world > 1:
        cnt_r = spec.counts()
        k1_bytes_r = cnt_r[synth.F_PLANE_OBS] * B_PLANE_EDGE + cnt_r[synth.F_ODOMETRY] * B_ODO_EDGE
        fl_r, k3_bytes_r = factorisation_work(g.analysis_dump())
        g_list = tuple(int(x) for x in os.environ.get("PPS_BENCH_MULTI_G", "8,128").split(","))
        barrier()
        mine = multi_graph_bench(P, synth, local_rank, mode, args, spec, fl_r, k1_bytes_r, torch, k3_bytes_r, g_list=g_list)
        barrier()
        multi_ranks = gather_objects(dist, mine, world)

    if rank == 0:
        counts = spec.counts()
        n_obs, n_odo = counts[synth.F_PLANE_OBS], counts[synth.F_ODOMETRY]
        bytes_per_launch = n_obs * B_PLANE_EDGE + n_odo * B_ODO_EDGE
        # K1 INSIDE a solve: every launch of one extra solve is made with hipExtLaunchKernelGGL, whose start / stop events carry
        # the dispatch's own begin / end timestamps (what rocprofv3 reports for the kernel: profiles/r6_kernel_stats_c2.txt)
        k1_in_solve = k1_time / max(1, k1_launches)
        g.restore_state()
        k1_replay = g.time_linearize(mode, 400)             # 400 back-to-back launches between two events: hot caches
        achieved = bytes_per_launch / k1_in_solve / 1e9 if k1_in_solve > 0 else 0.0
        roofline = {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": achieved / HBM_PEAK_GBS, "traffic": None,
                    "kernel": "k_trial_lin (both trials' retraction + chi2 and the K1 sweep at the trial point LM is predicted to accept, ONE launch); "
                              "k_linearize_lanes for the first linearisation and after a wrong prediction" if mode == P.JAC_NUMERIC else "k_linearize<1,0>+<1,1>",
                    "launches": k1_launches, "avg_launch_us": k1_in_solve * 1e6,
                    "replay_avg_launch_us": k1_replay * 1e6, "replay_launches": 400,
                    "algorithmic_bytes_per_launch": bytes_per_launch,
                    # the same launches with the trials' own work counted as well: k_trial_lin also evaluates every edge at both trial points
                    # (K4: 176 B per edge and trial) -- given for transparency, `frac` above counts the sweep alone
                    "frac_incl_trial_bytes": ((bytes_per_launch + 2 * B_TRIAL_EDGE * (n_obs + n_odo)) / k1_in_solve / 1e9 / HBM_PEAK_GBS
                                              if (mode == P.JAC_NUMERIC and k1_in_solve > 0) else None),
                    "note": "K1 of the C2 graph inside an LM solve, on the solver's stream: mean dispatch duration (start / stop "
                            "events of hipExtLaunchKernelGGL = the kernel's own begin / end timestamps) over every launch of one "
                            "solve whose sweep became a linearisation LM used.  Since round 6 that launch is k_trial_lin: the sweep "
                            "runs BESIDE the two trials' retraction + chi2 blocks, so its duration covers both (12.9 us against "
                            "9.1 + 9.3 for the two launches it replaces); only the sweep's 392 / 840 B per edge are counted as "
                            "algorithmic bytes, not the trials' 176 B per edge.  profiles/r6_kernel_stats_c2.txt has the same "
                            "launches (rocprofv3 of tools/timeline_c2.py, C2 only).  replay_avg_launch_us: 400 back-to-back "
                            "launches of the plain sweep between two events (hot caches, the more flattering figure; not used for "
                            "frac).  One C2 graph is 2.8 MB per sweep: cache-resident and latency bound, so HBM traffic is not "
                            "meaningful here (traffic: null); see roofline_batched for the same kernel family over > 256 MB"}
        # the same solve: dispatch durations of its factor launches; a launch set holds two factorisations (lambda and lambda * 10)
        # -- or one, where the loop dropped the speculation (graphs that fill the GPU: pps_solve.cpp)
        fact_us = 1e6 * st["t_factor"] / max(1, st["n_factorize"])               # device time per factorisation, amortised
        dual_factor_us = 2 * fact_us
        # batched variant: replicate the edge arrays until one sweep moves > 256 MB; the plane-edge launch
        # (5 of every 6 factors) is the dominant kernel, the odometry launch is reported next to it
        reps = args.batched_replicas or int(np.ceil(300e6 / bytes_per_launch))
        pmc_js, pmc_src = load_pmc()
        pmc = pmc_js.get("kernels", {})
        roofline_batched = {}
        # numeric_lanes: the lane-parallel central differences (3 plane observations per wavefront) -- the form a graph below
        # 200 000 factors (a batch chunk below 120 000) runs; numeric: one thread per factor (large batches); analytic: closed-form Jacobians
        for mname, mcode in (("analytic", P.JAC_ANALYTIC), ("numeric_lanes", 2), ("numeric", P.JAC_NUMERIC)):
            (sec_all, sec_pl, sec_od), npl, nod = g.bench_sweep(mcode, reps, 10)
            ent = {}
            kfmt = "k_sweep_bench_lanes<%d>" if mcode == 2 else "k_sweep_bench<" + str(mcode) + ",%d>"
            for part, sec_k, nbytes, kname in (("plane_edges", sec_pl, npl * B_PLANE_EDGE, "k_sweep_bench_obs_numeric" if mcode == P.JAC_NUMERIC else kfmt % 0),
                                               ("odometry", sec_od, nod * B_ODO_EDGE, kfmt % 1)):
                rec = pmc.get(f"{mname}_{part}")
                traffic = None
                if rec and reps == pmc_js.get("replicas") and "hbm_bytes_corrected" in rec:   # same replica count as the PMC passes
                    traffic = rec["hbm_bytes_corrected"]
                ent[part] = {"bound": "hbm", "achieved": nbytes / sec_k / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                             "frac": nbytes / sec_k / 1e9 / HBM_PEAK_GBS, "traffic": traffic, "kernel": kname,
                             "algorithmic_bytes_per_launch": nbytes, "avg_launch_us": sec_k * 1e6}
                # the numeric sweeps' own roof is vector-instruction ISSUE, not HBM: wave instructions of the launch (PMC SQ_INSTS_VALU, same
                # source hash) x 4 cycles (one fp64 wave instruction occupies its SIMD for four) / (1 024 SIMDs x clock) / measured time
                if rec and reps == pmc_js.get("replicas") and rec.get("valu_wave_insts_per_launch"):
                    issue_s = rec["valu_wave_insts_per_launch"] * 4.0 / (N_SIMD * CLOCK_HZ)
                    ent[part]["valu_frac"] = issue_s / sec_k
                    ent[part]["valu_insts_per_edge"] = rec.get("valu_insts_per_edge_lane")
                    ent[part]["valu_note"] = ("issue-bound time %.1f us = %.0f wave instructions x 4 cycles / (%d SIMDs x %.1f GHz)"
                                              % (issue_s * 1e6, rec["valu_wave_insts_per_launch"], N_SIMD, CLOCK_HZ / 1e9))
            ent["both_launches_us"] = sec_all * 1e6
            ent["replicas"], ent["n_plane_edges"], ent["n_odometry_edges"] = reps, npl, nod
            ent["traffic_source"] = pmc_src
            roofline_batched[mname] = ent
        out.update({
            # kernel launches of one LM solve (pps_stats.n_launches): the dual loop issues both damping values of a
            # linearisation in the same launches on one stream (round 1: 21 launches per accepted + rejected pair on two streams)
            "launches_per_lm_iteration": st["n_launches"] / max(1, st["lm_iterations"]), "launches_per_solve": st["n_launches"],
            "roofline": roofline, "roofline_batched": roofline_batched,
        })
        if multi_ranks is not None:
            # whole-job figures of the many-graphs-per-launch form: graphs/s added up over the ranks (every rank ran the same G
            # graphs on its own device between the same two barriers), roofline fractions as the range over the ranks
            agg = {}
            for G in multi_ranks[0]:
                per = [mr[G] for mr in multi_ranks]
                ent = {"graphs_per_rank": int(G), "graphs_per_sec": float(sum(p_["graphs_per_sec"] for p_ in per)),
                       "value": float(sum(p_["value"] for p_ in per)), "unit": "LM iters/s",
                       "graphs_per_sec_per_rank": [p_["graphs_per_sec"] for p_ in per],
                       "bit_identical_to_single_handle": all(p_["bit_identical_to_single_handle"] for p_ in per),
                       "same_iteration_counts": all(p_["same_iteration_counts"] for p_ in per)}
                for key in ("roofline_k1", "roofline_k3_hbm", "roofline_k3"):
                    fr = [p_[key]["frac"] for p_ in per if key in p_]
                    if fr:
                        ent[key] = {"bound": per[0][key]["bound"], "peak": per[0][key]["peak"], "unit": per[0][key]["unit"],
                                    "frac_min": min(fr), "frac_max": max(fr), "achieved_per_rank": [p_[key]["achieved"] for p_ in per if key in p_]}
                agg[G] = ent
            out["multi_graph_per_gpu"] = agg
            out["config"]["scale_line"] = ("the SCALE curve of north_star's quantities is multi_graph_per_gpu['128'].graphs_per_sec (and ['8'], config 4's "
                                           "size) with its roofline_k1 / roofline_k3_hbm fractions; `value` stays the BASELINE metric on single handles")
        if world == 1:
            # the closed-form Jacobian mode on the same graph (not the reference's arithmetic; reported, not the headline)
            other = P.JAC_ANALYTIC if mode == P.JAC_NUMERIC else P.JAC_NUMERIC
            g2 = P.Graph(device=local_rank, jacobian_mode=other)
            spec.replay(g2)
            g2.save_state()
            for _ in range(max(1, args.warmup)):
                g2.restore_state(); g2.batch_optimize()
            torch.cuda.synchronize()
            t1 = time.perf_counter(); it2 = 0
            for _ in range(args.steps):
                g2.restore_state(); it2 += g2.batch_optimize()
            torch.cuda.synchronize()
            e2 = time.perf_counter() - t1
            out["other_mode"] = {"jacobian_mode": "analytic" if other == P.JAC_ANALYTIC else "numeric",
                                 "value": it2 / e2, "unit": "LM iters/s", "final_chi2": g2.chi2()}
        if world == 1:
            # K3 (the kernels most of a solve's device time goes to): flops of one multifrontal factorisation against the
            # fp64 MFMA peak.  The fronts are <= 51 rows on a 10-level tree, so this is a dependency chain (tree depth x
            # per-front latency), not a throughput kernel -- the fraction says how far from a compute bound it sits.
            A = g.analysis_dump()
            fl, k3_bytes_c2 = factorisation_work(A)
            g.restore_state(); g.set_profiling(2); g.batch_optimize(); st2 = g.stats(); g.set_profiling(0)
            t_fac = st2["t_factor"] / max(1, st2["n_factorize"])
            whole_tree = int(A["n_groups"]) <= 512 and int(A["n_stages"]) >= 2       # (the rule of run_analysis, pps_upload.cpp: k_band_factor_all)
            k3_kernel = ("k_band_factor_all (every band group of the tree is a workgroup of ONE launch; groups hand their update matrices over through "
                         "per-front flags in global memory)" if whole_tree else
                         "k_band_factor_pre x %d + k_band_root<true, true>" % (int(A["n_stages"]) - 1))
            out["roofline_k3"] = {"bound": "mfma", "kernel": k3_kernel,
                                  "achieved": 2 * fl / (dual_factor_us * 1e-6) / 1e12, "peak": 78.6, "unit": "TFLOP/s",
                                  "frac": 2 * fl / (dual_factor_us * 1e-6) / 1e12 / 78.6,
                                  "flops_per_factorisation": fl, "us_per_pair_of_factorisations": dual_factor_us,
                                  "one_step_loop": {"us_per_factorisation": 1e6 * t_fac, "frac": fl / t_fac / 1e12 / 78.6,
                                                    "us_per_backsolve": 1e6 * st2["t_backsolve"] / max(1, st2["n_factorize"])},
                                  "hbm": {"bound": "hbm", "achieved": 2 * k3_bytes_c2 / (dual_factor_us * 1e-6) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                          "frac": 2 * k3_bytes_c2 / (dual_factor_us * 1e-6) / 1e9 / HBM_PEAK_GBS, "algorithmic_bytes_per_factorisation": k3_bytes_c2},
                                  "note": "the shipped dual-lambda loop factors H for lambda and lambda * 10 in the same launch (blockIdx.y): "
                                          "us_per_pair_of_factorisations = sum of the dispatch durations of the factor launches of one "
                                          "solve / number of launch sets (profiles/r6_kernel_stats_c2.txt: k_band_factor_all, one launch per set); "
                                          "one_step_loop = the profiling loop with one factorisation at a time.  Latency bound by construction "
                                          "(511 fronts of <= 51 rows, 9 tree levels: a chain of nine single-wave front latencies); peak = fp64 matrix "
                                          "rate of MI355X (public spec; the CDNA4 guide lists none)"}
            # headroom on one GPU: one C2 solve keeps a few dozen of the 256 CUs busy, so independent graphs (one handle
            # + one host thread each, no shared state) overlap.  Reported next to the headline, which stays the
            # one-graph-per-GPU configuration BASELINE.json names.
            import threading
            n_h = 0 if args.no_concurrent else 8
            hs = []
            for k in range(n_h):
                gk = P.Graph(device=local_rank, jacobian_mode=mode)
                synth.corridor(seed=rank_seed(k)).replay(gk)
                gk.save_state(); gk.batch_optimize()
                hs.append(gk)
            counts_k = [0] * n_h

            def work(k):
                for _ in range(max(2, args.steps // 4)):
                    hs[k].restore_state()
                    counts_k[k] += hs[k].batch_optimize()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            th = [threading.Thread(target=work, args=(k,)) for k in range(n_h)]
            for t in th: t.start()
            for t in th: t.join()
            torch.cuda.synchronize()
            e3 = time.perf_counter() - t1
            out["concurrent_graphs_one_gpu"] = {"handles": n_h, "value": sum(counts_k) / e3, "unit": "LM iters/s",
                                                "graphs_per_sec": n_h * max(2, args.steps // 4) / e3,
                                                "seeds": [rank_seed(k) for k in range(n_h)]}
            for gk in hs:
                gk.close()
        if world == 1:
            # pps_multi: G independent C2 graphs per launch (BASELINE config 4 on ONE device; north_star's graphs/sec).  The
            # headline above stays the single graph BASELINE.json's metric is quoted on.
            out["multi_graph_one_gpu"] = multi_graph_bench(P, synth, local_rank, mode, args, spec, out["roofline_k3"]["flops_per_factorisation"],
                                                           bytes_per_launch, torch, k3_bytes_c2)
        if world == 1 and not args.no_c3:
            # BASELINE config 3: 10 000 poses / 2 000 planes / 60 000 plane edges (one 31.9 MB Jacobian sweep per linearisation)
            spec3 = synth.manhattan_rooms()
            g3 = P.Graph(device=local_rank, jacobian_mode=mode)
            spec3.replay(g3); g3.save_state()
            it3 = g3.batch_optimize()
            c3_chi2 = g3.chi2()
            walls = []
            for _ in range(5):
                g3.restore_state()
                t1 = time.perf_counter(); it3 = g3.batch_optimize(); walls.append(time.perf_counter() - t1)
            w3 = float(np.median(walls))
            g3.restore_state(); g3.set_profiling(2); g3.batch_optimize(); s3 = g3.stats(); g3.set_profiling(0)
            cnt3 = spec3.counts()
            bytes3 = cnt3[synth.F_PLANE_OBS] * B_PLANE_EDGE + cnt3[synth.F_ODOMETRY] * B_ODO_EDGE
            g3.restore_state(); g3.set_profiling(1); g3.batch_optimize(); s3d = g3.stats(); g3.set_profiling(0)      # dual loop, dispatch timestamps
            fl3, k3_bytes3 = factorisation_work(g3.analysis_dump())
            pair3 = 2 * s3d["t_factor"] / max(1, s3d["n_factorize"])               # (amortised: C3 runs most launch sets with one factorisation)
            k1_3_solve = s3d["t_linearize"] / max(1, s3d["n_linearize"])
            g3.restore_state()
            k1_3 = g3.time_linearize(mode, 100)
            nf3, nl3 = max(1, s3["n_factorize"]), max(1, s3["n_linearize"])
            out["c3"] = {"workload": "C3 synthetic Manhattan rooms: %d poses, %d planes, %d plane edges, %d odometry edges (BASELINE.json configs[2])"
                                     % (spec3.n_poses, spec3.n_planes, cnt3[synth.F_PLANE_OBS], cnt3[synth.F_ODOMETRY]),
                         "lm_iterations": it3, "value": it3 / w3, "unit": "LM iters/s", "us_per_lm_iteration": 1e6 * w3 / max(1, it3),
                         "final_chi2": c3_chi2, "fronts": s3["n_fronts"], "levels": s3["n_levels"], "max_front": s3["max_front"],
                         "phase_us_per_call": {"k1": 1e6 * s3["t_linearize"] / nl3, "k2": 1e6 * s3["t_assemble"] / nl3, "factor": 1e6 * s3["t_factor"] / nf3,
                                               "backsolve": 1e6 * s3["t_backsolve"] / nf3, "trial": 1e6 * s3["t_retract_chi2"] / nf3},
                         "roofline_k1": {"bound": "hbm", "kernel": "k_linearize_lanes" if mode == P.JAC_NUMERIC else "k_linearize<1,*>",
                                         "achieved": bytes3 / k1_3_solve / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": bytes3 / k1_3_solve / 1e9 / HBM_PEAK_GBS,
                                         "algorithmic_bytes_per_launch": bytes3, "avg_launch_us": 1e6 * k1_3_solve, "launches": s3d["n_linearize"],
                                         "replay_avg_launch_us": 1e6 * k1_3, "traffic": None,
                                         "note": "inside the solve (dispatch timestamps); profiles/r6_kernel_stats_c3.txt"},
                         "roofline_k3_hbm": {"bound": "hbm", "kernel": "k_band_factor_pre / k_band_factor<true> + k_band_factor_r5",
                                             "achieved": 2 * k3_bytes3 / pair3 / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                             "frac": 2 * k3_bytes3 / pair3 / 1e9 / HBM_PEAK_GBS, "algorithmic_bytes_per_factorisation": k3_bytes3,
                                             "us_per_factorisation_amortised": 1e6 * pair3 / 2, "factorisations": s3d["n_factorize"], "traffic": None,
                                             "note": "sum of the dispatch durations of the factor launches of one solve / factorisations done (adaptive "
                                                     "speculation: most launch sets of C3 hold ONE factorisation); profiles/r6_kernel_stats_c3.txt"},
                         "roofline_k3": {"bound": "mfma", "achieved": 2 * fl3 / pair3 / 1e12, "peak": 78.6, "unit": "TFLOP/s", "frac": 2 * fl3 / pair3 / 1e12 / 78.6,
                                         "flops_per_factorisation": fl3}}
            g3.close()
        if world == 1 and not args.no_c5:
            # BASELINE config 5: 1000 synthetic 640x480 frames, pop-up (half resolution) fused with the incremental solve
            from pop_up_slam_amd import pipeline
            n5 = 1000
            frames = pipeline.popup_sequence(n5)
            # (round 6: the pop-up run of a frame is not waited for -- the graph construction takes the plane equations as soon as the kernel
            # has published them, the pixels of frame k are collected when frame k + 1 is launched; every frame's cloud is still computed)
            pl5, g5, pp5, st5 = pipeline.gpu_pipeline(step=2, async_popup=True)
            t1 = time.perf_counter(); lm5 = 0; an5 = up5 = 0.0
            for fr in frames:
                it5 = pl5.process(fr)
                lm5 += max(it5, 0)
                s5 = g5.stats(); an5 += s5["t_analysis"]; up5 += s5["t_upload"]
            pipeline.gpu_pipeline_finish(pp5, st5)
            e5 = time.perf_counter() - t1
            # (the pop-up kernel on its own: the synchronous entry point times it with an event pair, the asynchronous one does not)
            for fr in frames[:50]:
                pp5.run(fr.seg2d, synth.T_from_pose(fr.true_pose).astype(np.float32), fr.polys, step=2, depth_thre=10.0, ceiling_thre=2.5)
                st5["popup_kernel_s"] += pp5.last_kernel_time() * n5 / 50
            out["c5_frame_loop"] = {"frames": n5, "frames_per_sec": n5 / e5, "lm_iterations": lm5, "final_chi2": g5.chi2(),
                                    "host_analysis_ms_per_frame": 1e3 * an5 / n5, "upload_ms_per_frame": 1e3 * up5 / n5,
                                    "popup_kernel_us_per_frame": 1e6 * st5["popup_kernel_s"] / n5, "points_per_frame": st5["points"] / n5,
                                    "note": "Python frame loop over the C-ABI (tools/c5_bench.py); the C++ facade loop is tools/c5_bench_cpp.py"}
            g5.close(); pp5.close()
            # the same 1000 frames with the host loop in C++ over include/pps_isam.hpp (what a maintainer's Mapper_mono runs):
            # tools/c5_bench_cpp.py writes the drive as a binary script, builds tools/cpp/c5_replay.cpp with g++ and runs it
            try:
                import subprocess
                r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "c5_bench_cpp.py")], capture_output=True, text=True, timeout=240)
                line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
                out["c5_frame_loop_cpp_host"] = json.loads(line)
            except Exception as e:      # no compiler on the box, ...: the Python-loop figure above stands
                out["c5_frame_loop_cpp_host"] = {"error": repr(e)[:200]}
        if not args.no_cpu_baseline and world == 1:
            cb = cpu_baseline(spec)
            out["cpu_baseline"] = cb
            out["speedup_vs_cpu_baseline"] = out["value"] / cb["value"]
            cbo = cpu_baseline(spec, budget_s=4.0, optimised=True)      # the claim is shown against both
            out["cpu_baseline_optimised"] = cbo
            out["speedup_vs_cpu_baseline_optimised"] = out["value"] / cbo["value"]
            nth = max(2, min(8, (os.cpu_count() or 2) // 2))
            cbm = cpu_baseline(spec, budget_s=4.0, optimised=True, threads=nth)
            out["cpu_baseline_optimised_mt"] = cbm
            out["speedup_vs_cpu_baseline_optimised_mt"] = out["value"] / cbm["value"]
            out["chi2_rel_err_vs_cpu"] = abs(chi2 - cb["final_chi2"]) / abs(cb["final_chi2"])
            if "c3" in out:
                # the CPU oracle on C3 (one solve, ~10 s: part of this leg's budget): chi2 parity and the CPU rate at that size
                from oracle import oracle_py as O
                o3 = O.OracleGraph(); synth.manhattan_rooms().replay(o3)
                t1 = time.perf_counter(); ito3 = o3.batch_optimize(); eo3 = time.perf_counter() - t1
                co3 = o3.chi2()
                out["c3"]["cpu_oracle"] = {"lm_iterations": ito3, "value": ito3 / eo3, "unit": "LM iters/s", "seconds": eo3, "final_chi2": co3, "cores": 1, "kind": "port"}
                out["c3"]["chi2_rel_err_vs_cpu"] = abs(out["c3"]["final_chi2"] - co3) / abs(co3)
                out["c3"]["speedup_vs_cpu_oracle"] = out["c3"]["value"] / (ito3 / eo3)
            if "other_mode" in out:
                out["other_mode"]["chi2_rel_err_vs_cpu"] = abs(out["other_mode"]["final_chi2"] - cb["final_chi2"]) / abs(cb["final_chi2"])
        print(json.dumps(out))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
