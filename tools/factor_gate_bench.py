"""Time of pps_factor_gate over ALL factors of C2 (corridor, 1 000 poses) and C3 (manhattan rooms, 10 000 poses), after one optimisation and
one recovery each, next to the route that answers the same question without the call: pps_cov_marginals and pps_cov_access for the
blocks of every factor's joint marginal, pps_eval_factor per factor for r and J, numpy for P = J Sigma J', its trace and the solve.

  python tools/factor_gate_bench.py [--reps 11] [--out profiles/factor_gate_bench.json]

Reports, per graph: the device seconds around the call's kernel (pps_factor_gate_last; median, min, max over the repetitions after one
warm-up call, which also builds and uploads the factor table), the host wall time of the call, the wall time of the download route (once:
it is thousands of round trips), their ratio, and the largest relative difference between the two routes' d2.  A record, not a pass / fail
check; no ratio is promised.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pop_up_slam_amd as P  # noqa: E402
from pop_up_slam_amd import synth  # noqa: E402


def download_route(g, spec, nid, fid):
    """d2 and leverage of every factor from downloaded blocks, pps_eval_factor and numpy"""
    dims = {int(n): (6 if t == synth.NODE_POSE else 3) for n, t in zip(nid, spec.node_type)}
    nodes = [(int(nid[a]), int(nid[b]) if b >= 0 else -1) for a, b in spec.f_nodes]
    ids = sorted(dims)
    marg = dict(zip(ids, g.cov_marginals(ids)))
    pairs = sorted({(a, b) for a, b in nodes if b >= 0})
    cross = dict(zip(pairs, g.cov_access(pairs)))
    mode = g.get_props().jacobian_mode
    d2, lev = np.full(len(fid), np.nan), np.zeros(len(fid))
    for k, f in enumerate(fid):
        J, r = g.eval_factor(int(f), mode)
        a, b = nodes[k]
        if b < 0:
            S = marg[a]
        else:
            S = np.block([[marg[a], cross[(a, b)]], [cross[(a, b)].T, marg[b]]])
        Pm = J @ S @ J.T
        lev[k] = np.trace(Pm)
        A = np.eye(len(r)) - Pm
        try:
            L = np.linalg.cholesky(A)
            if np.min(np.diag(L)) ** 2 > 1e-7:
                y = np.linalg.solve(L, r); d2[k] = y @ y
        except np.linalg.LinAlgError:
            pass
    return d2, lev


def measure(name, spec, reps):
    g = P.Graph(); nid, fid = spec.replay(g)
    g.batch_optimize(); g.cov_recover()
    g.factor_gate()                                        # warm-up: the factor table, buffers, events
    dev, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); d2, lev, flagged = g.factor_gate(); wall.append(time.perf_counter() - t0)
        sec, launches, untestable = g.factor_gate_last(); dev.append(sec)
    t0 = time.perf_counter(); r2, rlev = download_route(g, spec, nid, fid); route = time.perf_counter() - t0
    both = np.isfinite(d2) & np.isfinite(r2)
    rec = {"graph": name, "n_factors": int(len(fid)), "dim_nodes": g.stats()["dim_nodes"], "reps": reps, "launches": launches, "n_untestable": untestable,
           "n_flagged": int(len(flagged)), "kernel_sec_median": float(np.median(dev)), "kernel_sec_min": float(np.min(dev)), "kernel_sec_max": float(np.max(dev)),
           "wall_sec_median": float(np.median(wall)), "download_route_wall_sec": route, "download_route_over_call": route / float(np.median(wall)),
           "sum_leverage": float(np.sum(lev)), "untestable_agree": bool(np.array_equal(np.isnan(d2), np.isnan(r2))),
           "d2_max_rel_difference": float(np.max(np.abs(d2 - r2)[both] / r2[both])), "recover_sec": g.cov_last_times()[0]}
    g.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "factor_gate_bench.json"))
    ap.add_argument("--graphs", default="c2,c3")
    a = ap.parse_args()
    makers = {"c2": ("c2_corridor_1000", synth.corridor), "c3": ("c3_manhattan_10000", synth.manhattan_rooms)}
    recs = [measure(makers[k][0], makers[k][1](), a.reps) for k in a.graphs.split(",")]
    for r in recs:
        print(json.dumps(r))
    with open(a.out, "w") as f:
        json.dump(recs, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
