"""Time of an LM iteration on C2 (corridor, 1 000 poses, 200 planes) with a robust cost function, next to the squared one-step loop.

  python tools/robust_time.py [--reps 7] [--b 1.0] [--parent-us X] [--out profiles/robust_times.json]

Two handles over the same graph, both created with PPS_NO_DUAL=1 so that the squared solve takes the one-step loop a cost function always
takes: one with pseudo-Huber, one without.  Per repetition the state is restored and pps_batch_optimize runs again; the figure is the
call's wall time divided by its LM iterations, median / min / max over the repetitions after one warm-up solve.  --parent-us records the
same squared figure measured at the parent commit (this tool's squared half needs nothing the parent lacks).  A record, not a check.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["PPS_NO_DUAL"] = "1"            # (read once per handle, at its creation)
import pop_up_slam_amd as P  # noqa: E402
from pop_up_slam_amd import synth  # noqa: E402


def per_iteration(g, reps):
    g.save_state()
    out, its = [], 0
    for k in range(reps + 1):
        g.restore_state()
        its = g.batch_optimize()
        s = g.stats()
        if k:                              # (the first solve is the warm-up: upload, analysis, first launches)
            out.append(1e6 * s["t_total"] / max(1, s["lm_iterations"]))
    return {"us_per_iteration_median": float(np.median(out)), "min": float(np.min(out)), "max": float(np.max(out)), "iterations": int(its),
            "launches": int(g.stats()["n_launches"]), "chi2_final": float(g.chi2())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--b", type=float, default=1.0)
    ap.add_argument("--parent-us", type=float, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    spec = synth.corridor()
    rec = {"graph": "c2_corridor_1000", "reps": a.reps, "b": a.b}
    g = P.Graph(); spec.replay(g)
    rec["squared_one_step"] = per_iteration(g, a.reps)
    g.close()
    if hasattr(P.Graph, "set_cost_function"):
        g = P.Graph(); spec.replay(g)
        g.set_cost_function(P.COST_PSEUDO_HUBER, a.b)
        rec["pseudo_huber_one_step"] = per_iteration(g, a.reps)
        g.close()
    rec["parent_squared_one_step_us"] = a.parent_us
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
