"""Times of pps_cov_select on dense-front graphs, next to pps_cov_factor and to the per-node route it replaces.

  python tools/cov_select_time.py [--out profiles/cov_select_times.json]

  Per graph -- dense_300p_3000l (300 poses, 3 000 loop closures: a front of 1 290 rows), sphere2500 and torus10000 after batch_optimize:
      pps_cov_select            device seconds of the whole call and of its root -> leaves pass alone (pps_cov_last_times), host wall time
      pps_cov_factor            device seconds of the whole call: the factor stage both calls share
      pps_cov_block, diagonal   the diagonal blocks of ALL poses by root-path solves, one call per pose as the facade's marginal_any makes
                                them: the sum of the kernels' device seconds (pps_cov_block_last) and the host wall time of the loop
      pps_cov_marginals         host wall time of reading all diagonal blocks from the selection (one gather launch, one copy)
Every figure is the median of 11 after two warm-ups (the per-pose loop: one warm-up pass over 50 poses, then one timed pass over all).
A record, not a pass / fail check.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pop_up_slam_amd as P  # noqa: E402
from pop_up_slam_amd import graphio  # noqa: E402

WARM, REPS = 2, 11
DATA = os.path.join(ROOT, "tests", "golden", "isam_data")


def median_of(call, read):
    vals, wall = [], []
    for k in range(WARM + REPS):
        t0 = time.perf_counter(); call(); dt = time.perf_counter() - t0
        if k >= WARM:
            vals.append(read()); wall.append(dt)
    return np.median(np.array(vals), axis=0), float(np.median(wall))


def measure(name, spec):
    g = P.Graph(jacobian_mode=1); nid, _ = spec.replay(g)
    poses = [int(n) for n in nid]
    it = g.batch_optimize()
    st = g.stats()
    sel, sel_wall = median_of(g.cov_select, g.cov_last_times)
    _, marg_wall = median_of(lambda: g.cov_marginals(poses), lambda: 0.0)
    fac, fac_wall = median_of(g.cov_factor, lambda: g.cov_last_times()[0])
    for p in poses[:50]:
        g.cov_block([p])
    kern = 0.0
    t0 = time.perf_counter()
    for p in poses:
        g.cov_block([p]); kern += g.cov_block_last()[0]
    loop_wall = time.perf_counter() - t0
    g.close()
    return {"poses": len(poses), "max_front": st["max_front"], "n_fronts": st["n_fronts"], "n_levels": st["n_levels"], "lm_iterations": it,
            "cov_select_sec": float(sel[0]), "cov_select_pass_sec": float(sel[1]), "cov_select_wall_sec": sel_wall,
            "cov_marginals_all_poses_wall_sec": marg_wall,
            "cov_factor_sec": float(fac), "cov_factor_wall_sec": fac_wall,
            "cov_block_diagonal_all_poses_kernel_sec": kern, "cov_block_diagonal_all_poses_wall_sec": loop_wall}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from linsolve_helpers import loop_graph
    rec = {"warm_ups": WARM, "reps": REPS}
    for name, make in (("dense_300p_3000l", lambda: loop_graph(300, 3000, seed=2)),
                       ("sphere2500", lambda: graphio.load_edge3_log(os.path.join(DATA, "sphere2500.txt"))),
                       ("torus10000", lambda: graphio.load_edge3_log(os.path.join(DATA, "torus10000.txt")))):
        rec[name] = measure(name, make())
        print(name, json.dumps(rec[name]), flush=True)
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
