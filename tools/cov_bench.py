"""Time of pps_cov_recover on C2 (corridor, 1 000 poses) and C3 (manhattan rooms, 10 000 poses), next to one pps_update of the same
graph and -- C2 only, C3's H is 66 000 x 66 000 -- the dense CPU inverse the tests compare with.

  python tools/cov_bench.py [--reps 11] [--out profiles/cov_bench.json]

Device times are HIP events on the handle's stream: pps_cov_last_times gives the whole recovery (K1 + K2 + factorisation + the
root -> leaves pass) and the pass alone; the update figure is the sum of pps_stats' phase times at profiling level 2 (the solve code
of pps_update is the parent commit's, untouched).  Medians over --reps calls after two warm-up calls; wall-clock next to them."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pop_up_slam_amd as P
from pop_up_slam_amd import synth


def bench(name, spec, reps, dense):
    g = P.Graph(); nid, fid = spec.replay(g)
    g.batch_optimize()
    g.save_state()
    dev, pas, wall = [], [], []
    for k in range(reps + 2):
        t0 = time.perf_counter(); g.cov_recover(); t1 = time.perf_counter()
        a, b = g.cov_last_times()
        if k >= 2:
            dev.append(a); pas.append(b); wall.append(t1 - t0)
    t0 = time.perf_counter(); m = g.cov_marginals(); t_read = time.perf_counter() - t0
    st = g.stats()
    g.set_profiling(2)
    upd, upd_wall = [], []
    for k in range(reps + 2):
        g.restore_state()
        t0 = time.perf_counter(); g.update(); t1 = time.perf_counter()
        s = g.stats()
        if k >= 2:
            upd.append(s["t_linearize"] + s["t_assemble"] + s["t_factor"] + s["t_backsolve"] + s["t_retract_chi2"]); upd_wall.append(t1 - t0)
    g.set_profiling(0)
    res = {"graph": name, "poses": st["n_poses"], "planes": st["n_planes"], "factors": st["n_factors"], "fronts": st["n_fronts"],
           "levels": st["n_levels"], "max_front": st["max_front"], "reps": reps,
           "cov_recover_device_us": 1e6 * float(np.median(dev)), "cov_pass_device_us": 1e6 * float(np.median(pas)),
           "cov_recover_wall_us": 1e6 * float(np.median(wall)), "cov_recover_device_us_min_max": [1e6 * min(dev), 1e6 * max(dev)],
           "read_all_marginals_wall_us": 1e6 * t_read, "n_marginals": len(m),
           "update_device_us_profiling2": 1e6 * float(np.median(upd)), "update_wall_us_profiling2": 1e6 * float(np.median(upd_wall))}
    if dense:
        dims = np.where(spec.node_type == synth.NODE_POSE, 6, 3)
        starts = np.concatenate([[0], np.cumsum(dims)])
        H = np.zeros((starts[-1], starts[-1]))
        for k, f in enumerate(fid):
            J, _ = g.eval_factor(int(f))
            a, b = spec.f_nodes[k]
            cols = list(range(starts[a], starts[a] + dims[a])) + (list(range(starts[b], starts[b] + dims[b])) if b >= 0 else [])
            H[np.ix_(cols, cols)] += J.T @ J
        t0 = time.perf_counter(); np.linalg.inv(H); res["cpu_dense_inverse_s"] = time.perf_counter() - t0
        res["cpu_dense_dim"] = int(starts[-1])
    g.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default="")
    ap.add_argument("--graphs", default="c2,c3")
    a = ap.parse_args()
    out = []
    for name in a.graphs.split(","):
        spec = synth.corridor() if name == "c2" else synth.manhattan_rooms()
        r = bench(name, spec, a.reps, dense=name == "c2")
        print(json.dumps(r)); out.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
