"""Time of pps_loop_gate: 1, 64 and 4 096 candidates on a band graph (band_60p_40l of tests/linsolve_helpers.py: 60 poses, 40 loop
closures, after pps_cov_recover) and on a dense-front graph (dense_64p_200l: 64 poses, 200 loop closures, after pps_cov_factor), after one
optimisation each.

  python tools/loop_gate_time.py [--reps 11] [--out profiles/loop_gate_times.json] [--note "which commit the run was made on"]

The candidates are random pose pairs with the relative pose of the two estimates as their measurement; every pose of the graph is in the
list from 64 candidates on, so the walk launch does the same work for 64 and for 4 096.  Reports the device seconds around the call's two
kernels (pps_loop_gate_last) -- median, min, max over the repetitions after one warm-up call --, the launch count, the candidates without a
positive definite S and the host wall time of a call with and without the n x 36 download of S.  A record, not a pass / fail check.
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
from linsolve_helpers import loop_graph  # noqa: E402
from pop_up_slam_amd import synth  # noqa: E402

COUNTS = (1, 64, 4096)


def measure(name, spec, recover, reps):
    g = P.Graph(jacobian_mode=1); nid, _ = spec.replay(g)
    poses = [int(n) for n, t in zip(nid, spec.node_type) if t == synth.NODE_POSE]
    g.batch_optimize()
    g.cov_recover() if recover else g.cov_factor()
    est = {n: g.get_pose(n) for n in poses}
    rng = np.random.default_rng(1)
    recs = []
    for n in COUNTS:
        ia = rng.choice(poses, n); ib = np.array([rng.choice([p for p in poses if p != a]) for a in ia])
        meas = np.array([synth.pose_vector(synth.pose_ominus(est[b], est[a])) for a, b in zip(ia, ib)])
        sq = np.tile(synth._ut_diag([4.0] * 3 + [20.0] * 3), (n, 1))
        g.loop_gate(ia, ib, meas, sq, want_S=True)              # warm-up: buffers, events
        dev, wall, wall_s = [], [], []
        for _ in range(reps):
            t0 = time.perf_counter(); d2, _, acc = g.loop_gate(ia, ib, meas, sq); wall.append(time.perf_counter() - t0)
            sec, launches, not_pd = g.loop_gate_last(); dev.append(sec)
            t0 = time.perf_counter(); g.loop_gate(ia, ib, meas, sq, want_S=True); wall_s.append(time.perf_counter() - t0)
        recs.append({"graph": name, "recovery": "pps_cov_recover" if recover else "pps_cov_factor", "n_candidates": n,
                     "n_distinct_poses": int(len(set(ia.tolist()) | set(ib.tolist()))), "reps": reps, "launches": launches, "n_not_pd": not_pd,
                     "kernel_sec_median": float(np.median(dev)), "kernel_sec_min": float(np.min(dev)), "kernel_sec_max": float(np.max(dev)),
                     "wall_sec_median": float(np.median(wall)), "wall_sec_median_with_S": float(np.median(wall_s)), "accepted_at_12.592": int(len(acc)),
                     "finite": bool(np.all(np.isfinite(d2)))})
    g.close()
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default=None)
    ap.add_argument("--note", default="", help="goes into the file as it is: the commit of the run")
    a = ap.parse_args()
    recs = measure("band_60p_40l", loop_graph(60, 40), True, a.reps) + measure("dense_64p_200l", loop_graph(64, 200), False, a.reps)
    for r in recs:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/loop_gate_time.py", "note": a.note, "records": recs}, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
