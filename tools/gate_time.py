"""Time of pps_assoc_gate on C2 (corridor, 1 000 poses, 200 planes): the last pose against all planes x 6 measurements, after one
optimisation and one recovery.

  python tools/gate_time.py [--reps 21] [--out profiles/gate_times.json]

Reports the device seconds around the call's two kernels (pps_assoc_gate_last) -- median, min, max over the repetitions after one warm-up
call --, the launch count and the host wall time of a call.  A record, not a pass / fail check.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    spec = synth.corridor()
    g = P.Graph(); nid, _ = spec.replay(g)
    poses = [int(n) for n, t in zip(nid, spec.node_type) if t == synth.NODE_POSE]
    planes = [int(n) for n, t in zip(nid, spec.node_type) if t != synth.NODE_POSE]
    g.batch_optimize(); g.cov_recover()
    rng = np.random.default_rng(0)
    tq = g.get_pose(poses[-1])
    meas = np.array([synth.plane_exmap(synth.plane_transform_to(g.get_plane(planes[-1 - k]), tq), 0.05 * rng.normal(size=3)) for k in range(6)])
    W = np.tile(synth._ut_diag([50.0] * 3), (6, 1))
    g.assoc_gate(poses[-1], meas, W)                       # warm-up: buffers, events
    dev, wall = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter(); d2, best = g.assoc_gate(poses[-1], meas, W); wall.append(time.perf_counter() - t0)
        sec, launches = g.assoc_gate_last(); dev.append(sec)
    rec = {"graph": "c2_corridor_1000", "n_meas": 6, "n_planes": len(planes), "reps": a.reps, "launches": launches,
           "kernel_sec_median": float(np.median(dev)), "kernel_sec_min": float(np.min(dev)), "kernel_sec_max": float(np.max(dev)),
           "wall_sec_median": float(np.median(wall)), "recover_sec": g.cov_last_times()[0], "finite": bool(np.all(np.isfinite(d2)))}
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1); f.write("\n")
    g.close()


if __name__ == "__main__":
    main()
