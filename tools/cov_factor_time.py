"""Times of pps_cov_factor: next to pps_cov_recover on C2 (band form), and on the full sphere2500 log (dense-front form) with one
pps_cov_block and one pps_assoc_gate behind it.

  python tools/cov_factor_time.py [--out profiles/cov_factor_times.json]

  C2 (corridor, 1 000 poses, 200 planes), after one optimisation: device seconds (pps_cov_last_times) of pps_cov_factor and of
      pps_cov_recover, whose root -> leaves pass the former leaves out
  sphere2500 (2 500 poses, 4 949 edges) plus 8 planes, each seen from three poses spread over the log, after batch_optimize:
      pps_cov_factor; pps_cov_block of (last pose, first pose); pps_assoc_gate of 1 measurement x the 8 planes (device seconds around
      the two kernels of each query, and the host wall time of the call)
Every figure is the median of 11 calls after two warm-up calls.  A record, not a pass / fail check.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pop_up_slam_amd as P  # noqa: E402
from pop_up_slam_amd import graphio, synth  # noqa: E402

WARM, REPS = 2, 11


def median_of(call, read):
    vals, wall = [], []
    for k in range(WARM + REPS):
        t0 = time.perf_counter(); call(); dt = time.perf_counter() - t0
        if k >= WARM:
            vals.append(read()); wall.append(dt)
    return float(np.median(vals)), float(np.median(wall))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rec = {"warm_ups": WARM, "reps": REPS}
    # ---- C2 ----
    g = P.Graph(); synth.corridor().replay(g)
    g.batch_optimize()
    fac, fac_wall = median_of(g.cov_factor, lambda: g.cov_last_times()[0])
    full, full_wall = median_of(g.cov_recover, lambda: g.cov_last_times()[0])
    rec["c2_corridor_1000"] = {"cov_factor_sec": fac, "cov_recover_sec": full, "cov_recover_level_pass_sec": g.cov_last_times()[1],
                               "cov_factor_wall_sec": fac_wall, "cov_recover_wall_sec": full_wall}
    g.close()
    # ---- sphere2500 ----
    spec = graphio.load_edge3_log(os.path.join(ROOT, "tests", "golden", "isam_data", "sphere2500.txt"))
    g = P.Graph(jacobian_mode=1); nid, _ = spec.replay(g)
    poses = [int(n) for n in nid]
    rng = np.random.default_rng(0)
    planes = []
    for k in range(8):
        n = rng.normal(size=3); n /= np.linalg.norm(n)
        pl = np.concatenate([n, [rng.uniform(20.0, 60.0)]]); pl /= np.linalg.norm(pl)
        planes.append(g.add_plane(pl))
        for p in (poses[(k * 97) % len(poses)], poses[(k * 311 + 800) % len(poses)], poses[(k * 53 + 1700) % len(poses)]):
            g.add_plane_obs(p, planes[-1], synth.plane_transform_to(pl, g.get_pose(p)), synth._ut_diag([20.0] * 3))
    it = g.batch_optimize()
    st = g.stats()
    fac, fac_wall = median_of(g.cov_factor, lambda: g.cov_last_times()[0])
    blk, blk_wall = median_of(lambda: g.cov_block([poses[-1]], [poses[0]]), lambda: g.cov_block_last()[0])
    meas = synth.plane_exmap(synth.plane_transform_to(g.get_plane(planes[0]), g.get_pose(poses[-1])), 0.05 * rng.normal(size=3))[None, :]
    W = synth._ut_diag([50.0] * 3)[None, :]
    out = {}
    gate, gate_wall = median_of(lambda: out.update(r=g.assoc_gate(poses[-1], meas, W, planes)), lambda: g.assoc_gate_last()[0])
    rec["sphere2500"] = {"poses": len(poses), "planes_added": len(planes), "max_front": st["max_front"], "lm_iterations": it,
                         "cov_factor_sec": fac, "cov_factor_wall_sec": fac_wall,
                         "cov_block_last_first_kernel_sec": blk, "cov_block_wall_sec": blk_wall, "cov_block_launches": g.cov_block_last()[1],
                         "assoc_gate_1x8_kernel_sec": gate, "assoc_gate_wall_sec": gate_wall, "assoc_gate_launches": g.assoc_gate_last()[1],
                         "finite": bool(np.all(np.isfinite(out["r"][0])))}
    g.close()
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
