"""Time of pps_cov_block: three queries on C2 (corridor, 1 000 poses) after one recovery, and the 16-pose joint on C3 (manhattan
rooms, 10 000 poses).

  python tools/cov_block_time.py [--reps 21] [--out profiles/cov_block_times.json] [--graphs c2,c3]

C2 queries: the joint of 16 poses spread evenly over the trajectory, the last pose against all planes, the first pose against the
last pose.  Per query: the median wall time of the C call itself (ctypes, buffers made beforehand: request upload, two launches, copy
back, synchronisation), the median device time between HIP events around the two kernels and the number of launches
(pps_cov_block_last), next to the device time of the pps_cov_recover of the same handle (pps_cov_last_times).  Records, not
thresholds: the selected inverse cannot answer these queries at all, so there is no ratio to hold them against."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pop_up_slam_amd as P
from pop_up_slam_amd import synth

_ip, _dp = C.POINTER(C.c_int), C.POINTER(C.c_double)


def time_query(g, name, rows, cols, reps):
    r = np.ascontiguousarray(rows, dtype=np.int32)
    c = None if cols is None else np.ascontiguousarray(cols, dtype=np.int32)
    out = np.zeros(36 * len(r) * (len(r) if c is None else len(c)))
    wall, dev, launches = [], [], 0
    for k in range(reps + 3):
        t0 = time.perf_counter()
        rc = g.L.pps_cov_block(g.h, len(r), r.ctypes.data_as(_ip), 0 if c is None else len(c), None if c is None else c.ctypes.data_as(_ip),
                               out.ctypes.data_as(_dp))
        t1 = time.perf_counter()
        if rc != P.PPS_OK:
            raise RuntimeError(f"pps_cov_block: {rc}")
        sec, launches = g.cov_block_last()
        if k >= 3:
            wall.append(t1 - t0); dev.append(sec)
    return {"query": name, "row_nodes": len(r), "col_nodes": len(r) if c is None else len(c), "call_wall_us": 1e6 * float(np.median(wall)),
            "kernels_device_us": 1e6 * float(np.median(dev)), "kernels_device_us_min_max": [1e6 * min(dev), 1e6 * max(dev)], "launches": launches}


def bench(name, spec, reps):
    g = P.Graph(); nid, _ = spec.replay(g)
    g.batch_optimize()
    for _ in range(3):
        g.cov_recover()
    rec_all, rec_pass = g.cov_last_times()
    poses = [int(n) for n, t in zip(nid, spec.node_type) if t == synth.NODE_POSE]
    planes = [int(n) for n, t in zip(nid, spec.node_type) if t != synth.NODE_POSE]
    spread = [poses[k] for k in np.linspace(0, len(poses) - 1, 16).astype(int)]
    queries = [("joint of 16 poses", spread, None)]
    if name == "c2":
        queries += [("last pose x all planes", [poses[-1]], planes), ("first pose x last pose", [poses[0]], [poses[-1]])]
    st = g.stats()
    res = {"graph": name, "poses": st["n_poses"], "planes": st["n_planes"], "fronts": st["n_fronts"], "levels": st["n_levels"], "reps": reps,
           "cov_recover_device_us": 1e6 * rec_all, "cov_pass_device_us": 1e6 * rec_pass,
           "queries": [time_query(g, q, r, c, reps) for q, r, c in queries]}
    g.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default="")
    ap.add_argument("--graphs", default="c2,c3")
    a = ap.parse_args()
    out = []
    for name in a.graphs.split(","):
        r = bench(name, synth.corridor() if name == "c2" else synth.manhattan_rooms(), a.reps)
        print(json.dumps(r)); out.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
