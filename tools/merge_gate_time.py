"""Time of pps_merge_gate: all planes of corridor_60_14 (14 planes, 91 pairs) and of C2 (corridor, 1 000 poses, 200 planes: 19 900 pairs),
after one optimisation and one recovery each.

  python tools/merge_gate_time.py [--reps 21] [--out profiles/merge_gate_times.json]

Reports the device seconds around the call's two kernels (pps_merge_gate_last) -- median, min, max over the repetitions after one warm-up
call --, the launch count, the pairs without a positive definite S and the host wall time of a call with and without the n x n download.
A record, not a pass / fail check.
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


def measure(name, spec, reps):
    g = P.Graph(); nid, _ = spec.replay(g)
    planes = [int(n) for n, t in zip(nid, spec.node_type) if t != synth.NODE_POSE]
    g.batch_optimize(); g.cov_recover()
    g.merge_gate(planes)                                   # warm-up: buffers, events
    dev, wall, wall_no = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter(); d2, best, pairs = g.merge_gate(planes); wall.append(time.perf_counter() - t0)
        sec, launches, not_pd = g.merge_gate_last(); dev.append(sec)
        t0 = time.perf_counter(); g.merge_gate(planes, want_d2=False); wall_no.append(time.perf_counter() - t0)
    n = len(planes)
    rec = {"graph": name, "n_planes": n, "n_pairs": n * (n - 1) // 2, "reps": reps, "launches": launches, "n_not_pd": not_pd,
           "kernel_sec_median": float(np.median(dev)), "kernel_sec_min": float(np.min(dev)), "kernel_sec_max": float(np.max(dev)),
           "wall_sec_median": float(np.median(wall)), "wall_sec_median_without_d2": float(np.median(wall_no)), "pairs_below_7.815": int(len(pairs)),
           "recover_sec": g.cov_last_times()[0], "finite": bool(np.all(np.isfinite(d2)))}
    g.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    recs = [measure("corridor_60_14", synth.corridor(60, 14, seed=7), a.reps), measure("c2_corridor_1000", synth.corridor(), a.reps)]
    for r in recs:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
