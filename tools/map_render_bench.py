"""Rendered view (pps_map_render) of the grid map of tools/map_grid_bench.py.

The first N frames of the config-5 sequence (pipeline.popup_sequence, 640 x 480) run through the frame loop at step 1 and fill a store; the
2 cm grid is built from it (the workload of profiles/map_grid_bench.json).  Then 640 x 480 views from three poses of the drive -- its first
frame, its middle and its last -- at reach 0, 1 and 2: the device seconds of the render kernel per view (median of --repeats renders) and
the pixels hit.  The one-time slot-table launch is measured as the difference between the first render after a fresh grid (two kernels in
the timed span) and the same 1 x 1 view rendered again (one kernel).  For context, on the same run: the wall time of pps_map_grid_download
of all cells.  Writes profiles/map_render_bench.json.

    python tools/map_render_bench.py [--frames 200] [--repeats 5] [--out profiles/map_render_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pop_up_slam_amd as P                      # noqa: E402
from pop_up_slam_amd import pipeline, synth      # noqa: E402

CELL = 0.02
REACHES = (0, 1, 2)


def run(frames, repeats, width=640, height=480, step=1):
    pl, g, pp, stats = pipeline.gpu_pipeline(width=width, height=height, step=step)
    pp.set_outputs(depth=False, plane_id=True)
    m = P.Map(g, len(frames) * (width * height // (step * step)))
    for k, fr in enumerate(frames):
        pl.process(fr)
        m.add_frame(pp, k, [pl.landmarks[key] for key in ["g"] + list(fr.ids)])
    g.batch_optimize()
    invK = np.linalg.inv(synth.K_TUM).astype(np.float32)
    poses = {name: synth.T_from_pose(frames[k].true_pose).astype(np.float32) for name, k in (("first", 0), ("middle", len(frames) // 2), ("last", len(frames) - 1))}
    # the slot table: a fresh grid, then the smallest view twice
    slot_s = []
    for _ in range(repeats):
        m.build_grid(cell=CELL, max_cells=1 << 30)
        a = m.render(1, 1, invK, poses["first"], reach=0)["totals"]
        b = m.render(1, 1, invK, poses["first"], reach=0)["totals"]
        assert (a["launches"], b["launches"]) == (2, 1)
        slot_s.append(a["sec"] - b["sec"])
    info = m.grid_info()
    boxes = m.grid_planes()
    views = []
    for name, T in poses.items():
        for reach in REACHES:
            secs, n_hit = [], None
            for _ in range(repeats):
                t = m.render(width, height, invK, T, reach=reach)["totals"]
                assert t["launches"] == 1
                secs.append(t["sec"]); n_hit = t["n_hit"]
            views.append(dict(pose=name, reach=reach, kernel_us=1e6 * float(np.median(secs)), n_hit=int(n_hit), n_planes=t["n_planes"]))
    down = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        pts, counts, ij, src = m.grid_download()
        down.append(time.perf_counter() - t0)
    out = dict(step=step, frames=len(frames), cell=CELL, cells=info["n_cells"], box_cells=int(boxes["ni"].astype(np.int64) @ boxes["nj"]),
               planes=info["n_planes"], grid_call_seconds=info["sec"][3], slot_table_us=1e6 * float(np.median(slot_s)), views=views,
               grid_download_all_cells_wall_us=1e6 * float(np.median(down)), grid_download_bytes=int(pts.nbytes + counts.nbytes + ij.nbytes + src.nbytes))
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_render_bench.json"))
    a = ap.parse_args()
    frames = pipeline.popup_sequence(n_frames=a.frames)
    res = dict(tool="tools/map_render_bench.py", width=640, height=480, repeats=a.repeats, run=run(frames, a.repeats))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
