"""Grid map (pps_map_build_grid) next to pps_map_build on the store of tools/map_bench.py.

The first N frames of the config-5 sequence (pipeline.popup_sequence, 640 x 480) run through the frame loop at step 1 and 2 and fill a
store.  Then, on that store and the selection of every chunk: the device seconds of pps_map_build -- the yardstick, a kernel this call
does not change --, and per cell edge (0.01, 0.02, 0.05 m) the three pass times and the whole call of pps_map_build_grid, points in and
cells out, with the vote pass in both forms (one atomic pair per run of lanes that share a cell / one per point, PPS_GRID_VOTE=direct).
Every figure is the median of --repeats calls.  Writes profiles/map_grid_bench.json.

    python tools/map_grid_bench.py [--frames 200] [--repeats 5] [--out profiles/map_grid_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pop_up_slam_amd as P                      # noqa: E402
from pop_up_slam_amd import pipeline             # noqa: E402

CELLS = (0.01, 0.02, 0.05)


def grid_times(m, cell, repeats, direct):
    if direct:
        os.environ["PPS_GRID_VOTE"] = "direct"
    try:
        secs = []
        for _ in range(repeats):
            m.build_grid(cell=cell, max_cells=1 << 30)
            secs.append(m.grid_info()["sec"])
    finally:
        os.environ.pop("PPS_GRID_VOTE", None)
    return [float(v) for v in np.median(np.array(secs), axis=0)], m.grid_info()


def run(frames, step, repeats, width=640, height=480):
    pl, g, pp, stats = pipeline.gpu_pipeline(width=width, height=height, step=step)
    pp.set_outputs(depth=False, plane_id=True)
    m = P.Map(g, len(frames) * (width * height // (step * step)))
    for k, fr in enumerate(frames):
        pl.process(fr)
        m.add_frame(pp, k, [pl.landmarks[key] for key in ["g"] + list(fr.ids)])
    g.batch_optimize()
    build_s = []
    for _ in range(repeats):
        n_pts, n_chunks = m.build()
        build_s.append(m.last_times()[1])
    build = float(np.median(build_s))
    out = dict(step=step, frames=len(frames), points=n_pts, chunks=n_chunks, build_seconds=build, cells=[])
    for cell in CELLS:
        sec, info = grid_times(m, cell, repeats, direct=False)
        sec_direct, info_direct = grid_times(m, cell, repeats, direct=True)
        assert info_direct["n_cells"] == info["n_cells"]
        boxes = m.grid_planes()
        out["cells"].append(dict(
            cell=cell, points_in=info["n_in"], dropped=info["n_dropped"], passed_through=info["n_passed_through"], planes=info["n_planes"],
            cells_out=info["n_cells"], box_cells=int(boxes["ni"].astype(np.int64) @ boxes["nj"]), launches=info["launches"],
            extent_seconds=sec[0], vote_seconds=sec[1], emission_seconds=sec[2], call_seconds=sec[3],
            vote_seconds_direct=sec_direct[1], call_seconds_direct=sec_direct[3],
            call_over_build=sec[3] / build if build > 0 else None, passes_over_build=(sec[0] + sec[1] + sec[2]) / build if build > 0 else None))
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_grid_bench.json"))
    a = ap.parse_args()
    frames = pipeline.popup_sequence(n_frames=a.frames)
    res = dict(tool="tools/map_grid_bench.py", width=640, height=480, repeats=a.repeats, runs=[run(frames, step, a.repeats) for step in (1, 2)])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
