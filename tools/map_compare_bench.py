"""A pop-up frame against the rendered map view (pps_map_compare), on the workload of tools/map_render_bench.py.

The first N frames of the config-5 sequence (pipeline.popup_sequence, 640 x 480) run through the frame loop at step 1 and fill a store; the
2 cm grid is built from it.  The view is rendered from the last pose at reach 0 and compared with that pose's own pop-up frame, which is
still the last run of the pop-up context.  After one warm-up call of both: --repeats times a render and a comparison, the device seconds
of each (HIP events around their kernels) taken in the SAME run, so k_render at reach 0 is the yardstick of the comparison.  Recorded
with the medians: the pairs and the class counts.  For context: the wall time of the host route -- both sides downloaded and compared with
the numpy statement of tests/compare_helpers.py, whose result must be the device's.  Writes profiles/map_compare_bench.json.

    python tools/map_compare_bench.py [--frames 200] [--repeats 5] [--out profiles/map_compare_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pop_up_slam_amd as P                      # noqa: E402
from pop_up_slam_amd import pipeline, synth      # noqa: E402
from compare_helpers import TOTAL_KEYS, ref_compare  # noqa: E402

CELL = 0.02
TOL = 0.05


def run(frames, repeats, width=640, height=480, step=1):
    pl, g, pp, stats = pipeline.gpu_pipeline(width=width, height=height, step=step)
    pp.set_outputs(depth=False, plane_id=True)
    m = P.Map(g, len(frames) * (width * height // (step * step)))
    for k, fr in enumerate(frames):
        pl.process(fr)
        m.add_frame(pp, k, [pl.landmarks[key] for key in ["g"] + list(fr.ids)])
    g.batch_optimize()
    nplanes = len(frames[-1].ids) + 1
    invK = np.linalg.inv(synth.K_TUM).astype(np.float32)
    T = synth.T_from_pose(frames[-1].true_pose).astype(np.float32)
    m.build_grid(cell=CELL, max_cells=1 << 30)
    m.render(width, height, invK, T, reach=0)                            # warm-up: the slot table, the images, the compare buffers
    m.compare(pp, nplanes, TOL)
    render_s, compare_s = [], []
    for _ in range(repeats):
        t = m.render(width, height, invK, T, reach=0)["totals"]
        assert t["launches"] == 1
        render_s.append(t["sec"])
        rec = m.compare(pp, nplanes, TOL)
        compare_s.append(m.compare_info()["sec"])
    tot, pairs = m.compare_info(), m.compare_pairs()
    host = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        cloud = np.zeros(width * height, dtype=P.POINT_DTYPE); pid = np.zeros(width * height, dtype=np.int32)      # (the depth output is off)
        pp._ck(pp.L.pps_popup_download(pp.h, None, cloud.ctypes.data_as(C.c_void_p), None, pid.ctypes.data_as(C.POINTER(C.c_int32))))
        view = m.render_download()
        want = ref_compare(view["plane_id"], m.grid_planes(), m.grid_plane_eq(), cloud, pid, nplanes, TOL)
        host.append(time.perf_counter() - t0)
    assert {k: tot[k] for k in TOTAL_KEYS} == want["totals"] and pairs.tobytes() == want["pairs"].tobytes() and rec.tobytes() == want["planes"].tobytes()
    out = dict(step=step, frames=len(frames), cell=CELL, cells=m.grid_info()["n_cells"], reach=0, tol=TOL, nplanes=nplanes, n_rows=tot["n_rows"],
               compare_kernels_us=1e6 * float(np.median(compare_s)), compare_kernels_us_all=[1e6 * s for s in compare_s], launches=tot["launches"],
               render_kernel_us=1e6 * float(np.median(render_s)), render_kernel_us_all=[1e6 * s for s in render_s],
               n_pairs=tot["n_pairs"], classes={k: tot[k] for k in ("n_both", "n_frame_only", "n_view_only", "n_neither", "n_bad_id")},
               best=[dict(frame_plane=k, plane_id=int(p["best_plane_id"]), n_valid=int(p["n_valid"]), n_new=int(p["n_new"]), best_n=int(p["best_n"]),
                          best_agree=int(p["best_agree"])) for k, p in enumerate(rec)],
               pairs=[dict(frame_plane=int(p["frame_plane"]), plane_id=int(p["plane_id"]), n=int(p["n"]), n_agree=int(p["n_agree"]),
                           mean_m=float(p["sum_q"]) / (4096.0 * float(p["n"])), rms_m=float(np.sqrt(float(p["sum_q2"]) / float(p["n"])) / 4096.0)) for p in pairs],
               host_route_wall_us=1e6 * float(np.median(host)), host_route_download_bytes=int(cloud.nbytes + pid.nbytes + sum(v.nbytes for v in view.values())))
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_compare_bench.json"))
    a = ap.parse_args()
    frames = pipeline.popup_sequence(n_frames=a.frames)
    res = dict(tool="tools/map_compare_bench.py", width=640, height=480, repeats=a.repeats, run=run(frames, a.repeats))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
