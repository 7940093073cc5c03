"""Dense map on the device against the route a caller had to take before (download, host split, pps_reproject_points).

The first N frames of the config-5 sequence (pipeline.popup_sequence, 640 x 480) run through the frame loop at step 1 and 2.  Per frame:
device seconds of the pps_map_add_frame kernels next to pps_popup_last_kernel_time of the same frame (the pop-up kernel is the yardstick
the compaction is compared with), and the wall time of the call next to download + numpy split.  At the end: pps_map_build over the
whole store (points, device seconds, 32 B x points / seconds as a fraction of 8 TB/s -- below a 256 MB store that is cache bandwidth, not
HBM) next to pps_reproject_points over the host copy.  Both routes must give the same map.  Writes profiles/map_bench.json.

    python tools/map_bench.py [--frames 200] [--out profiles/map_bench.json]
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

import pop_up_slam_amd as P                      # noqa: E402
from pop_up_slam_amd import pipeline             # noqa: E402

HBM_BYTES_PER_S = 8e12


def run(frames, step, width=640, height=480):
    pl, g, pp, stats = pipeline.gpu_pipeline(width=width, height=height, step=step)
    pp.set_outputs(depth=False, plane_id=True)                     # the map partitions the cloud by the plane-id map
    m = P.Map(g, len(frames) * (width * height // (step * step)))
    host_chunks, host_ids = [], []
    add_s, popup_s, add_wall, host_wall = [], [], [], []
    for k, fr in enumerate(frames):
        pl.process(fr)
        ids = [pl.landmarks[key] for key in ["g"] + list(fr.ids)]
        popup_s.append(pp.last_kernel_time())
        t0 = time.perf_counter()
        counts = m.add_frame(pp, k, ids)
        add_wall.append(time.perf_counter() - t0)
        add_s.append(m.last_times()[0])
        # the route without the map: the cloud and the plane-id map come to the host and are split there
        t0 = time.perf_counter()
        c = np.zeros(width * height, dtype=P.POINT_DTYPE); p = np.zeros(width * height, dtype=np.int32)
        pp._ck(pp.L.pps_popup_download(pp.h, None, c.ctypes.data_as(C.c_void_p), None, p.ctypes.data_as(C.POINTER(C.c_int32))))
        valid = ((c["rgba"] >> 24) & 1) == 1
        for j, lm in enumerate(ids):
            ch = c[valid & (p == j)]
            host_chunks.append(ch); host_ids.append(np.full(len(ch), lm, dtype=np.int32))
        host_wall.append(time.perf_counter() - t0)
        assert [len(x) for x in host_chunks[-len(ids):]] == list(counts)
    g.batch_optimize()
    t0 = time.perf_counter()
    n_pts, n_chunks = m.build()
    build_wall = time.perf_counter() - t0
    build_s = m.last_times()[1]
    pts = np.concatenate(host_chunks); lm = np.concatenate(host_ids)
    t0 = time.perf_counter()
    xyz = g.reproject_points(lm, np.stack([pts["x"], pts["y"], pts["z"]], axis=1))
    host_build_wall = time.perf_counter() - t0
    got = m.download(1)
    same = (len(got) == len(pts) and np.array_equal(np.stack([got["x"], got["y"], got["z"]], axis=1).view(np.uint32), xyz.view(np.uint32))
            and np.array_equal(got["rgba"], pts["rgba"]))
    store_bytes = 16 * n_pts
    med = lambda a: float(np.median(a))
    return {
        "step": step, "frames": len(frames), "width": width, "height": height,
        "points": int(n_pts), "chunks": int(n_chunks), "store_bytes": int(store_bytes), "store_exceeds_256MB": bool(store_bytes > 256e6),
        "add_frame_kernel_s_median": med(add_s), "add_frame_kernel_s_max": float(np.max(add_s)),
        "popup_kernel_s_median": med(popup_s), "add_over_popup_median": med(np.array(add_s) / np.array(popup_s)),
        "add_frame_wall_s_median": med(add_wall), "host_download_split_wall_s_median": med(host_wall),
        "build_kernel_s": build_s, "build_wall_s": build_wall,
        "build_bytes_per_s": 32.0 * n_pts / build_s if build_s > 0 else None,
        "build_fraction_of_8TBps": 32.0 * n_pts / build_s / HBM_BYTES_PER_S if build_s > 0 else None,
        "host_route_reproject_wall_s": host_build_wall,
        "host_route_total_wall_s": float(np.sum(host_wall)) + host_build_wall,
        "device_route_total_wall_s": float(np.sum(add_wall)) + build_wall,
        "same_map_as_host_route": bool(same),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_bench.json"))
    a = ap.parse_args()
    frames = pipeline.popup_sequence(n_frames=a.frames)
    res = {"what": "tools/map_bench.py: pps_map against download + host split + pps_reproject_points, config-5 sequence",
           "runs": [run(frames, step) for step in (1, 2)]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    assert all(r["same_map_as_host_route"] for r in res["runs"])


if __name__ == "__main__":
    main()
