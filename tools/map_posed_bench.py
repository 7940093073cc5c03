"""Posed build (pps_map_build_posed) next to pps_map_build on the store of tools/map_bench.py.

The first N frames of the config-5 sequence (pipeline.popup_sequence, 640 x 480) run through the frame loop at step 1 and 2 and fill the
map the pipeline keeps; every frame is registered with its pose node, so every point of the posed build is moved.  On that store and the
selection of every chunk: the device seconds of pps_map_build, --repeats times -- the yardstick, a kernel this call does not change --,
then of pps_map_build_posed (motion kernel and build kernel) as often.  Both builds read 16 B and write 16 B per point.

The expectation that is checked: the posed kernel stays bandwidth-bound, i.e. its median is within the spread of the plain timings
(max - min) plus 10 % for the table reads of the plain median.  Writes profiles/map_posed_bench.json.

    python tools/map_posed_bench.py [--frames 200] [--repeats 5] [--out profiles/map_posed_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pop_up_slam_amd import pipeline             # noqa: E402


def run(frames, step, repeats, width=640, height=480):
    pl, g, pp, stats = pipeline.gpu_pipeline(width=width, height=height, step=step, map_points=len(frames) * (width * height // (step * step)))
    m = stats["map"]
    for fr in frames:
        pl.process(fr)
    g.batch_optimize()
    assert np.all(m.frames()["pose_id"] >= 0)
    m.build(); m.build(posed=True)                       # (first calls allocate)
    plain, posed, motion = [], [], []
    for _ in range(repeats):
        n_pts, n_chunks = m.build()
        plain.append(m.last_times()[1])
    for _ in range(repeats):
        assert m.build(posed=True) == (n_pts, n_chunks)
        last = m.posed_last()
        assert last["n_unposed_frames"] == 0
        motion.append(last["sec"][0]); posed.append(last["sec"][1])
    head = m.download(1, 0, min(n_pts, 1 << 20))
    d = np.stack([head[k] for k in "xyz"])
    p_med, q_med = float(np.median(plain)), float(np.median(posed))
    margin = (max(plain) - min(plain)) + 0.10 * p_med
    out = dict(step=step, frames=len(frames), points=n_pts, chunks=n_chunks, motion_rows=len(m.frame_motions()[1]),
               build_seconds=plain, build_seconds_median=p_med, posed_build_seconds=posed, posed_build_seconds_median=q_med,
               motion_seconds_median=float(np.median(motion)),
               build_bytes_per_s=32.0 * n_pts / p_med if p_med > 0 else None, posed_bytes_per_s=32.0 * n_pts / q_med if q_med > 0 else None,
               posed_over_build=q_med / p_med if p_med > 0 else None, margin_seconds=margin, within_margin=bool(q_med <= p_med + margin),
               finite=bool(np.isfinite(d).all()))
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_posed_bench.json"))
    a = ap.parse_args()
    frames = pipeline.popup_sequence(n_frames=a.frames)
    res = dict(tool="tools/map_posed_bench.py", width=640, height=480, repeats=a.repeats, runs=[run(frames, step, a.repeats) for step in (1, 2)])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
