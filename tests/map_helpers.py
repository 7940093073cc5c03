"""What tests/test_host_map.py and tests/test_gpu_map.py share: the references the dense map is compared with.  None of it calls the
code under test."""
import numpy as np


def ref_select(chunks, counter, every_frame):
    """main_3d.cpp:538-562, loop for loop; being_tracked_times of a landmark = the chunks that belong to it"""
    tracked = {}
    for c in chunks:
        tracked[int(c["plane_id"])] = tracked.get(int(c["plane_id"]), 0) + 1
    keep = []
    for c in chunks:
        frame_ind, frame_sequ_id, tracked_times = int(c["frame"]), int(c["frame_seq_id"]), tracked[int(c["plane_id"])]
        k = True
        if not every_frame:
            if frame_sequ_id <= counter - 10:
                if frame_ind % 3 != 0:
                    k = False
            else:
                if frame_ind % 2 != 0:
                    k = False
        if frame_sequ_id <= counter - 15 and tracked_times < 10:
            k = False
        if frame_sequ_id <= counter - 8 and tracked_times < 5:
            k = False
        if frame_sequ_id <= counter - 4 and tracked_times < 2:
            k = False
        keep.append(k)
    return np.array(keep, dtype=bool)


def project_to_plane(abcd, xyz32):
    """Plane3d::project_to_plane (src/isam_plane3d.h:173-178) in fp64 on fp32 points: x - n (n . x - d), n = abc / |abc|, d = -d4 / |abc|"""
    x = xyz32.astype(np.float64)
    l = np.linalg.norm(abcd[:3]); n = abcd[:3] / l; d = -abcd[3] / l
    return x - np.outer(x @ n - d, n)


def assert_within_one_ulp(got32, want64):
    w32 = want64.astype(np.float32)
    lo = np.nextafter(w32, np.float32(-np.inf)); hi = np.nextafter(w32, np.float32(np.inf))
    assert np.all((got32 >= lo) & (got32 <= hi)), float(np.max(np.abs(got32.astype(np.float64) - want64)))


def split_frame(cloud, pid, k):
    """the chunk of frame plane k: the valid points whose plane-id pixel is k, in raster order (boolean indexing keeps it)"""
    c = cloud.reshape(-1); valid = ((c["rgba"] >> 24) & 1) == 1
    return c[valid & (pid.reshape(-1) == k)]


def raw16(points):
    """points as rows of 16 raw bytes: comparisons are on the records, not on float values (NaN, -0.0)"""
    return np.ascontiguousarray(points).view(np.uint8).reshape(-1, 16)


def xyz_of(points):
    return np.stack([points["x"], points["y"], points["z"]], axis=1)
