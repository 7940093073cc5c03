"""What tests/test_host_map.py, tests/test_gpu_map.py and tests/test_gpu_map_shapes.py share: the references the dense map is compared
with, and the flat frames (generators and the properties asserted of them) the kernels are fed.  None of it calls the code under test."""
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


def kept_key(cloud, pid, nplanes):
    """per pixel of a flat frame the plane its point is kept in, -1 if it is dropped: valid bit (bit 24 of rgba) and 0 <= id < nplanes"""
    c = cloud.reshape(-1); p = pid.reshape(-1)
    valid = ((c["rgba"] >> 24) & 1) == 1
    return np.where(valid & (p >= 0) & (p < nplanes), p, -1)


def split_flat(cloud, pid, nplanes):
    """split_frame for flat arrays and every plane at once: the chunk of each frame plane k = 0 .. nplanes-1, raster order kept"""
    c = cloud.reshape(-1); key = kept_key(c, pid, nplanes)
    return [c[key == k] for k in range(nplanes)]


MAP_THREADS = 256


def tiling(npx):
    """(wt, nT, seg) as csrc/pps_map.h and k_map_scan state them: 256 pixels per wave tile until that would pass 8192 tiles, then the
    least multiple of 64 that stays below; seg tiles per thread of the scan"""
    wt = 256
    if -(-npx // wt) > 8192:
        wt = -(-(-(-npx // 8192)) // 64) * 64
    nT = -(-npx // wt)
    return wt, nT, -(-nT // MAP_THREADS)


def random_points(rng, n):
    """n records with random coordinates and colours, every valid bit set"""
    pts = np.zeros(n, dtype=np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("rgba", "<u4")]))
    for name in "xyz":
        pts[name] = (rng.normal(size=n) * 5).astype(np.float32)
    pts["rgba"] = rng.integers(0, 1 << 32, size=n, dtype=np.uint32) | np.uint32(1 << 24)
    return pts


def _some_invalid(rng, cloud, p_valid):
    """clears the valid bit of 1 - p_valid of the pixels; half of those keep bits above it (they do not make a point valid)"""
    n = len(cloud)
    invalid = rng.random(n) >= p_valid
    high = rng.integers(0, 2, size=n, dtype=np.uint32) << 25
    cloud["rgba"][invalid] = (cloud["rgba"][invalid] & np.uint32(0x00FFFFFF)) | high[invalid]
    return cloud


def runs_frame(rng, npx, nplanes, p_valid=0.7):
    """flat frame: equal plane ids in runs of 1 .. 13 pixels, like polygons give them, drawn from -1 (gaps) .. nplanes + 1 (ids past
    nplanes: another frame's leftovers), p_valid of the pixels valid"""
    n_runs = npx // 4 + 16
    pid = np.repeat(rng.integers(-1, nplanes + 2, size=n_runs), rng.integers(1, 14, size=n_runs))[:npx].astype(np.int32)
    assert pid.size == npx
    return _some_invalid(rng, random_points(rng, npx), p_valid), pid


def confetti_frame(rng, npx, nplanes, p_valid=0.7):
    """flat frame: an independent key per pixel, from the same range as runs_frame"""
    pid = rng.integers(-1, nplanes + 2, size=npx).astype(np.int32)
    return _some_invalid(rng, random_points(rng, npx), p_valid), pid


def batch_keys(cloud, pid, nplanes):
    """kept keys per aligned batch of 64 pixels (what one turn of a wave's loop sees); the tail batch is padded with -1.  Exact while the
    wave tile is a multiple of 64 pixels, which every tiling is."""
    key = kept_key(cloud, pid, nplanes)
    pad = (-len(key)) % 64
    return np.concatenate([key, np.full(pad, -1, dtype=key.dtype)]).reshape(-1, 64)


def distinct_per_batch(cloud, pid, nplanes):
    """distinct kept planes in every aligned 64-pixel batch = turns of the `while (rem)` loop for that batch"""
    return np.array([len(np.unique(b[b >= 0])) for b in batch_keys(cloud, pid, nplanes)])


def wave_pattern_frame(rng):
    """165 pixels, 65 planes.  Batch 0: a permutation of planes 0 .. 63, every pixel valid -- 64 turns of the loop, every lane a leader
    once.  Batch 1: the only kept pixel is lane 63 with plane 64 (the other lanes: valid pixels with ids outside the frame's planes, and
    invalid pixels with ids inside).  Then a tail of 37 independent pixels.  Asserted here, from the arrays."""
    cloud, pid = confetti_frame(rng, 165, 65, p_valid=0.8)
    cloud["rgba"][:64] |= np.uint32(1 << 24)
    pid[:64] = rng.permutation(64)
    lanes = np.arange(64)
    pid[64:128] = np.where(lanes % 2 == 0, rng.choice([-1, 65, 66], size=64), rng.integers(0, 65, size=64))
    cloud["rgba"][64:128] = np.where(lanes % 2 == 0, cloud["rgba"][64:128] | np.uint32(1 << 24), cloud["rgba"][64:128] & np.uint32(0xFEFFFFFF))
    pid[127] = 64; cloud["rgba"][127] |= np.uint32(1 << 24)
    keys = batch_keys(cloud, pid, 65)
    assert sorted(keys[0]) == list(range(64))
    assert np.all(keys[1][:63] == -1) and keys[1][63] == 64
    assert np.any(pid[64:127][((cloud["rgba"][64:127] >> 24) & 1) == 0] >= 0)     # ids that would count if the valid bit did not
    return cloud, pid


def workgroup_windows(counts):
    """For the build of chunks with these counts (selected ones, empty ones included): per workgroup of 256 output points
    (starts inside a chunk and not on its first point, distinct chunks its points lie in)."""
    c = np.asarray(counts, dtype=np.int64); c = c[c > 0]
    off = np.concatenate([[0], np.cumsum(c)])
    out = []
    for first in range(0, int(off[-1]), MAP_THREADS):
        last = min(first + MAP_THREADS, int(off[-1])) - 1
        c0 = int(np.searchsorted(off, first, side="right")) - 1
        c1 = int(np.searchsorted(off, last, side="right")) - 1
        out.append((bool(off[c0] != first), c1 - c0 + 1))
    return out
