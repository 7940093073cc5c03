"""GPU: the dense-map kernels (csrc/pps_map.hip) at the shapes a pop-up run does not produce -- every tiling regime of the partition, up
to 65 planes, the wave patterns of the ballot loop, and builds whose workgroups cross hundreds of chunks.  The frames go in through
pps_debug_map_add_points, which uploads host arrays and then runs pps_map_add_frame's own body; one test holds the hook to add_frame.

Expected values never come from the code under test: a chunk is the numpy stable split of the same arrays (map_helpers.split_flat), raw
record against raw record; a build is pps_reproject_points bit for bit and the numpy fp64 projection within one fp32 ulp
(test_gpu_map._check_build).  No number here is a measurement, and no tolerance is introduced.  Every case first asserts, from its inputs
alone, the property it exists for."""
import ctypes as C

import numpy as np
import pytest

import pop_up_slam_amd as P
from map_helpers import (batch_keys, confetti_frame, distinct_per_batch, kept_key, random_points, raw16, runs_frame, split_flat, tiling,
                         wave_pattern_frame, workgroup_windows)
from pop_up_slam_amd import synth
from test_gpu_map import _check_build, _check_store, _plane_graph, _popup, _pose

pytestmark = pytest.mark.gpu

VALID = np.uint32(1 << 24)


@pytest.fixture(scope="module")
def planes65(built):
    """one graph with 65 plane nodes for every test that only stores"""
    g, pl = _plane_graph(65)
    yield g, pl
    g.close()


def _add(m, frames, seq, cloud, pid, ids):
    """one frame through the hook; the counts against the numpy split; the frame is remembered for _check_store"""
    want = split_flat(cloud, pid, len(ids))
    counts = m.debug_add_points(cloud, pid, seq, ids)
    np.testing.assert_array_equal(counts, [len(want[k]) if ids[k] >= 0 else 0 for k in range(len(ids))])
    frames.append((seq, list(ids), want))
    return counts


# ---- tilings ------------------------------------------------------------------------------------------------------------------------
# npx: (wt, nT, seg, planes)
TILINGS = {
    1: (256, 1, 1, 7), 63: (256, 1, 1, 7), 64: (256, 1, 1, 7), 65: (256, 1, 1, 7), 255: (256, 1, 1, 7), 256: (256, 1, 1, 7),
    257: (256, 2, 1, 7),
    65536: (256, 256, 1, 7),             # seg = 1 with every scan thread busy
    65537: (256, 257, 2, 7),             # seg = 2: thread 128 holds one tile, the threads above it none
    307200: (256, 1200, 5, 9),           # the product's 640 x 480
    2097152: (256, 8192, 32, 5),         # the last frame with 256-pixel tiles
    2097153: (320, 6554, 26, 5),         # the first with larger ones
}


@pytest.mark.parametrize("pattern", ["runs", "confetti"])
@pytest.mark.parametrize("npx", sorted(TILINGS))
def test_partition_at_every_tiling(planes65, npx, pattern):
    g, pl = planes65
    wt, nT, seg, nplanes = TILINGS[npx]
    assert tiling(npx) == (wt, nT, seg)                                  # the regime, recomputed from the formulas
    assert wt % 64 == 0 and (nT - 1) * wt < npx <= nT * wt
    rng = np.random.default_rng(2 * npx + (pattern == "confetti"))
    cloud, pid = (runs_frame if pattern == "runs" else confetti_frame)(rng, npx, nplanes)
    pid[-1] = nplanes - 1; cloud["rgba"][-1] |= VALID                    # the frame's last pixel is kept: the last lane of the last tile works
    ids = list(pl[:nplanes]); ids[1] = -1
    key = kept_key(cloud, pid, nplanes)
    assert key[-1] == nplanes - 1
    if npx >= 255:
        invalid = ((cloud["rgba"] >> 24) & 1) == 0
        assert np.any(pid == -1) and np.any(pid >= nplanes) and np.any(invalid & (pid >= 0) & (pid < nplanes))
        assert np.any(invalid & ((cloud["rgba"] >> 25) != 0))            # bits above the valid bit on invalid pixels
        assert all(np.any(key == k) for k in range(nplanes))             # every plane has points, the skipped one too
        assert pattern == "confetti" or np.diff(np.flatnonzero(np.diff(pid) != 0)).max() >= 2       # runs of equal ids
    if nT > 1:
        per_tile = [np.count_nonzero(key[T * wt:(T + 1) * wt] >= 0) for T in (0, nT // 2, nT - 1)]
        assert all(n > 0 for n in per_tile)                              # first, middle and last tile keep points
    m = P.Map(g, npx + 63)
    frames = []
    c0, p0 = runs_frame(np.random.default_rng(5), 63, 3)                 # a small frame first: the bases are not 0, the count table grows
    _add(m, frames, 10, c0, p0, pl[:3])
    counts = _add(m, frames, 11, cloud, pid, ids)
    assert counts[1] == 0 and counts[nplanes - 1] >= 1
    _check_store(m, frames)
    m.close()


# ---- plane counts and wave patterns -------------------------------------------------------------------------------------------------
def _confetti65(rng, pl):
    """every plane index a pixel can hold; a batch with >= 32 turns of the loop; a batch that keeps nothing"""
    cloud, pid = confetti_frame(rng, 64 * 70 + 37, 65, p_valid=0.9)
    cloud["rgba"][640:704] = (cloud["rgba"][640:704] & np.uint32(0x00FFFFFF)) | np.uint32(0xFE000000)
    key = kept_key(cloud, pid, 65)
    assert sorted(np.unique(key[key >= 0])) == list(range(65))
    d = distinct_per_batch(cloud, pid, 65)
    assert d.max() >= 32 and d[10] == 0 and np.any(pid[640:704] >= 0)
    return cloud, pid, list(pl)


def _permutation_then_lane63(rng, pl):
    """64 turns in one batch, then a leader in lane 63 found in a mask whose only bit is bit 63 (asserted by wave_pattern_frame)"""
    cloud, pid = wave_pattern_frame(rng)
    keys = batch_keys(cloud, pid, 65)
    assert len(np.unique(keys[0])) == 64 and np.flatnonzero(keys[1] >= 0).tolist() == [63]
    return cloud, pid, list(pl)


def _single_points_at_the_ends(rng, pl):
    """plane 0's only point is pixel 0, plane 6's only point is the frame's last pixel"""
    npx = 1000
    cloud, pid = confetti_frame(rng, npx, 5)
    pid = np.where((pid == 0) | (pid >= 5), -1, pid).astype(np.int32)
    pid[0] = 0; pid[-1] = 6; cloud["rgba"][[0, -1]] |= VALID
    key = kept_key(cloud, pid, 7)
    assert np.flatnonzero(key == 0).tolist() == [0] and np.flatnonzero(key == 6).tolist() == [npx - 1] and npx % 64 != 0
    assert np.count_nonzero(key == 5) == 0 and np.count_nonzero(key == 3) > 10      # (and a plane between them without a point)
    return cloud, pid, list(pl[:7])


def _high_bits_on_invalid_pixels(rng, pl):
    cloud, pid = runs_frame(rng, 3000, 4, p_valid=0.5)
    invalid = ((cloud["rgba"] >> 24) & 1) == 0
    cloud["rgba"][invalid] |= np.uint32(0xFE000000)
    would = invalid & (pid >= 0) & (pid < 4)
    assert np.count_nonzero(would) > 500 and np.all((cloud["rgba"][would] >> 25) == 0x7F) and np.all(kept_key(cloud, pid, 4)[invalid] == -1)
    return cloud, pid, list(pl[:4])


def _skipped_first_and_last_plane(rng, pl):
    cloud, pid = confetti_frame(rng, 64 * 40 + 1, 65, p_valid=0.9)
    key = kept_key(cloud, pid, 65)
    assert np.count_nonzero(key == 0) > 0 and np.count_nonzero(key == 64) > 0       # they have points; none may be stored
    ids = list(pl); ids[0] = -1; ids[64] = -1
    return cloud, pid, ids


def _one_plane_all_valid(rng, pl):
    cloud = random_points(rng, 777); pid = np.zeros(777, dtype=np.int32)
    assert np.all(kept_key(cloud, pid, 1) == 0)
    return cloud, pid, [pl[0]]


def _nothing_valid(rng, pl):
    cloud, pid = runs_frame(rng, 2049, 3, p_valid=0.0)
    assert np.all(kept_key(cloud, pid, 3) == -1) and np.any((pid >= 0) & (pid < 3))
    return cloud, pid, list(pl[:3])


PATTERNS = [_confetti65, _permutation_then_lane63, _single_points_at_the_ends, _high_bits_on_invalid_pixels, _skipped_first_and_last_plane,
            _one_plane_all_valid, _nothing_valid]


@pytest.mark.parametrize("case", PATTERNS, ids=lambda f: f.__name__.strip("_"))
def test_plane_counts_and_wave_patterns(planes65, case):
    g, pl = planes65
    cloud, pid, ids = case(np.random.default_rng(PATTERNS.index(case) + 650), pl)
    m = P.Map(g, 2 * len(cloud))
    frames = []
    _add(m, frames, 3, cloud, pid, ids)
    _add(m, frames, 4, cloud[::-1].copy(), pid[::-1].copy(), ids)        # the same pixels in reverse raster order, behind the first frame
    _check_store(m, frames)
    m.close()


# ---- build windows ------------------------------------------------------------------------------------------------------------------
def _solvable_graph(n_planes):
    """65 plane landmarks the build can read the estimate of: every node carries a prior, nothing is optimised"""
    g = P.Graph()
    pose = g.add_pose([0, 0, 1, 0, 0, 0, 1])
    g.add_pose_prior(pose, np.zeros(6), synth._ut_diag([1.0] * 6))
    pl = []
    for i in range(n_planes):
        pl.append(g.add_plane([np.sin(i), np.cos(i), 0.1 * i, -1.0 - 0.1 * i]))
        g.add_plane_prior(pl[-1], g.get_plane(pl[-1]), synth._ut_diag([300.0] * 3))
    return g, pl


def _one_point_frame(rng, empty):
    """64 pixels: one point for every plane 0 .. 64 but `empty` (an empty chunk)"""
    order = rng.permutation([k for k in range(65) if k != empty]).astype(np.int32)
    return random_points(rng, 64), order


def test_build_windows_of_tiny_chunks(built):
    g, pl = _solvable_graph(65)
    rng = np.random.default_rng(4096)
    m = P.Map(g, 4096)
    frames = []
    rare = list(range(20, 25))                                           # frame planes whose landmarks are seen in the first block only
    _add(m, frames, 0, random_points(rng, 512), np.zeros(512, np.int32), [pl[0]])             # one chunk of 2 x 256 points
    for f in range(5):                                                   # 5 x (64 one-point chunks and an empty one)
        cloud, pid = _one_point_frame(rng, empty=7 * f + 3)
        _add(m, frames, 1 + f, cloud, pid, pl)
    _add(m, frames, 6, random_points(rng, 200), np.zeros(200, np.int32), [pl[3]])             # ends 8 points into a workgroup
    for f in range(4):
        cloud, pid = _one_point_frame(rng, empty=5 * f + 40)
        _add(m, frames, 7 + f, cloud, pid, [-1 if k in rare else pl[k] for k in range(65)])
    _check_store(m, frames)
    t = m.chunks()
    # the table, before any build: what each workgroup of the full build will see
    win = workgroup_windows(t["count"])
    assert t["count"][0] % 256 == 0 and np.all(t["count"][1:66][t["count"][1:66] > 0] == 1)
    assert win[2] == (False, 256)                                        # starts on a chunk's first point, 256 points in 256 chunks
    assert win[4][0] and win[4][1] >= 200                                # starts inside the 200-point chunk and crosses > 200 chunks
    assert np.count_nonzero(t["count"] == 0) == 9 and np.all(np.diff(np.flatnonzero(t["count"] == 0)) > 1)
    n_all = int(t["count"].sum())
    assert m.build() == (n_all, len(t))
    assert len(m.built_chunks()) == len(t)                               # empty chunks stay in the host table ...
    _check_build(g, m, t)                                                # ... and leave the device table (offsets and counts checked there)
    # a selection that drops chunks from the middle of a window: landmarks seen fewer than 6 times
    gate = P.map_select(100, every_frame=1, age=(-1000, -1000, -1000), min_tracked=(6, 6, 6))
    keep = P.map_select_host(t, gate)
    np.testing.assert_array_equal(keep, ~np.isin(t["plane_id"], [pl[k] for k in rare]))
    inner = np.flatnonzero(~keep)
    assert len(inner) == 25 and keep[0] and all(keep[i - 1] and keep[i + 5] for i in inner[::5])      # kept chunks on both sides
    assert workgroup_windows(t["count"][keep])[2] == (False, 256)
    assert m.build(gate) == (int(t["count"][keep].sum()), int(keep.sum()))
    _check_build(g, m, t[keep])
    # one landmark redirected, one removed without a successor: slot -1 inside a window of one-point chunks
    a, b, c = pl[30], pl[31], pl[50]
    m.redirect(b, a); g.remove_node(b); g.remove_node(c)
    t2 = m.chunks()
    np.testing.assert_array_equal(t2["plane_id"], np.where(t["plane_id"] == b, a, t["plane_id"]))
    gone = np.flatnonzero(t2["plane_id"] == c)
    assert len(gone) == 9 and np.all(t2["count"][gone] <= 1) and t2["count"][gone].sum() >= 7
    m.build()
    pts, ids, got = _check_build(g, m, t2)
    assert np.count_nonzero(ids == c) >= 7
    np.testing.assert_array_equal(raw16(got[ids == c]), raw16(pts[ids == c]))
    assert np.any(raw16(got[ids == a]) != raw16(pts[ids == a]))          # (the projection moves points: the check is not vacuous)
    m.close(); g.close()


def test_build_sizes_at_the_workgroup_edge(built):
    """n_out = 1 with one chunk; n_out a multiple of 256; that + 1"""
    g, pl = _solvable_graph(65)
    rng = np.random.default_rng(257)
    one = P.Map(g, 8)
    _add(one, [], 0, random_points(rng, 1), np.zeros(1, np.int32), [pl[9]])
    assert one.build() == (1, 1)
    _check_build(g, one, one.chunks())
    m = P.Map(g, 1024)
    frames = []
    for f in range(4):
        cloud, pid = _one_point_frame(rng, empty=64)
        _add(m, frames, f, cloud, pid, pl)
    assert m.info()["n_points"] == 256 and workgroup_windows(m.chunks()["count"]) == [(False, 256)]
    assert m.build() == (256, 260)
    _check_build(g, m, m.chunks())
    _add(m, frames, 4, random_points(rng, 1), np.zeros(1, np.int32), [pl[2]])
    assert workgroup_windows(m.chunks()["count"]) == [(False, 256), (False, 1)]
    assert m.build() == (257, 261)
    _check_build(g, m, m.chunks())
    _check_store(m, frames)
    one.close(); m.close(); g.close()


# ---- the hook against the shipped path ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("w,h", [(160, 120), (640, 480)])
def test_hook_stores_what_add_frame_stores(built, w, h, step):
    pp, K = _popup(w, h)
    g, pl = _plane_graph(4)
    shipped, hook = P.Map(g, w * h), P.Map(g, w * h)
    seg, polys, T = synth.corridor_frame(_pose(0), width=w, height=h, K=K)
    assert pp.run(seg, T, polys, step=step, depth_thre=10.0, ceiling_thre=2.5) > 0
    _, cloud, _, pid = pp.download()
    assert cloud.size == w * h == pid.size
    ids = [pl[0], pl[1], -1, pl[3]]
    c1 = shipped.add_frame(pp, 8, ids)
    c2 = hook.debug_add_points(cloud, pid, 8, ids)
    assert c1[0] > 0 and c1[1] > 0 and c1[3] > 0
    np.testing.assert_array_equal(c1, c2)
    np.testing.assert_array_equal(shipped.chunks(), hook.chunks())
    assert shipped.info() == hook.info()
    np.testing.assert_array_equal(raw16(shipped.download(0)), raw16(hook.download(0)))
    assert shipped.last_times()[0] > 0.0 and hook.last_times()[0] > 0.0
    if (w, h) == (640, 480):
        assert tiling(w * h) == (256, 1200, 5)                           # the product's frame: seg = 5 in the scan
    want = split_flat(cloud, pid, 4)
    for m in (shipped, hook):
        _check_store(m, [(8, ids, want)])
        m.close()


def test_hook_refusals_leave_the_map_usable(built):
    g, pl = _plane_graph(4)
    rng = np.random.default_rng(31)
    cloud, pid = runs_frame(rng, 1500, 4)
    want = split_flat(cloud, pid, 4)
    kept = sum(len(x) for x in want)
    assert kept > 400
    m = P.Map(g, 2 * kept - 1)                                           # room for the frame once, not twice
    L = P.lib()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    cids = (C.c_int * 4)(*pl)
    state = lambda: (m.info(), m.chunks().tobytes(), m.download(0).tobytes())

    def refused(fn, code):
        before = state()
        with pytest.raises(P.PpsError) as e:
            fn()
        assert e.value.code == code, e.value
        assert state() == before

    def raw_refused(*args):
        before = state()
        assert L.pps_debug_map_add_points(m.h, *args) == P.PPS_EINVAL
        assert state() == before

    for stored in (False, True):
        raw_refused(None, vp(pid), 1500, 0, 4, cids, None)
        raw_refused(vp(cloud), None, 1500, 0, 4, cids, None)
        raw_refused(vp(cloud), vp(pid), 1500, 0, 4, None, None)
        raw_refused(vp(cloud), vp(pid), 0, 0, 4, cids, None)
        raw_refused(vp(cloud), vp(pid), -1, 0, 4, cids, None)
        raw_refused(vp(cloud), vp(pid), (1 << 32) + 1500, 0, 4, cids, None)          # would be 1500 if it were cut to int
        raw_refused(vp(cloud), vp(pid), 1500, 0, -1, cids, None)
        refused(lambda: m.debug_add_points(cloud, pid, 0, list(pl) * 17), P.PPS_EINVAL)              # 68 planes
        refused(lambda: m.debug_add_points(cloud, pid, 0, [pl[0], 0, pl[2], pl[3]]), P.PPS_EINVAL)   # node 0 is a pose
        refused(lambda: m.debug_add_points(cloud, pid, 0, [pl[0], 77, pl[2], pl[3]]), P.PPS_EINVAL)
        refused(lambda: m.debug_add_points(cloud, pid, 0, [pl[0], -2, pl[2], pl[3]]), P.PPS_EINVAL)  # only -1 skips
        if not stored:
            assert m.info()["n_frames"] == 0 and m.build() == (0, 0)
            m.debug_add_points(cloud, pid, 0, pl)
            _check_store(m, [(0, pl, want)])
    refused(lambda: m.debug_add_points(cloud, pid, 1, pl), P.PPS_ENOMEM)                             # one point too many
    _check_store(m, [(0, pl, want)])
    ids = [pl[0], -1, pl[2], pl[3]]                                      # without plane 1 the frame fits
    assert len(want[1]) > 0
    m.debug_add_points(cloud, pid, 2, ids)
    _check_store(m, [(0, pl, want), (2, ids, want)])
    m.close(); g.close()
