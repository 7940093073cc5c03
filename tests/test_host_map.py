"""CPU: the dense map (include/pps.h: pps_map_*) before any kernel runs on a device.

  * pps_map_select_host against a Python restatement of the reference's publishing loop (main_3d.cpp:538-562);
  * the argument and state checks of every entry point, answered on the host (this suite runs without a device);
  * the kernels of csrc/pps_map.hip themselves, compiled for the host (tests/cpp/map_emu.cpp, one std::thread per GPU thread, barriers at
    the wave operations): the stable partition against numpy, the build against a numpy fp64 projection (1 fp32 ulp: the fp64 arithmetic
    differs by rounding order only, which can move the final fp32 rounding by at most one ulp); the tiling arithmetic; two tiles per
    scan thread, 64 distinct planes in one batch, a leader in lane 63, build windows of one-point chunks (the same frames run on the
    device in tests/test_gpu_map_shapes.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pop_up_slam_amd as P
from map_helpers import (assert_within_one_ulp, kept_key, project_to_plane, raw16, ref_select, split_flat, tiling, wave_pattern_frame,
                         workgroup_windows)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- selection --------------------------------------------------------------------------------------------------------------------
def random_table(rng, n_frames=40, n_planes=5, redirects=0):
    """a drive past landmarks: frame f sees the ground (landmark 0) and a window of wall landmarks that moves on; some walls are seen
    once or twice only; key frames are not every frame (frame_seq_id runs ahead of the frame index)"""
    rows, off, seq = [], 0, 0
    for f in range(n_frames):
        seq += int(rng.integers(1, 3))
        for k in range(n_planes):
            if k == 0:
                lm = 0
            elif rng.random() < 0.25:
                lm = 1000 + 10 * f + k                                   # seen once
            else:
                lm = 1 + (f // int(rng.integers(2, 9))) * 4 + k
            cnt = 0 if rng.random() < 0.15 else int(rng.integers(1, 500))   # empty chunks count as observations too
            rows.append((f, seq, k, lm, off, cnt)); off += cnt
    t = np.array(rows, dtype=P.CHUNK_DTYPE)
    ids = np.unique(t["plane_id"])
    for _ in range(redirects):                                           # what pps_map_redirect does to a table
        a, b = rng.choice(ids[1:], 2, replace=False)
        t["plane_id"][t["plane_id"] == b] = a
    return t, seq


@pytest.mark.parametrize("redirects", [0, 6])
@pytest.mark.parametrize("every_frame", [0, 1])
def test_select_host_restates_the_publishing_loop(built, every_frame, redirects):
    rng = np.random.default_rng(100 + 2 * redirects + every_frame)
    n_drop = 0
    for trial in range(6):
        t, last_seq = random_table(rng, redirects=redirects)
        seqs = np.unique(t["frame_seq_id"])
        # counters that put frames on both sides of every age gate (4, 8, 10, 15), and one before / far behind the sequence
        counters = [int(seqs[len(seqs) // 2]) + a for a in (4, 8, 10, 15)] + [last_seq, last_seq + 3, int(seqs[0]) - 1, last_seq + 100]
        for counter in counters:
            sides = [(t["frame_seq_id"] <= counter - a) for a in (4, 8, 10, 15)]
            if counter in counters[:6]:
                assert all(s.any() and (~s).any() for s in sides), counter
            got = P.map_select_host(t, P.map_select(counter, every_frame=every_frame))
            want = ref_select(t, counter, every_frame)
            np.testing.assert_array_equal(got, want)
            n_drop += int((~want).sum())
    assert n_drop > 0
    assert P.map_select_host(t).all()                                    # sel == NULL keeps all
    assert len(P.map_select_host(t[:0], P.map_select(5))) == 0


def test_default_select_is_the_references(built):
    s = P.map_select(37)
    assert (s.counter, s.every_frame, s.old_age, s.old_every, s.new_every) == (37, 0, 10, 3, 2)
    assert list(zip(s.age, s.min_tracked)) == [(15, 10), (8, 5), (4, 2)]


def test_select_gates_are_parameters(built):
    t, last = random_table(np.random.default_rng(5))
    loose = P.map_select_host(t, P.map_select(last, every_frame=1, min_tracked=(0, 0, 0)))
    assert loose.all()
    third = P.map_select_host(t, P.map_select(last, old_age=-10 ** 6, old_every=4, min_tracked=(0, 0, 0)))
    np.testing.assert_array_equal(third, t["frame"] % 4 == 0)


# ---- argument checks, all on the host ------------------------------------------------------------------------------------------------
def test_every_refusal_is_answered_without_a_device(built):
    L = P.lib()
    g = P.Graph()
    pose = g.add_pose([0, 0, 1, 0, 0, 0, 1]); a = g.add_plane([0, 0, 1, 0]); b = g.add_plane([1, 0, 0, -1])
    h = C.c_void_p()
    assert L.pps_map_create(None, 10, C.byref(h)) == P.PPS_EINVAL
    assert L.pps_map_create(g.h, 10, None) == P.PPS_EINVAL
    assert L.pps_map_create(g.h, -1, C.byref(h)) == P.PPS_EINVAL
    assert L.pps_map_destroy(None) == P.PPS_EINVAL
    assert L.pps_map_last_error(None) == b"null handle"
    ids = (C.c_int * 2)(a, b); n = C.c_int(); tot = P.PpsMapTotals(); sec = (C.c_double * 2)()
    assert L.pps_map_add_frame(None, None, 0, 2, ids, None) == P.PPS_EINVAL
    assert L.pps_map_redirect(None, a, b) == P.PPS_EINVAL
    assert L.pps_map_info(None, C.byref(tot)) == P.PPS_EINVAL
    assert L.pps_map_chunks(None, 0, None, C.byref(n)) == P.PPS_EINVAL
    assert L.pps_map_built_chunks(None, 0, None, C.byref(n)) == P.PPS_EINVAL
    assert L.pps_map_build(None, None, None, None) == P.PPS_EINVAL
    assert L.pps_map_download(None, 0, 0, 0, None) == P.PPS_EINVAL
    assert L.pps_map_last_times(None, sec) == P.PPS_EINVAL
    keep = (C.c_int32 * 4)()
    assert L.pps_map_select_host(None, 4, None, keep, None) == P.PPS_EINVAL
    assert L.pps_map_select_host(None, -1, None, keep, None) == P.PPS_EINVAL
    assert L.pps_map_select_host(None, 0, None, None, C.byref(n)) == P.PPS_OK and n.value == 0

    m = P.Map(g, 1000)
    assert m.info() == dict(capacity=1000, n_points=0, built_points=0, n_frames=0, n_chunks=0, built_chunks=0)

    def refused(fn, code=P.PPS_EINVAL):
        with pytest.raises(P.PpsError) as e:
            fn()
        assert e.value.code == code, e.value
        assert m.info()["n_chunks"] == 0                                  # the map stays usable and unchanged

    refused(lambda: m.add_frame(None, 0, [a, b]))                        # no pop-up context
    refused(lambda: m.redirect(pose, a))                                 # a pose is not a plane
    refused(lambda: m.redirect(a, pose))
    refused(lambda: m.redirect(a, 99))                                   # unknown ids
    refused(lambda: m.redirect(99, a))
    refused(lambda: m.redirect(-1, a))
    refused(lambda: m.download(0, 0, 1))                                 # nothing stored
    refused(lambda: m.download(1, 0, 1))
    refused(lambda: m.download(2, 0, 0))
    refused(lambda: m.download(0, -1, 0))
    refused(lambda: m.build(P.map_select(3, old_every=0)))
    refused(lambda: m.build(P.map_select(3, new_every=-2)))
    # the ids are checked before the pop-up context is looked at: a non-null handle that is never dereferenced reaches the check
    fake = type("FakePopup", (), {"h": C.cast(C.create_string_buffer(4096), C.c_void_p)})()
    refused(lambda: m.add_frame(fake, 0, [a, pose]))                     # a pose among the plane ids
    refused(lambda: m.add_frame(fake, 0, [a, 99]))                       # an unknown id
    refused(lambda: m.add_frame(fake, 0, [a, -2]))                       # only -1 skips
    refused(lambda: m.add_frame(fake, 0, [a] * 66))                      # more planes than a frame can hold
    m.redirect(b, a)                                                     # a known pair: accepted, nothing to move yet
    g.remove_node(b)
    m.redirect(b, a)                                                     # the node that was merged away may still be named as the source
    refused(lambda: m.redirect(a, b))                                    # ... not as the target
    assert m.build() == (0, 0)                                           # an empty map builds to nothing, without a device
    assert len(m.download(1)) == 0 and len(m.chunks()) == 0 and len(m.built_chunks()) == 0
    assert m.last_times() == (0.0, 0.0)
    m.close(); g.close()


def test_hook_refusals_are_answered_without_a_device(built):
    """pps_debug_map_add_points checks everything pps_map_add_frame checks, and its own arrays, before it touches a device"""
    L = P.lib()
    g = P.Graph()
    pose = g.add_pose([0, 0, 1, 0, 0, 0, 1]); a = g.add_plane([0, 0, 1, 0]); b = g.add_plane([1, 0, 0, -1])
    m = P.Map(g, 1000)
    cloud = np.zeros(8, dtype=P.POINT_DTYPE); cloud["rgba"] = 1 << 24
    pid = np.zeros(8, dtype=np.int32)
    ids = (C.c_int * 2)(a, b)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    assert L.pps_debug_map_add_points(None, vp(cloud), vp(pid), 8, 0, 2, ids, None) == P.PPS_EINVAL
    for args in [(None, vp(pid), 8, 0, 2, ids, None), (vp(cloud), None, 8, 0, 2, ids, None), (vp(cloud), vp(pid), 8, 0, 2, None, None),
                 (vp(cloud), vp(pid), 0, 0, 2, ids, None), (vp(cloud), vp(pid), -8, 0, 2, ids, None),
                 (vp(cloud), vp(pid), 1 << 31, 0, 2, ids, None), (vp(cloud), vp(pid), (1 << 32) + 8, 0, 2, ids, None),
                 (vp(cloud), vp(pid), (1 << 30) + 1, 0, 2, ids, None), (vp(cloud), vp(pid), 8, 0, -1, ids, None)]:
        assert L.pps_debug_map_add_points(m.h, *args) == P.PPS_EINVAL, args
        assert L.pps_map_last_error(m.h) != b""

    def refused(fn):
        with pytest.raises(P.PpsError) as e:
            fn()
        assert e.value.code == P.PPS_EINVAL, e.value

    refused(lambda: m.debug_add_points(cloud, pid, 0, [a, pose]))        # a pose among the plane ids
    refused(lambda: m.debug_add_points(cloud, pid, 0, [a, 99]))          # an unknown id
    refused(lambda: m.debug_add_points(cloud, pid, 0, [a, -2]))          # only -1 skips
    refused(lambda: m.debug_add_points(cloud, pid, 0, [a] * 66))         # more planes than a frame can hold
    g.remove_node(b)
    refused(lambda: m.debug_add_points(cloud, pid, 0, [a, b]))           # a node that left the graph
    assert m.info() == dict(capacity=1000, n_points=0, built_points=0, n_frames=0, n_chunks=0, built_chunks=0)
    assert len(m.debug_add_points(cloud, pid, 5, [])) == 0               # a frame without planes: no pixel is read, no device needed
    assert m.info()["n_frames"] == 1 and m.info()["n_chunks"] == 0
    m.close(); g.close()


# ---- the kernels, compiled for the host ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu(built, tmp_path_factory):
    so = tmp_path_factory.mktemp("mapemu") / "libmapemu.so"
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-fPIC", "-shared", "-pthread", "-ffp-contract=off",
                           "-I", os.path.join(ROOT, "tests", "cpp", "map_emu"), "-I", os.path.join(ROOT, "pop_up_slam_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "map_emu.cpp"), "-o", str(so)])
    return C.CDLL(str(so))


N_PLANES_MAX = 65


def emu_partition(E, cloud, pid, nplanes, take):
    """the three kernels the way pps_map_add_frame drives them; -> (counts per plane, base per plane, store)"""
    npx = cloud.size
    nT = E.emu_map_tiles(npx)
    table = np.full(N_PLANES_MAX * nT, -12345, dtype=np.int32); totals = np.full(N_PLANES_MAX, -1, dtype=np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert E.emu_map_count(vp(cloud), vp(pid), npx, nplanes, vp(table), vp(totals)) == 0
    base = np.full(N_PLANES_MAX, -1, dtype=np.int64); used = 0
    for k in range(nplanes):
        if take[k]:
            base[k] = used; used += int(totals[k])
    guard = 7
    store = np.zeros(used + guard, dtype=P.POINT_DTYPE); store["rgba"] = 0xDEADBEEF
    assert E.emu_map_scatter(vp(cloud), vp(pid), npx, nplanes, vp(table), vp(base), vp(store)) == 0
    assert np.all(store["rgba"][used:] == 0xDEADBEEF)                    # nothing behind the frame's points
    return totals[:nplanes].copy(), base, store[:used]


def random_grid(rng, w, h, nplanes, p_valid=0.7, empty_planes=()):
    cloud = np.zeros(w * h, dtype=P.POINT_DTYPE)
    for name in "xyz":
        cloud[name] = rng.normal(size=w * h).astype(np.float32)
    # runs of equal plane ids along a row, like polygons give them, with -1 gaps and ids past nplanes (another frame's leftovers)
    pid = np.repeat(rng.integers(-1, nplanes + 2, size=w * h), rng.integers(1, 14, size=w * h))[:w * h].astype(np.int32)
    assert pid.size == w * h
    for k in empty_planes:
        pid[pid == k] = -1
    valid = rng.random(w * h) < p_valid
    cloud["rgba"] = (valid.astype(np.uint32) << 24) | rng.integers(0, 1 << 24, size=w * h, dtype=np.uint32)
    cloud["rgba"] |= rng.integers(0, 2, size=w * h, dtype=np.uint32) << 25     # bits above the valid bit do not make a point valid
    return cloud, pid, valid


@pytest.mark.parametrize("w,h,nplanes,p_valid,empty", [
    (150, 113, 5, 0.7, (3,)),        # width no multiple of 64, pixels no multiple of 256, a plane without a point
    (67, 9, 65, 0.9, ()),            # every plane index a pixel can hold
    (64, 4, 3, 0.0, ()),             # one workgroup, no valid point at all
    (333, 31, 1, 0.5, ()),           # ground only
])
def test_emulated_partition_is_stable_and_complete(emu, w, h, nplanes, p_valid, empty):
    rng = np.random.default_rng(w * h + nplanes)
    cloud, pid, valid = random_grid(rng, w, h, nplanes, p_valid, empty)
    take = np.ones(nplanes, dtype=bool)
    if nplanes > 2:
        take[1] = False                                                  # plane_node_ids[1] = -1
    counts, base, store = emu_partition(emu, cloud, pid, nplanes, take)
    raw = lambda a: a.view(np.uint8).reshape(-1, 16)
    for k in range(nplanes):
        want = cloud[valid & (pid == k)]                                 # boolean indexing keeps raster order
        assert counts[k] == len(want)
        if k in empty or p_valid == 0.0:
            assert len(want) == 0
        if take[k]:
            np.testing.assert_array_equal(raw(store[base[k]:base[k] + counts[k]]), raw(want))
    assert len(store) == int(counts[take].sum())


def emu_build_check(emu, rng, counts, sel, n_slots=6, ld=11):
    """the build of the chunks `sel` (indices into a store of chunks with `counts` points) against the numpy fp64 projection; slots are
    drawn from -1 .. n_slots-1; returns the chunks that passed through untouched"""
    n_chunks = len(counts)
    src_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    store = np.zeros(int(src_off[-1]), dtype=P.POINT_DTYPE)
    for name in "xyz":
        store[name] = (rng.normal(size=len(store)) * 5).astype(np.float32)
    store["rgba"] = rng.integers(0, 1 << 32, size=len(store), dtype=np.uint32)
    planes = rng.normal(size=(n_slots, 4)); planes /= np.linalg.norm(planes, axis=1, keepdims=True)      # unit 4-vectors, like the state
    est = np.full((4, ld), np.nan); est[:, :n_slots] = planes.T
    assert np.all(counts[sel] > 0) and np.all(np.diff(sel) > 0) and sel[-1] < n_chunks
    slot = rng.integers(-1, n_slots, size=len(sel)).astype(np.int32)
    out_off = np.concatenate([[0], np.cumsum(counts[sel])]).astype(np.int64)
    built = np.zeros(int(out_off[-1]) + 3, dtype=P.POINT_DTYPE); built["rgba"] = 0xDEADBEEF
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    sel_src = np.ascontiguousarray(src_off[sel])
    assert emu.emu_map_build(C.c_longlong(int(out_off[-1])), len(sel), vp(out_off), vp(sel_src), vp(slot), vp(est), ld, vp(store), vp(built)) == 0
    assert np.all(built["rgba"][-3:] == 0xDEADBEEF)
    n_through = 0
    for j, c in enumerate(sel):
        src = store[src_off[c]:src_off[c + 1]]; got = built[out_off[j]:out_off[j + 1]]
        np.testing.assert_array_equal(got["rgba"], src["rgba"])
        xyz = np.stack([src["x"], src["y"], src["z"]], axis=1)
        gxyz = np.stack([got["x"], got["y"], got["z"]], axis=1)
        if slot[j] < 0:
            np.testing.assert_array_equal(gxyz, xyz); n_through += 1
            continue
        want = project_to_plane(planes[slot[j]], xyz)
        assert_within_one_ulp(gxyz, want)
    return n_through


def test_emulated_build_projects_the_selected_chunks(emu):
    rng = np.random.default_rng(9)
    n_chunks = 700                                                       # more chunks than one workgroup's window of 256
    counts = rng.integers(1, 5, size=n_chunks); counts[rng.integers(0, n_chunks, 20)] = rng.integers(200, 900, 20)
    sel = np.sort(rng.choice(n_chunks, 500, replace=False))
    assert emu_build_check(emu, rng, counts, sel) > 10


# ---- what the random grids above do not reach ----------------------------------------------------------------------------------------
BOUNDARIES = (65536, 65537, 307200, 2097152, 2097153)


def test_tiling_arithmetic(emu):
    """map_tiling (csrc/pps_map.h) over every small frame, the boundaries the device tests run at and random sizes up to 2^30: the tiles
    are whole batches of 64, they cover the frame with no tile to spare, the count table stays within 8192 columns, and a wave keeps 256
    pixels whenever that fits"""
    rng = np.random.default_rng(77)
    sizes = list(range(1, 301)) + list(BOUNDARIES) + [8192 * 320, 8192 * 320 + 1, 1 << 30] + [int(v) for v in rng.integers(1, 1 << 30, size=4000)]
    grown = 0
    for npx in sizes:
        wt, nT = emu.emu_map_wt(npx), emu.emu_map_tiles(npx)
        assert wt > 0 and wt % 64 == 0, npx
        assert (nT - 1) * wt < npx <= nT * wt, npx
        assert nT <= 8192, npx
        if npx <= 8192 * 256:
            assert wt == 256, npx
        else:
            grown += 1
        assert (wt, nT) == tiling(npx)[:2], npx                          # the restatement the device tests assert their regime with
    assert grown > 1000
    assert [tiling(n) for n in BOUNDARIES] == [(256, 256, 1), (256, 257, 2), (256, 1200, 5), (256, 8192, 32), (320, 6554, 26)]


def check_emulated_partition(emu, cloud, pid, nplanes, take):
    """the emulated store against the numpy split of the same flat frame"""
    counts, base, store = emu_partition(emu, cloud, pid, nplanes, take)
    want = split_flat(cloud, pid, nplanes)
    for k in range(nplanes):
        assert counts[k] == len(want[k])
        if take[k]:
            np.testing.assert_array_equal(raw16(store[base[k]:base[k] + counts[k]]), raw16(want[k]))
    assert len(store) == int(counts[take].sum())
    return counts


def test_emulated_scan_with_two_tiles_per_thread(emu):
    """257 x 256: nT = 257, so the scan gives its threads seg = 2 tiles, thread 128 one tile and the threads above it none"""
    w, h, nplanes = 257, 256, 7
    assert tiling(w * h) == (256, 257, 2) and emu.emu_map_tiles(w * h) == 257
    cloud, pid, valid = random_grid(np.random.default_rng(257), w, h, nplanes)
    take = np.ones(nplanes, dtype=bool); take[1] = False
    counts = check_emulated_partition(emu, cloud, pid, nplanes, take)
    last_tile = kept_key(cloud, pid, nplanes)[256 * 256:]
    assert np.all(counts > 0) and len(np.unique(last_tile[last_tile >= 0])) > 1     # the tile of thread 128 holds points of several planes


def test_emulated_wave_patterns(emu):
    """a batch of 64 distinct planes (64 turns of the loop), then a batch whose only kept pixel sits in lane 63: the leader is lane 63,
    found in a mask whose only bit is bit 63, and its plane is the 65th"""
    cloud, pid = wave_pattern_frame(np.random.default_rng(63))
    take = np.ones(65, dtype=bool)
    counts = check_emulated_partition(emu, cloud, pid, 65, take)
    assert counts[64] >= 1


def test_emulated_build_windows(emu):
    """tiny chunks: a workgroup that starts on a chunk's first point and whose 256 points lie in 256 chunks, one that starts inside a chunk
    and crosses more than 200, chunks dropped from the middle of both windows"""
    rng = np.random.default_rng(256)
    counts = np.array([512] + [1] * 300 + [220] + [1] * 300, dtype=np.int64)
    every = np.arange(len(counts))
    win = workgroup_windows(counts)
    assert (False, 256) in win and any(mid and n >= 200 for mid, n in win)
    emu_build_check(emu, rng, counts, every)
    # the same after a selection: chunk 0 keeps the window's start on a chunk's first point, the dropped ones lie inside the windows
    sel = np.sort(np.concatenate([[0], 1 + rng.choice(len(counts) - 1, 560, replace=False)]))
    win = workgroup_windows(counts[sel])
    assert (False, 256) in win
    assert emu_build_check(emu, rng, counts, sel) > 10
