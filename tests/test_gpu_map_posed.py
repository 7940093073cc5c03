"""GPU: the posed map (pps_map_build_posed, pps_map_build_grid_posed; k_map_motion / k_map_build_posed of csrc/pps_map.hip and the moved
variant of the grid kernels in csrc/pps_grid.hip).

The device is compared with the host entry points pps_map_motion_host / pps_map_move_point_host -- compiled from the header the kernels
include -- as raw records: no tolerance.  Those host functions are held to the numpy restatement in tests/test_host_map_posed.py.  The
frames go in through pps_debug_map_add_points unless stated otherwise."""
import ctypes as C

import numpy as np
import pytest

import pop_up_slam_amd as P
import map_posed_helpers as H
from grid_helpers import NEWEST, OLDEST, on_plane, one_point_frame, points, ref_grid, scan_frame
from map_helpers import raw16, runs_frame, wave_pattern_frame, workgroup_windows, xyz_of
from pop_up_slam_amd import synth
from test_gpu_map import _popup
from test_gpu_map_grid import _live

pytestmark = pytest.mark.gpu

GROUND, WALL, SIDE = [0.0, 0.0, -1.0, 0.2], [0.6, -0.8, 0.0, 0.7], [1.0, 0.0, 0.0, -2.0]
ERR_T, ERR_AXIS, ERR_ANGLE = [0.25, -0.12, 0.11], [0.2, 1.0, -0.3], np.deg2rad(5.0)       # |ERR_T| = 0.3 m


def _graph(planes, poses):
    """pose and plane nodes the builds can read the estimate of: every node carries a prior, nothing is optimised unless a test does"""
    g = P.Graph()
    ps, pl = [], []
    for tq in poses:
        ps.append(g.add_pose(list(tq)))
        g.add_pose_prior(ps[-1], synth.pose_vector(np.asarray(tq, dtype=np.float64)), synth._ut_diag([1.0] * 6))
    for abcd in planes:
        pl.append(g.add_plane(list(abcd)))
        g.add_plane_prior(pl[-1], g.get_plane(pl[-1]), synth._ut_diag([300.0] * 3))
    return g, ps, pl


def _poses(rng, n):
    """(estimate, capture pose T0 fp32) per frame: T0 is 0.3 m / 5 degrees (about a random axis) off the estimate"""
    est = [H.random_pose(rng, 2.0) for _ in range(n)]
    return est, [H.T_of(H.compose(tq, ERR_T, rng.normal(size=3), ERR_ANGLE)).astype(np.float32) for tq in est]


def _move_all(D, abcd, xyz32):
    """pps_map_move_point_host over (n, 3) fp32 points"""
    L = P.lib()
    xyz = np.ascontiguousarray(xyz32, dtype=np.float32).reshape(-1, 3); out = np.zeros_like(xyz)
    d = np.ascontiguousarray(D, dtype=np.float64) if D is not None else None
    pl = np.ascontiguousarray(abcd, dtype=np.float64) if abcd is not None else None
    dp = d.ctypes.data_as(C.POINTER(C.c_double)) if d is not None else None
    pp = pl.ctypes.data_as(C.POINTER(C.c_double)) if pl is not None else None
    fp = C.POINTER(C.c_float)
    a, b = xyz.ctypes.data, out.ctypes.data
    for i in range(len(xyz)):
        assert L.pps_map_move_point_host(dp, pp, C.cast(a + 12 * i, fp), C.cast(b + 12 * i, fp)) == P.PPS_OK
    return out


def _node(get, nid):
    try:
        return get(int(nid))
    except P.PpsError:
        return None


def _expected(g, m, sel=None, sample=None):
    """what the statement says of the state, from the host functions: (posed map as records, motion table, moved flags, unposed frames).
    sample: indices of the built map to evaluate (None: all); the other records are left zero."""
    chunks, frames, store = m.chunks(), m.frames(), m.download(0)
    keep = P.map_select_host(chunks, sel)
    rows, Ds, moved = {}, [], []
    n_out = int(chunks["count"][keep].sum())
    want = np.zeros(n_out, dtype=P.POINT_DTYPE)
    take = np.ones(n_out, dtype=bool) if sample is None else np.isin(np.arange(n_out), sample)
    o = 0
    for c in chunks[keep]:
        cnt = int(c["count"])
        if cnt == 0:
            continue
        f = int(c["frame"])
        if f not in rows:
            rows[f] = len(Ds)
            tq = _node(g.get_pose, frames[f]["pose_id"]) if frames[f]["pose_id"] >= 0 else None
            moved.append(0 if tq is None else 1)
            Ds.append(np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]) if tq is None else P.map_motion_host(frames[f]["T_wc"], tq))
        r = rows[f]
        idx = np.flatnonzero(take[o:o + cnt])
        if len(idx):
            raw = store[int(c["offset"]) + idx]
            xyz = _move_all(Ds[r] if moved[r] else None, _node(g.get_plane, c["plane_id"]), xyz_of(raw))
            seg = np.zeros(len(idx), dtype=P.POINT_DTYPE)
            seg["x"], seg["y"], seg["z"], seg["rgba"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], raw["rgba"]
            want[o + idx] = seg
        o += cnt
    return want, np.array(Ds).reshape(-1, 12), np.array(moved, dtype=np.int32), int(len(moved) - sum(moved))


def _check(g, m, sel=None, sample=None):
    """build(posed=True) against the host functions; returns the downloaded posed map"""
    want, Ds, moved, unposed = _expected(g, m, sel, sample)
    n_pts, n_chunks = m.build(sel, posed=True)
    keep = P.map_select_host(m.chunks(), sel)
    assert (n_pts, n_chunks) == (len(want), int(keep.sum())) and m.info()["built_points"] == len(want)
    got = m.download(1)
    D, mv = m.frame_motions()
    np.testing.assert_array_equal(mv, moved)
    np.testing.assert_array_equal(D.view(np.uint64), Ds.view(np.uint64))
    last = m.posed_last()
    assert last["n_unposed_frames"] == unposed
    if len(want):
        assert last["launches"] == 2 and last["sec"][0] > 0.0 and last["sec"][1] > 0.0
    if sample is None:
        np.testing.assert_array_equal(raw16(got), raw16(want))
    else:
        np.testing.assert_array_equal(raw16(got[sample]), raw16(want[sample]))
    bt = m.built_chunks()
    np.testing.assert_array_equal(bt["count"], m.chunks()["count"][keep])
    np.testing.assert_array_equal(bt["offset"], np.concatenate([[0], np.cumsum(bt["count"])[:-1]]) if len(bt) else bt["offset"])
    return got


# ---- device = host functions ---------------------------------------------------------------------------------------------------------
def test_device_equals_host_functions(built):
    rng = np.random.default_rng(11)
    est, T0 = _poses(rng, 3)
    g, ps, pl = _graph([GROUND, WALL, SIDE], est)
    m = P.Map(g, 3 * 150)
    for f in range(3):
        cloud, pid = scan_frame(rng, [GROUND, WALL, SIDE], 15, 10, (-0.3 + 0.1 * f, -0.2), 0.05)
        m.debug_add_points(cloud, pid, f, pl)
        m.set_frame_pose(f, ps[f], T0[f])
    assert 300 < m.info()["n_points"] <= 450
    for f in range(3):                                                   # the estimate from pps_set_pose
        g.set_pose(ps[f], H.compose(est[f], [0.02 * f, 0.01, -0.03], [0, 0, 1], 0.02))
    got = _check(g, m)
    plain_n = m.build()
    plain = m.download(1)
    assert plain_n[0] == len(got) and np.max(np.abs(xyz_of(got) - xyz_of(plain))) > 0.1               # 0.3 m / 5 degrees were taken back
    was = [g.get_pose(p) for p in ps]
    g.update()                                                           # the estimate the device computed itself (a step towards the priors)
    assert min(np.max(np.abs(g.get_pose(p) - a)) for p, a in zip(ps, was)) > 1e-4
    _check(g, m)
    m.close(); g.close()


# ---- no records ----------------------------------------------------------------------------------------------------------------------
def test_without_records_the_posed_calls_are_the_plain_ones(built):
    rng = np.random.default_rng(12)
    g, ps, pl = _graph([GROUND, WALL], [H.random_pose(rng)])
    m = P.Map(g, 3 * 1200)
    for f in range(3):
        cloud, pid = scan_frame(rng, [GROUND, WALL], 40, 30, (-0.5 + 0.2 * f, -0.4), 0.03)
        m.debug_add_points(cloud, pid, f, pl)
    m.build()
    plain = (m.download(1).tobytes(), m.built_chunks().tobytes())
    m.build_grid(cell=0.05)
    plain_grid = tuple(a.tobytes() for a in m.grid_download()) + (m.grid_planes().tobytes(),)
    assert m.build(posed=True)[0] == m.info()["n_points"] > 2000
    assert (m.download(1).tobytes(), m.built_chunks().tobytes()) == plain
    assert m.frame_motions()[1].tolist() == [0, 0, 0] and m.posed_last()["n_unposed_frames"] == 3
    m.build_grid(cell=0.05, posed=True)
    assert tuple(a.tobytes() for a in m.grid_download()) + (m.grid_planes().tobytes(),) == plain_grid
    m.close(); g.close()


# ---- workgroup and window edges ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_b", [255, 256, 257, 511, 513])
def test_sizes_at_the_workgroup_edge(built, n_b):
    rng = np.random.default_rng(n_b)
    est, T0 = _poses(rng, 2)
    g, ps, pl = _graph([GROUND, WALL], est)
    m = P.Map(g, 1024)
    first = n_b // 3
    m.debug_add_points(points(on_plane(np.array(GROUND), rng.uniform(-1, 1, size=(first, 2))), rng), np.zeros(first, np.int32), 0, [pl[0]])
    m.debug_add_points(points(on_plane(np.array(WALL), rng.uniform(-1, 1, size=(n_b - first, 2))), rng), np.zeros(n_b - first, np.int32), 1, [pl[1]])
    m.set_frame_pose(0, ps[0], T0[0]); m.set_frame_pose(1, ps[1], T0[1])
    assert len(_check(g, m)) == n_b
    m.close(); g.close()


def test_one_point_chunks_of_twelve_frames(built):
    """720 one-point chunks, 60 per frame, every frame with a motion of its own: a workgroup's 256 points lie in 256 chunks of five or six
    frames (more chunks under a workgroup than one LDS window holds), a wave's 64 points in two frames"""
    rng = np.random.default_rng(13)
    est, T0 = _poses(rng, 12)
    planes = [GROUND, WALL, SIDE, [0, 2, 0, 1], [0.1, 0.2, -0.9, 0.5], [0.3, 0.5, 0.81, 1.0], [-0.6, 0.1, 0.3, 0.4]]
    g, ps, pl = _graph(planes, est)
    m = P.Map(g, 1024)
    for f in range(12):
        cloud, pid = one_point_frame(rng, 60)
        m.debug_add_points(cloud, pid, f, [pl[int(v)] for v in rng.integers(0, 7, size=60)])
        m.set_frame_pose(f, ps[f], T0[f])
    t = m.chunks()
    assert len(t) == 720 and np.all(t["count"] == 1)
    w = workgroup_windows(t["count"])
    assert len(w) == 3 and w[0][1] == 256
    _check(g, m)
    m.close(); g.close()


def test_65_planes_and_an_empty_chunk(built):
    rng = np.random.default_rng(14)
    est, T0 = _poses(rng, 3)
    g, ps, pl = _graph([[np.sin(i), np.cos(i), 0.1 * i, -1.0 - 0.1 * i] for i in range(65)], est)
    m = P.Map(g, 165 + 4097 + 600)
    cloud, pid = wave_pattern_frame(rng); m.debug_add_points(cloud, pid, 0, pl)
    cloud, pid = runs_frame(rng, 4097, 65); m.debug_add_points(cloud, pid, 1, pl)
    cloud, pid = runs_frame(rng, 600, 3); pid[pid == 1] = -1             # frame 2: plane 1 is observed and has no point
    m.debug_add_points(cloud, pid, 2, pl[:3])
    for f in range(3):
        m.set_frame_pose(f, ps[f], T0[f])
    t = m.chunks()
    assert len(t) == 133 and t["count"][131] == 0 and t["count"][130] > 0 and t["count"][132] > 0
    got = _check(g, m)
    assert len(got) > 2000 and len(m.built_chunks()) == 133
    m.close(); g.close()


# ---- mixed states in one build -------------------------------------------------------------------------------------------------------
def test_mixed_states_in_one_build(built):
    rng = np.random.default_rng(15)
    est, T0 = _poses(rng, 4)
    near = np.array(WALL) + [0.02, 0.01, 0.0, 0.01]
    g, ps, pl = _graph([GROUND, WALL, near, SIDE], est)
    m = P.Map(g, 4 * 1200)
    for f in range(4):
        cloud, pid = scan_frame(rng, [GROUND, WALL, WALL, SIDE], 40, 30, (-0.5, -0.4 + 0.1 * f), 0.03)
        m.debug_add_points(cloud, pid, f, pl)
    m.set_frame_pose(0, ps[0], T0[0])                                    # frame 0: posed; frame 1: no record
    m.set_frame_pose(2, ps[2], T0[2]); m.set_frame_pose(3, ps[3], T0[3])
    g.remove_node(ps[2])                                                 # frame 2: its pose node is gone -> unmoved and counted
    m.redirect(pl[2], pl[1]); g.remove_node(pl[2])                       # a redirected landmark
    g.remove_node(pl[3])                                                 # a landmark that is gone: moved, not projected
    got = _check(g, m)
    assert m.frame_motions()[1].tolist() == [1, 0, 0, 1] and m.posed_last()["n_unposed_frames"] == 2
    store, t = m.download(0), m.chunks()
    gone0 = t[(t["frame"] == 0) & (t["plane_id"] == pl[3])][0]; gone1 = t[(t["frame"] == 1) & (t["plane_id"] == pl[3])][0]
    bt = m.built_chunks()
    b0 = bt[(bt["frame"] == 0) & (bt["plane_id"] == pl[3])][0]; b1 = bt[(bt["frame"] == 1) & (bt["plane_id"] == pl[3])][0]
    seg = lambda a, c: a[int(c["offset"]):int(c["offset"] + c["count"])]
    assert gone0["count"] > 50
    np.testing.assert_array_equal(raw16(seg(got, b1)), raw16(seg(store, gone1)))                     # unmoved and unprojected: the stored bytes
    assert np.min(np.linalg.norm(xyz_of(seg(got, b0)).astype(np.float64) - xyz_of(seg(store, gone0)), axis=1)) > 0.05
    # a selection that drops frames: the motion table follows it
    sel = P.map_select(3, every_frame=0, old_age=-100, old_every=3, min_tracked=(0, 0, 0))           # frames 0 and 3
    keep = P.map_select_host(m.chunks(), sel)
    assert sorted(set(m.chunks()["frame"][keep].tolist())) == [0, 3]
    _check(g, m, sel)
    assert m.frame_motions()[1].tolist() == [1, 1] and m.posed_last()["n_unposed_frames"] == 0
    m.close(); g.close()


# ---- returns to truth ----------------------------------------------------------------------------------------------------------------
def test_two_frames_of_one_wall_patch_coincide(built):
    """Two frames see the same 4000 wall points w from true poses a and b; each is captured 0.3 m / 5 degrees off (T0 = T* o E, another E
    each) and stores fl32(T0 s), s = T*^-1 w.  With the true poses as the estimate the posed build brings both frames' points back to w;
    the plain build leaves matching points of the two frames more than 0.1 m apart.

    Bound per frame, around w: the one-ulp check of the host test with its absolute term 64 eps64 (1 + |p| + |t_D|), plus what the INPUTS
    carry, from the number formats alone: every stored coordinate was rounded to fp32 once (half an ulp of a coordinate below 32 m, three
    coordinates: sqrt(3) 2^-20 m, carried rigidly), and T0 is rigid to fp32 only, which moves a point by at most |R0^T R0 - I|_2 |p - t0|."""
    rng = np.random.default_rng(16)
    wall = np.array([0.6, -0.8, 0.0, 0.0]); n = wall[:3]
    centre = np.array([14.0, -12.0, 10.0]); wall[3] = -(n @ centre)
    e1, e2 = np.array([0.8, 0.6, 0.0]), np.array([0.0, 0.0, 1.0])
    uv = rng.uniform(-1.0, 1.0, size=(4000, 2))
    w = centre + uv[:, :1] * e1 + uv[:, 1:] * e2
    true = [np.concatenate([centre - 2.0 * n + 0.4 * e1, H.quat_from_axis_angle([0.1, 0.2, 1.0], 0.7)]),
            np.concatenate([centre - 2.2 * n - 0.5 * e1 + 0.2 * e2, H.quat_from_axis_angle([0.3, -0.2, 1.0], 1.1)])]
    errs = [(ERR_T, ERR_AXIS), ([-0.2, 0.2, 0.1], [1.0, 0.1, 0.4])]
    g, ps, pl = _graph([wall], true)
    m = P.Map(g, 8000)
    carried = []
    for f in range(2):
        Tt = H.T_of(true[f])
        s = (w - Tt[:3, 3]) @ Tt[:3, :3]
        T0 = H.T_of(H.compose(true[f], errs[f][0], errs[f][1], ERR_ANGLE)).astype(np.float32)
        R0, t0 = T0[:3, :3].astype(np.float64), T0[:3, 3].astype(np.float64)
        p = s @ R0.T + t0
        assert np.max(np.abs(p)) < 32.0
        m.debug_add_points(points(p), np.zeros(len(p), np.int32), f, pl)
        m.set_frame_pose(f, ps[f], T0)
        carried.append(np.sqrt(3.0) * 2.0 ** -20 + np.linalg.norm(R0.T @ R0 - np.eye(3), 2) * np.linalg.norm(p - t0, axis=1))
    assert m.info()["n_points"] == 8000
    got = _check(g, m)
    stored = m.download(0)
    for f in range(2):
        D = m.frame_motions()[0][f]
        H.assert_points_within(xyz_of(got[4000 * f:4000 * (f + 1)]), w, H.point_abs_bound(D, xyz_of(stored[4000 * f:4000 * (f + 1)])) + carried[f])
    a, b = xyz_of(got[:4000]).astype(np.float64), xyz_of(got[4000:]).astype(np.float64)
    # matching points of the two frames: each lies within its carried term and one and a half fp32 ulps (of a coordinate below 32 m) of w
    assert np.max(np.linalg.norm(a - b, axis=1)) <= np.sqrt(3.0) * sum(float(np.max(c)) + 1.5 * 2.0 ** -19 for c in carried)
    m.build()
    plain = xyz_of(m.download(1)).astype(np.float64)
    assert np.min(np.linalg.norm(plain[:4000] - plain[4000:], axis=1)) >= 0.1
    m.close(); g.close()


# ---- posed grid ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def overlapping(built):
    rng = np.random.default_rng(17)
    est, T0 = _poses(rng, 3)
    g, ps, pl = _graph([GROUND, WALL], est)
    m = P.Map(g, 3 * 5000)
    for f in range(3):
        cloud, pid = scan_frame(rng, [GROUND, WALL], 100, 50, (-2.0 + 0.5 * f, -1.0 + 0.2 * f), 0.027)
        m.debug_add_points(cloud, pid, f, pl)
        if f != 1:
            m.set_frame_pose(f, ps[f], T0[f])                            # frame 1 has no record
    yield g, m, pl
    m.close(); g.close()


def _grid_bytes(m):
    return tuple(a.tobytes() for a in m.grid_download()) + (m.grid_planes().tobytes(),)


@pytest.mark.parametrize("rule", [NEWEST, OLDEST], ids=["newest", "oldest"])
@pytest.mark.parametrize("cell", [0.05, 0.5])
def test_posed_grid(overlapping, cell, rule):
    g, m, pl = overlapping
    m.build_grid(cell=cell, rule=rule)
    plain = _grid_bytes(m)
    ret = m.build_grid(cell=cell, rule=rule, posed=True)
    pts, counts, ij, src = m.grid_download()
    info, planes = m.grid_info(), m.grid_planes()
    first = _grid_bytes(m)
    assert m.frame_motions()[1].tolist() == [1, 0, 1] and m.posed_last()["launches"] == 1
    B = _check(g, m)                                                     # the posed map, held to the host functions
    want = ref_grid(B, m.built_chunks(), _live(g, m), planes, info["inv_cell"], rule, 1)
    assert {k: info[k] for k in want["totals"]} == want["totals"] and ret == (want["totals"]["n_cells"], want["totals"]["n_planes"])
    for k in want["planes"].dtype.names:
        np.testing.assert_array_equal(planes[k], want["planes"][k], err_msg=k)
    np.testing.assert_array_equal(src, want["src"]); np.testing.assert_array_equal(counts, want["counts"]); np.testing.assert_array_equal(ij, want["ij"])
    np.testing.assert_array_equal(raw16(pts), raw16(want["pts"]))
    np.testing.assert_array_equal(raw16(pts), raw16(B[src]))             # src indexes the posed map
    assert first != plain and want["totals"]["n_cells"] > 10
    m.build_grid(cell=cell, rule=rule, posed=True)
    assert _grid_bytes(m) == first                                       # two posed calls on the same state: the same bytes
    assert m.download(1).tobytes() == B.tobytes()                        # the posed grid left the built map alone
    m.build_grid(cell=cell, rule=rule)
    assert _grid_bytes(m) == plain                                       # a plain grid afterwards: today's bytes


# ---- state ---------------------------------------------------------------------------------------------------------------------------
def test_a_posed_build_leaves_store_tables_and_graph_alone(built):
    rng = np.random.default_rng(18)
    spec = synth.small_world(6, 4, seed=5)
    g = P.Graph(); spec.replay(g); g.batch_optimize()
    pl = [i for i, t in enumerate(spec.node_type) if t == synth.NODE_PLANE]
    ps = [i for i, t in enumerate(spec.node_type) if t == synth.NODE_POSE]
    m = P.Map(g, 2 * 1200)
    T0 = []
    for f in range(2):
        cloud, pid = scan_frame(rng, [g.get_plane(p) for p in pl[:3]], 40, 30, (-0.5, -0.4 + 0.1 * f), 0.03)
        m.debug_add_points(cloud, pid, f, pl[:3])
        T0.append(H.T_of(H.compose(g.get_pose(ps[f]), ERR_T, ERR_AXIS, ERR_ANGLE)).astype(np.float32))
        m.set_frame_pose(f, ps[f], T0[f])
    g.cov_recover()
    # the store, the chunk and frame tables; the estimate, the LM trace, and the recovery (it answers only while nothing invalidated it)
    state = lambda: (m.info()["n_points"], m.chunks().tobytes(), m.download(0).tobytes(), m.frames().tobytes(),
                     np.asarray(g.get_poses(ps)).tobytes(), np.asarray(g.get_planes(pl)).tobytes(), g.trace(),
                     [b.tobytes() for b in g.cov_marginals([ps[0], pl[0]])])
    before = state()
    _check(g, m)
    m.build_grid(cell=0.05, posed=True)
    assert state() == before
    # set_frame_pose twice overwrites; clearing works
    other = H.T_of(H.compose(g.get_pose(ps[1]), [0.1, 0.0, 0.0], [0, 0, 1], 0.01)).astype(np.float32)
    m.set_frame_pose(0, ps[1], other)
    fr = m.frames()
    assert fr["pose_id"].tolist() == [ps[1], ps[1]] and fr["T_wc"][0].tobytes() == other.tobytes()
    second = _check(g, m)
    m.set_frame_pose(0, -1)
    assert m.frames()["pose_id"].tolist() == [-1, ps[1]]
    third = _check(g, m)
    assert m.frame_motions()[1].tolist() == [0, 1] and second.tobytes() != third.tobytes()
    m.close(); g.close()


# ---- a real frame --------------------------------------------------------------------------------------------------------------------
def test_popup_frame(built):
    """add_frame remembers the T_wc of the run.  The pose: the camera convention's own rotation (quaternion of halves, a matrix of 0 and
    +-1) at a translation of binary fractions, so the fp32 T_wc IS the pose and D is exactly the identity -- posed and plain build then
    agree to the stated bound of one fp32 ulp plus the absolute term (they are equal).  A general pose follows, held to the host functions bit for bit."""
    w, h = 160, 120
    pp, K = _popup(w, h)
    spec = synth.small_world(12, 6, seed=3)
    g = P.Graph(); spec.replay(g); g.batch_optimize()
    pl = [i for i, t in enumerate(spec.node_type) if t == synth.NODE_PLANE]
    m = P.Map(g, 2 * w * h)
    poses = [synth.pose_from_Rt(synth.CAM_R0, np.array([0.125, 0.25, 1.0])),
             synth.pose_from_Rt(synth._Rz(0.05) @ synth.CAM_R0, np.array([0.1, 0.3, 1.0]))]
    nodes = []
    for f, tq in enumerate(poses):
        seg, polys, T = synth.corridor_frame(tq, width=w, height=h, K=K)
        assert pp.run(seg, T, polys, step=2, depth_thre=10.0, ceiling_thre=2.5) > 0
        assert np.all(m.add_frame(pp, f, pl[:4]) > 0)
        nodes.append(g.add_pose(tq)); g.add_pose_prior(nodes[-1], synth.pose_vector(tq), synth._ut_diag([1.0] * 6))
        m.set_frame_pose(f, nodes[-1])                                   # T_wc = NULL: the run's
        assert m.frames()["T_wc"][f].tobytes() == np.ascontiguousarray(T, dtype=np.float32).tobytes()
    D = P.map_motion_host(m.frames()["T_wc"][0], g.get_pose(nodes[0]))
    assert D.tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
    posed = _check(g, m)
    m.build()
    plain = m.download(1)
    n0 = int(m.chunks()["count"][m.chunks()["frame"] == 0].sum())
    H.assert_points_within(xyz_of(posed[:n0]), xyz_of(plain[:n0]).astype(np.float64), H.point_abs_bound(D, xyz_of(m.download(0)[:n0])))
    assert np.max(np.abs(xyz_of(posed[n0:]) - xyz_of(plain[n0:]))) < 1e-5          # frame 1: T_wc is its pose to fp32
    m.close(); g.close()


def test_the_pipeline_registers_every_frame(built):
    """gpu_pipeline(map_points=..): every frame is added to the kept map and carries its pose node and the T_wc its run was given"""
    from pop_up_slam_amd import pipeline
    frames = pipeline.popup_sequence(n_frames=6)
    given = []
    pl, g, pp, stats = pipeline.gpu_pipeline(step=2, map_points=6 * 320 * 240)
    popup_fn = pl.popup_fn
    pl.popup_fn = lambda seg, T32, polys: (given.append(np.array(T32, dtype=np.float32)), popup_fn(seg, T32, polys))[1]
    for fr in frames:
        pl.process(fr)
    m = stats["map"]
    fr = m.frames()
    assert fr["pose_id"].tolist() == pl.pose_nodes and fr["frame_seq_id"].tolist() == list(range(6))
    np.testing.assert_array_equal(fr["T_wc"], np.array(given))
    assert len(m.chunks()) == sum(len(f.ids) + 1 for f in frames) and m.info()["n_points"] > 10000
    posed = _check(g, m)
    m.build()
    d = np.abs(xyz_of(posed).astype(np.float64) - xyz_of(m.download(1)))
    assert np.isfinite(d).all() and 1e-6 < d.max() < 0.5               # the optimiser moved the poses a little, the map followed
    m.close(); g.close()


# ---- size ----------------------------------------------------------------------------------------------------------------------------
def test_300000_points(built):
    """four flat frames of 320 x 240 over six landmarks: the host function on a strided sample of 4096 points plus both ends of every chunk"""
    planes = [GROUND, WALL, SIDE, [0, 2, 0, 1], [0.1, 0.2, -0.9, 0.5], [0.3, 0.5, 0.81, 1.0]]
    rng = np.random.default_rng(19)
    est, T0 = _poses(rng, 4)
    g, ps, pl = _graph(planes, est)
    m = P.Map(g, 4 * 320 * 240)
    for f in range(4):
        cloud, pid = scan_frame(rng, planes, 320, 240, (-3.0 + 0.4 * f, -2.0 + 0.3 * f), 0.011)
        m.debug_add_points(cloud, pid, f, pl)
        m.set_frame_pose(f, ps[f], T0[f])
    n = m.info()["n_points"]
    assert n > 250000
    t = m.chunks()
    ends = np.concatenate([np.cumsum(t["count"]) - t["count"], np.cumsum(t["count"]) - 1])
    sample = np.unique(np.concatenate([np.linspace(0, n - 1, 4096).astype(np.int64), ends[(ends >= 0) & (ends < n)]]))
    assert 4096 <= len(sample) <= 4096 + 2 * len(t)
    _check(g, m, sample=sample)
    m.close(); g.close()
