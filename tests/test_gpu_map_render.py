"""GPU: the rendered view (pps_map_render, csrc/pps_render.hip).  Every pixel of the four images and the hit count are compared EXACTLY
with the numpy statement of render_helpers.ref_render, which reads the plane equations the grid was built with (grid_plane_eq), the boxes
of grid_planes, the library's inv_cell and the grid map grid_download returns -- none of the render code.  The frames go in through
pps_debug_map_add_points.  No tolerance is introduced anywhere."""
import ctypes as C

import numpy as np
import pytest

import pop_up_slam_amd as P
from grid_helpers import NEWEST, OLDEST, on_plane, points
from render_helpers import assert_view_equal, look_at, pinhole_invK, pose, ref_render, rot_xyz
from test_gpu_map_grid import _graph

pytestmark = pytest.mark.gpu

GROUND, WALL, TILTED = [0.0, 0.0, -1.0, 0.2], [0.6, -0.8, 0.0, 0.7], [0.3, 0.5, 0.81, 1.0]


def patch(rng, abcd, u, v, pitch, keep=1.0, lift=0.004):
    """points of a landmark: a raster of plane coordinates [u0, u1] x [v0, v1] at `pitch`, jittered inside the pitch and lifted a few
    millimetres off the plane (the projection takes that away), a fraction `keep` of them kept"""
    uu, vv = np.meshgrid(np.arange(u[0], u[1], pitch), np.arange(v[0], v[1], pitch), indexing="xy")
    uv = np.stack([uu.ravel(), vv.ravel()], axis=1) + rng.uniform(0.0, 0.3 * pitch, size=(uu.size, 2))
    uv = uv[rng.random(len(uv)) < keep]
    return points(on_plane(np.asarray(abcd, dtype=np.float64), uv, rng.normal(size=len(uv)) * lift), rng)


def fill(m, clouds, nodes, first_frame=0):
    """one frame per cloud, all of its points on plane node nodes[k]"""
    for k, (cloud, node) in enumerate(zip(clouds, nodes)):
        m.debug_add_points(cloud, np.zeros(len(cloud), np.int32), first_frame + k, [node])


class Scene:
    """a map with a grid, and the grid's read-back the statement computes from (taken once per grid)"""

    def __init__(self, g, m):
        self.g, self.m = g, m
        self.refresh()

    def refresh(self):
        m = self.m
        self.planes, self.eq, self.info = m.grid_planes(), m.grid_plane_eq(), m.grid_info()
        self.pts, self.counts, self.ij, self.src = m.grid_download()

    def check(self, width, height, invK, T_wc, reach=1, z_near=0.0, z_far=np.inf):
        got = self.m.render(width, height, invK, T_wc, reach, z_near, z_far)
        want = ref_render(width, height, invK, T_wc, self.planes, self.eq, self.info["inv_cell"], self.pts, self.ij, reach, z_near, z_far)
        assert_view_equal(got, want)
        t = got["totals"]
        assert (t["width"], t["height"], t["n_hit"]) == (width, height, want["n_hit"]) and t["launches"] in (1, 2) and t["sec"] > 0.0
        assert t["n_planes"] == int(np.count_nonzero(self.planes["ni"].astype(np.int64) * self.planes["nj"]))
        return want


# ---- a ground, a wall and a tilted plane ---------------------------------------------------------------------------------------------
THREE_EYE, THREE_TARGET = [2.6, -2.4, -1.6], [-0.2, 0.2, 0.1]


def three_planes_clouds(rng):
    return [patch(rng, GROUND, (-2.0, 2.0), (-2.0, 2.0), 0.03, keep=0.8), patch(rng, WALL, (-2.0, 2.0), (-1.5, 0.2), 0.03, keep=0.8),
            patch(rng, TILTED, (-1.0, 1.0), (-1.0, 1.0), 0.03, keep=0.8)]


def three_poses():
    T0 = look_at(THREE_EYE, THREE_TARGET, up=(0.0, 0.0, -1.0))
    R = np.asarray(T0[:3, :3], dtype=np.float64) @ rot_xyz(0.25, -0.2, 0.4)
    return [T0, pose(R, [2.2, -2.0, -1.2])]


@pytest.fixture(scope="module")
def three(built):
    g, pl = _graph([GROUND, WALL, TILTED])
    rng = np.random.default_rng(31)
    clouds = three_planes_clouds(rng)
    m = P.Map(g, sum(len(c) for c in clouds))
    fill(m, clouds, pl)
    m.build_grid(cell=0.05)
    yield Scene(g, m), pl
    m.close(); g.close()


@pytest.mark.parametrize("which", [0, 1], ids=["level", "rotated"])
@pytest.mark.parametrize("size", [(1, 1), (5, 3), (17, 9), (64, 48)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_three_planes(three, size, which):
    s, pl = three
    w, h = size
    want = s.check(w, h, pinhole_invK(w, h, 0.7 * max(w, h)), three_poses()[which])
    if size == (64, 48):
        assert set(np.unique(want["plane_id"]).tolist()) == {-1, pl[0], pl[1], pl[2]}    # the three landmarks and the empty background
    if size == (1, 1):
        assert want["n_hit"] == 1


def test_cell_output_indexes_the_grid_map(three):
    s, pl = three
    w, h = 64, 48
    got = s.m.render(w, h, pinhole_invK(w, h, 45.0), three_poses()[0], reach=2)
    hit = got["plane_id"] >= 0
    assert hit.sum() == got["n_hit"] > 500 and np.all(got["cell"][~hit] == -1)
    c = got["cell"][hit]
    assert c.min() >= 0 and c.max() < s.info["n_cells"]
    np.testing.assert_array_equal(got["cloud"]["rgba"][hit], s.pts["rgba"][c])           # the colour is the grid point's
    # the plane id is that of the landmark whose range of the grid map holds the cell
    row = np.searchsorted(s.planes["offset"], c, side="right") - 1
    np.testing.assert_array_equal(got["plane_id"][hit], s.planes["plane_id"][row])
    # the answering cell lies within `reach` rings of the pixel's own cell: its ij, from the library's axes
    xyz = np.stack([got["cloud"][k][hit].astype(np.float64) for k in "xyz"], axis=1)
    own = np.stack([np.floor(((xyz[:, 0] * s.planes[e][row, 0] + xyz[:, 1] * s.planes[e][row, 1]) + xyz[:, 2] * s.planes[e][row, 2]) * s.info["inv_cell"])
                    for e in ("e1", "e2")], axis=1).astype(np.int64)
    d = np.abs(s.ij[c] - own).max(axis=1)
    assert d.max() <= 2 and np.count_nonzero(d == 0) > 0.5 * len(d) and np.any(d > 0)
    for one in (0, len(c) // 2, len(c) - 1):                             # single cells through pps_map_grid_download
        p, _, ij, _ = s.m.grid_download(int(c[one]), 1)
        assert ij[0].tolist() == s.ij[c[one]].tolist() and p["rgba"][0] == got["cloud"]["rgba"][hit][one]


def test_two_renders_give_the_same_bytes_and_leave_the_grid_alone(three):
    s, pl = three
    w, h = 64, 48
    info = s.m.grid_info(); grid = tuple(a.tobytes() for a in s.m.grid_download()) + (s.m.grid_planes().tobytes(), s.m.grid_plane_eq().tobytes())
    a = s.m.render(w, h, pinhole_invK(w, h, 45.0), three_poses()[1])
    b = s.m.render(w, h, pinhole_invK(w, h, 45.0), three_poses()[1])
    for k in ("cloud", "depth", "plane_id", "cell"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["n_hit"] == b["n_hit"] > 0 and b["totals"]["launches"] == 1                 # the slot table is kept
    again = s.m.render_download()
    assert all(again[k].tobytes() == b[k].tobytes() for k in again)
    only = np.zeros((h, w), dtype=np.float32)                            # any subset of the outputs
    s.m._ck(s.m.L.pps_map_render_download(s.m.h, None, only.ctypes.data_as(C.c_void_p), None, None))
    assert only.tobytes() == b["depth"].tobytes()
    assert s.m.grid_info() == info                                       # launches, cells and seconds of the grid call included
    assert tuple(x.tobytes() for x in s.m.grid_download()) + (s.m.grid_planes().tobytes(), s.m.grid_plane_eq().tobytes()) == grid


def test_looking_away(three):
    s, pl = three
    T = look_at(THREE_EYE, 2.0 * np.array(THREE_EYE) - np.array(THREE_TARGET), up=(0.0, 0.0, -1.0))
    want = s.check(32, 24, pinhole_invK(32, 24, 40.0), T)
    assert want["n_hit"] == 0 and not want["depth"].any() and np.all(want["cell"] == -1)
    got = s.m.render_download()
    assert not got["cloud"].view(np.uint8).any() and np.all(got["plane_id"] == -1)


# ---- occlusion, ties, depth limits ---------------------------------------------------------------------------------------------------
FAR_WALL, NEAR_WALL = [1.0, 0.0, 0.0, -4.0], [1.0, 0.0, 0.0, -2.0]
AXIS_T = look_at([0.0, 0.0, 0.0], [1.0, 0.0, 0.0])


def test_occluder_in_front_of_a_wall(built):
    g, pl = _graph([FAR_WALL, NEAR_WALL])
    rng = np.random.default_rng(32)
    clouds = [patch(rng, FAR_WALL, (-3.6, 3.6), (-2.6, 2.6), 0.04), patch(rng, NEAR_WALL, (-0.4, 0.5), (-0.3, 0.4), 0.04)]
    m = P.Map(g, sum(len(c) for c in clouds)); fill(m, clouds, pl)
    m.build_grid(cell=0.05)
    want = Scene(g, m).check(48, 32, pinhole_invK(48, 32, 30.0), AXIS_T)
    near = want["plane_id"] == pl[1]
    assert want["n_hit"] == 48 * 32 and 50 < near.sum() < 800            # the occluder covers the middle, the wall the rest
    assert np.all(want["depth"][near] == 2.0) and np.all(want["depth"][~near] == 4.0)
    m.close(); g.close()


def test_two_landmarks_on_one_plane(built):
    """the same plane twice: equal z on every shared pixel, the earlier row (the lower id) keeps it"""
    g, pl = _graph([NEAR_WALL, NEAR_WALL])
    rng = np.random.default_rng(33)
    clouds = [patch(rng, NEAR_WALL, (-1.0, 0.3), (-1.0, 1.0), 0.04), patch(rng, NEAR_WALL, (-0.3, 1.0), (-1.0, 1.0), 0.04)]
    m = P.Map(g, sum(len(c) for c in clouds)); fill(m, clouds, [pl[1], pl[0]])           # (the higher id first in the store: the order is the ids')
    m.build_grid(cell=0.05)
    s = Scene(g, m)
    assert s.planes["plane_id"].tolist() == sorted(pl) and np.array_equal(s.eq[0], s.eq[1])
    w, h = 48, 32
    iK = pinhole_invK(w, h, 30.0)
    want = s.check(w, h, iK, AXIS_T, reach=0)
    # a pixel is shared if either landmark alone would answer it: render each alone through the statement
    alone = [ref_render(w, h, iK, AXIS_T, s.planes[r:r + 1], s.eq[r:r + 1], s.info["inv_cell"], s.pts, s.ij, 0) for r in (0, 1)]
    shared = (alone[0]["plane_id"] >= 0) & (alone[1]["plane_id"] >= 0)
    assert shared.sum() > 100 and np.all(want["plane_id"][shared] == min(pl))
    assert np.any(want["plane_id"] == max(pl))
    m.close(); g.close()


def test_depth_limits_cut_a_wall_in_half(built):
    """a wall seen at a slant: z grows across the image, z_far (then z_near) at its middle keeps one half each, and both halves make the whole"""
    wall = [1.0, 1.0, 0.0, -3.0]
    g, pl = _graph([wall])
    rng = np.random.default_rng(34)
    cloud = patch(rng, wall, (-4.0, 4.0), (-2.0, 2.0), 0.04)
    m = P.Map(g, len(cloud)); fill(m, [cloud], pl)
    m.build_grid(cell=0.05)
    s = Scene(g, m)
    w, h = 48, 32
    iK = pinhole_invK(w, h, 30.0)
    whole = s.check(w, h, iK, AXIS_T)
    mid = float(np.median(whole["depth"][whole["plane_id"] >= 0]))
    near = s.check(w, h, iK, AXIS_T, z_far=mid)
    far = s.check(w, h, iK, AXIS_T, z_near=np.nextafter(mid, np.inf))
    assert whole["n_hit"] > 1000 and near["n_hit"] + far["n_hit"] == whole["n_hit"] and min(near["n_hit"], far["n_hit"]) > 0.3 * whole["n_hit"]
    assert near["depth"].max() <= mid < far["depth"][far["plane_id"] >= 0].min()
    m.close(); g.close()


# ---- what the grid call decided: min_count, the rule, the posed map --------------------------------------------------------------------
def test_min_count_2(built):
    """two frames over one wall, the second covers half of it: with min_count = 2 only the cells both frames reached answer"""
    g, pl = _graph([NEAR_WALL])
    rng = np.random.default_rng(35)
    clouds = [patch(rng, NEAR_WALL, (-1.0, 1.0), (-1.0, 1.0), 0.05), patch(rng, NEAR_WALL, (-1.0, 0.0), (-1.0, 1.0), 0.05)]
    m = P.Map(g, sum(len(c) for c in clouds)); fill(m, clouds, [pl[0], pl[0]])
    w, h = 48, 32
    iK = pinhole_invK(w, h, 30.0)
    m.build_grid(cell=0.05, min_count=1)
    one = Scene(g, m).check(w, h, iK, AXIS_T, reach=0)
    m.build_grid(cell=0.05, min_count=2)
    s = Scene(g, m)
    two = s.check(w, h, iK, AXIS_T, reach=0)
    assert s.counts.min() >= 2 and 0.2 * one["n_hit"] < two["n_hit"] < 0.7 * one["n_hit"]
    assert np.all(one["plane_id"][two["plane_id"] >= 0] >= 0)
    m.close(); g.close()


def test_oldest_rule_colours(built):
    """three frames over the same wall: the view has the colours of the first frame under PPS_GRID_OLDEST, of the last under NEWEST"""
    g, pl = _graph([NEAR_WALL])
    rng = np.random.default_rng(36)
    clouds = [patch(rng, NEAR_WALL, (-1.0, 1.0), (-1.0, 1.0), 0.025) for _ in range(3)]
    for f, c in enumerate(clouds):
        c["rgba"] = (c["rgba"] & np.uint32(0xFFFFFF00)) | np.uint32(f + 1)              # the frame, in the low byte
    m = P.Map(g, sum(len(c) for c in clouds)); fill(m, clouds, [pl[0]] * 3)
    w, h = 48, 32
    iK = pinhole_invK(w, h, 30.0)
    seen = {}
    for rule in (OLDEST, NEWEST):
        m.build_grid(cell=0.05, rule=rule)
        want = Scene(g, m).check(w, h, iK, AXIS_T)
        seen[rule] = want["cloud"]["rgba"][want["plane_id"] >= 0] & np.uint32(0xFF)
    assert len(seen[OLDEST]) > 1000 and np.mean(seen[OLDEST] == 1) > 0.9 and np.mean(seen[NEWEST] == 3) > 0.9
    m.close(); g.close()


def test_posed_grid_after_a_pose_change(built):
    g, pl = _graph([NEAR_WALL])
    rng = np.random.default_rng(37)
    cloud = patch(rng, NEAR_WALL, (-0.5, 0.5), (-0.4, 0.4), 0.04)
    m = P.Map(g, len(cloud)); fill(m, [cloud], pl)
    T0 = pose(np.eye(3), [0.0, 0.0, 1.0])                                # the capture pose: the estimate of pose node 0
    m.set_frame_pose(0, 0, T0)
    w, h = 48, 32
    iK = pinhole_invK(w, h, 30.0)
    m.build_grid(cell=0.05, posed=True)
    before = Scene(g, m).check(w, h, iK, AXIS_T)
    g.set_pose(0, [0.0, 0.6, 1.0, 0, 0, 0, 1])                           # the frame's pose moves 0.6 m along the wall
    m.build_grid(cell=0.05, posed=True)
    s = Scene(g, m)
    after = s.check(w, h, iK, AXIS_T)
    assert m.posed_last()["n_unposed_frames"] == 0
    cols = lambda v: np.flatnonzero((v["plane_id"] >= 0).any(axis=0))
    assert before["n_hit"] > 200 and after["n_hit"] > 200
    shift = np.mean(after["cloud"]["y"][after["plane_id"] >= 0]) - np.mean(before["cloud"]["y"][before["plane_id"] >= 0])
    assert abs(shift - 0.6) < 0.05 and cols(after).mean() != cols(before).mean()          # the view follows the moved cells
    m.build_grid(cell=0.05)                                              # ... and the unposed grid is where it was
    assert_view_equal(m.render(w, h, iK, AXIS_T), before)
    m.close(); g.close()


# ---- many landmarks, many pixels -----------------------------------------------------------------------------------------------------
def test_300_landmarks(built):
    """300 walls x = 2 .. 5 in no order of depth, a cluster of four points each: the landmark table passes through LDS in two slices"""
    depth = [2.0 + 0.01 * ((k * 37) % 300) for k in range(300)]
    g, pl = _graph([[1.0, 0.0, 0.0, -d] for d in depth])
    rng = np.random.default_rng(38)
    m = P.Map(g, 1200)
    for f in range(5):
        cloud, pid = [], []
        for k in range(60):
            c = rng.uniform(-1.0, 1.0, size=2) * [1.3, 0.9]
            cloud.append(points(on_plane(np.array([1.0, 0.0, 0.0, -depth[60 * f + k]]), c + rng.uniform(0.0, 0.12, size=(4, 2))), rng))
            pid.append(np.full(4, k, np.int32))
        m.debug_add_points(np.concatenate(cloud), np.concatenate(pid), f, pl[60 * f:60 * f + 60])
    m.build_grid(cell=0.05)
    s = Scene(g, m)
    assert len(s.planes) == 300 and np.all(s.planes["count"] > 0)
    want = s.check(64, 48, pinhole_invK(64, 48, 40.0), AXIS_T, reach=2)
    ids = np.unique(want["plane_id"][want["plane_id"] >= 0])
    assert len(ids) > 100 and ids.min() < pl[255] < ids.max()            # rows of both slices
    m.close(); g.close()


def test_640x480_of_50000_cells(built):
    ground, left, right = [0.0, 0.0, 1.0, 1.2], [0.0, 1.0, 0.0, 3.0], [0.0, -1.0, 0.0, 3.0]
    g, pl = _graph([ground, left, right])
    rng = np.random.default_rng(39)
    clouds = [patch(rng, ground, (-3.0, 3.0), (0.0, 8.5), 0.05, keep=0.95), patch(rng, left, (-8.5, 8.5), (-1.2, 1.3), 0.05, keep=0.95),
              patch(rng, right, (-8.5, 8.5), (-1.2, 1.3), 0.05, keep=0.95)]
    m = P.Map(g, sum(len(c) for c in clouds)); fill(m, clouds, pl)
    m.build_grid(cell=0.05)
    s = Scene(g, m)
    assert 40000 < s.info["n_cells"] < 60000
    want = s.check(640, 480, pinhole_invK(640, 480, 500.0), look_at([0.0, 0.0, 0.0], [1.0, 0.05, -0.05]))
    assert want["n_hit"] > 0.5 * 640 * 480 and set(np.unique(want["plane_id"]).tolist()) == {-1, pl[0], pl[1], pl[2]}
    m.close(); g.close()


# ---- state ---------------------------------------------------------------------------------------------------------------------------
def test_a_failed_grid_call_ends_the_view(built):
    g, pl = _graph([NEAR_WALL])
    rng = np.random.default_rng(40)
    cloud = patch(rng, NEAR_WALL, (-0.5, 0.5), (-0.4, 0.4), 0.04)
    m = P.Map(g, len(cloud)); fill(m, [cloud], pl)
    w, h = 16, 12
    iK = pinhole_invK(w, h, 10.0)
    with pytest.raises(P.PpsError) as e:                                 # no grid yet
        m.render(w, h, iK, AXIS_T)
    assert e.value.code == P.PPS_ESTATE
    m.build_grid(cell=0.05)
    s = Scene(g, m)
    assert s.check(w, h, iK, AXIS_T)["n_hit"] > 0
    with pytest.raises(P.PpsError) as e:
        m.build_grid(cell=0.05, max_cells=1)                             # fails on the device, after the extent pass
    assert e.value.code == P.PPS_ENOMEM
    for fn in (lambda: m.render(w, h, iK, AXIS_T), m.render_download, m.render_info):
        with pytest.raises(P.PpsError) as e:
            fn()
        assert e.value.code == P.PPS_ESTATE
    m.build_grid(cell=0.05)                                              # a grid again: no view until the next render
    with pytest.raises(P.PpsError) as e:
        m.render_download()
    assert e.value.code == P.PPS_ESTATE
    s.refresh()
    assert s.check(w, h, iK, AXIS_T)["n_hit"] > 0
    m.close(); g.close()


def test_plane_eq_is_the_estimate_at_the_grid_call(built):
    g, pl = _graph([GROUND, WALL])
    rng = np.random.default_rng(41)
    clouds = [patch(rng, GROUND, (-1.0, 1.0), (-1.0, 1.0), 0.05), patch(rng, WALL, (-1.0, 1.0), (-1.0, 0.2), 0.05)]
    m = P.Map(g, sum(len(c) for c in clouds)); fill(m, clouds, pl)
    m.build_grid(cell=0.05)
    at_grid = np.stack([g.get_plane(p) for p in pl])
    np.testing.assert_array_equal(m.grid_plane_eq(), at_grid)
    s = Scene(g, m)
    w, h = 32, 24
    T = look_at([2.0, -2.0, -1.5], [0.0, 0.0, 0.0], up=(0.0, 0.0, -1.0))
    before = s.check(w, h, pinhole_invK(w, h, 25.0), T)
    g.set_plane(pl[1], np.array(WALL) + [0.05, 0.02, 0.03, 0.1])        # the estimate moves; the grid, its equations and its view do not
    assert np.abs(g.get_plane(pl[1]) - at_grid[1]).max() > 0.01
    np.testing.assert_array_equal(m.grid_plane_eq(), at_grid)
    assert_view_equal(m.render(w, h, pinhole_invK(w, h, 25.0), T), before)
    assert before["n_hit"] > 100
    m.build_grid(cell=0.05)                                              # a new grid: the new estimate
    np.testing.assert_array_equal(m.grid_plane_eq(), np.stack([g.get_plane(p) for p in pl]))
    assert np.any(m.grid_plane_eq() != at_grid)
    s.refresh()
    s.check(w, h, pinhole_invK(w, h, 25.0), T)
    m.close(); g.close()
