"""GPU: a frame against the rendered map view (pps_map_compare, csrc/pps_compare.hip).  Every output -- the plane records, the row records,
the pair list and the totals -- is compared EXACTLY with the numpy statement compare_helpers.ref_compare, which reads the view through
render_download and the map through grid_planes and grid_plane_eq, none of the compare code.  The scenes are the small made-up ones of
the render tests, fed through pps_debug_map_add_points; the frame side goes in through pps_debug_map_compare_points, and once through a
real pop-up run.  No tolerance is introduced anywhere: every accumulator is an integer."""
import numpy as np
import pytest

import pop_up_slam_amd as P
from compare_helpers import (VALID, assert_compare_equal, check_ties, mixed_frame, read_compare, ref_compare, rows_of, shifted, ties_frame)
from grid_helpers import on_plane, points
from pop_up_slam_amd import synth
from render_helpers import look_at, pinhole_invK, pose, ref_hit, ref_rays, rot_xyz
from test_gpu_map import _calib, _popup, _pose
from test_gpu_map_grid import _graph

pytestmark = pytest.mark.gpu

GROUND, WALL, TILTED = [0.0, 0.0, -1.0, 0.2], [0.6, -0.8, 0.0, 0.7], [0.3, 0.5, 0.81, 1.0]
AXIS_T = look_at([0.0, 0.0, 0.0], [1.0, 0.0, 0.0])                       # sensor z along world x, columns towards -y, rows towards -z
TOL = 0.05


def patch(rng, abcd, u, v, pitch, keep=1.0, lift=0.004):
    """points of a landmark: a raster of plane coordinates [u0, u1] x [v0, v1] at `pitch`, jittered inside the pitch and lifted a few
    millimetres off the plane, a fraction `keep` of them kept"""
    uu, vv = np.meshgrid(np.arange(u[0], u[1], pitch), np.arange(v[0], v[1], pitch), indexing="xy")
    uv = np.stack([uu.ravel(), vv.ravel()], axis=1) + rng.uniform(0.0, 0.3 * pitch, size=(uu.size, 2))
    uv = uv[rng.random(len(uv)) < keep]
    return points(on_plane(np.asarray(abcd, dtype=np.float64), uv, rng.normal(size=len(uv)) * lift), rng)


class Scene:
    """a map with a grid: its plane table and equations (taken once per grid), the last view, and the check of a frame against it"""

    def __init__(self, g, m):
        self.g, self.m = g, m
        self.refresh()

    def refresh(self):
        self.planes, self.eq = self.m.grid_planes(), self.m.grid_plane_eq()

    def render(self, w, h, invK, T_wc, reach=1):
        self.view = self.m.render(w, h, invK, T_wc, reach)
        self.r = rows_of(self.view["plane_id"], self.planes)
        return self.view

    def check(self, cloud, fid, nplanes, tol=TOL):
        rec = self.m.debug_compare(cloud, fid, nplanes, tol)
        got = read_compare(self.m, rec)
        want = ref_compare(self.view["plane_id"], self.planes, self.eq, cloud, fid, nplanes, tol)
        assert_compare_equal(got, want)
        t = got["totals"]
        assert t["launches"] == 3 and t["sec"] > 0.0 and t["tol"] == tol
        return want


def make(planes, clouds, cell=0.05, nodes=None):
    g, pl = _graph(planes)
    m = P.Map(g, sum(len(c) for c in clouds))
    for k, cloud in enumerate(clouds):
        m.debug_add_points(cloud, np.zeros(len(cloud), np.int32), k, [pl[k] if nodes is None else pl[nodes[k]]])
    m.build_grid(cell=cell)
    return Scene(g, m), pl


# ---- a ground, a wall and a tilted plane ---------------------------------------------------------------------------------------------
THREE_EYE, THREE_TARGET = [2.6, -2.4, -1.6], [-0.2, 0.2, 0.1]


def three_poses():
    T0 = look_at(THREE_EYE, THREE_TARGET, up=(0.0, 0.0, -1.0))
    R = np.asarray(T0[:3, :3], dtype=np.float64) @ rot_xyz(0.25, -0.2, 0.4)
    return [T0, pose(R, [2.2, -2.0, -1.2])]


@pytest.fixture(scope="module")
def three(built):
    rng = np.random.default_rng(71)
    clouds = [patch(rng, GROUND, (-2.0, 2.0), (-2.0, 2.0), 0.03, keep=0.8), patch(rng, WALL, (-2.0, 2.0), (-1.5, 0.2), 0.03, keep=0.8),
              patch(rng, TILTED, (-1.0, 1.0), (-1.0, 1.0), 0.03, keep=0.8)]
    s, pl = make([GROUND, WALL, TILTED], clouds)
    yield s, pl
    s.m.close(); s.g.close()


@pytest.mark.parametrize("size", [(1, 1), (5, 3), (17, 9), (64, 48), (257, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_three_planes_shifted_along_the_normals(three, size):
    """the frame is the view's own cloud, every point moved along its landmark's normal by offsets on both sides of tol"""
    s, pl = three
    w, h = size
    rng = np.random.default_rng(72 + w)
    s.render(w, h, pinhole_invK(w, h, 0.7 * max(w, h)), three_poses()[0])
    off = rng.choice([0.0, 0.5, 0.98, 1.02, -0.98, -1.02, 2.0, -6.0], size=(h, w)) * TOL
    cloud = shifted(s.view["cloud"], s.r, s.eq, off)
    fid = np.where(s.r >= 0, (s.r + 1) % 3, rng.integers(-1, 3, size=(h, w))).astype(np.int32)
    fid[rng.random((h, w)) < 0.1] = -1
    want = s.check(cloud, fid, 3)
    if size == (64, 48):
        t = want["totals"]
        assert want["planes"]["best_plane_id"].tolist() == [pl[2], pl[0], pl[1]] and t["n_pairs"] == 3
        assert t["n_both"] > 100
        assert np.all(want["pairs"]["n_agree"] > 0.2 * want["pairs"]["n"]) and np.all(want["pairs"]["n_agree"] < 0.8 * want["pairs"]["n"])
    if size == (1, 1):
        assert want["totals"]["n_both"] + want["totals"]["n_view_only"] == 1


def test_margins_and_junk(three):
    s, pl = three
    w, h = 64, 48
    rng = np.random.default_rng(73)
    s.render(w, h, pinhole_invK(w, h, 0.7 * w), three_poses()[1])      # (the three landmarks and the empty background)
    cloud, fid = mixed_frame(rng, s.view["cloud"], s.r, s.eq, 3, TOL)
    want = s.check(cloud, fid, 3)
    t = want["totals"]
    assert min(t["n_both"], t["n_frame_only"], t["n_view_only"], t["n_neither"]) > 0 and t["n_bad_id"] == 6
    # valid points at infinity, NaN and 1e30 on pixels that show a landmark: q saturates
    at = np.flatnonzero(s.r.reshape(-1) >= 0)[:6]
    flat_c, flat_id = cloud.reshape(-1), fid.reshape(-1)
    for i, v in zip(at, (np.inf, -np.inf, np.nan, 1e30, -1e30, 3e38)):
        flat_c["x"][i] = v; flat_c["rgba"][i] |= VALID; flat_id[i] = 1
    s.check(cloud, fid, 3)
    # ids beyond nplanes count as junk when fewer frame planes are asked for; a frame without any valid pixel
    want = s.check(cloud, fid, 1)
    assert want["totals"]["n_bad_id"] > 100
    cloud["rgba"] &= ~VALID
    want = s.check(cloud, fid, 3)
    assert want["totals"]["n_both"] == want["totals"]["n_frame_only"] == 0 and want["totals"]["n_pairs"] == 0


def test_best_landmark_ties(three):
    s, pl = three
    w, h = 64, 48
    s.render(w, h, pinhole_invK(w, h, 45.0), three_poses()[0])
    assert all(np.count_nonzero(s.r == row) >= 20 for row in range(3))
    cloud, fid = ties_frame(np.random.default_rng(74), s.view["cloud"], s.r, s.eq, TOL)
    check_ties(s.check(cloud, fid, 4), pl)


def test_the_frame_of_the_same_planes_finds_its_landmarks(three):
    """the property: the frame is what a pop-up of the three planes at the render's pose gives (the point of every pixel's ray on the
    plane the view shows there, computed from the plane equations), frame plane k showing landmark PAIR[k]"""
    s, pl = three
    w, h = 64, 48
    iK, T = pinhole_invK(w, h, 45.0), three_poses()[0]
    s.render(w, h, iK, T)
    PAIR = [2, 0, 1]
    row, col = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    o, ds, dw = ref_rays(col, row, iK, T)
    cloud = np.zeros((h, w), dtype=P.POINT_DTYPE); fid = np.full((h, w), -1, dtype=np.int32)
    for k, r in enumerate(PAIR):
        ok, _, xf, _, _ = ref_hit(o, ds, dw, s.eq[r], 20.0)
        at = ok & (s.r == r)
        for i, name in enumerate("xyz"):
            cloud[name][at] = xf[i][at]
        cloud["rgba"][at] = VALID | np.uint32(k); fid[at] = k
    want = s.check(cloud, fid, 3)
    assert want["planes"]["best_plane_id"].tolist() == [pl[r] for r in PAIR] and np.all(want["planes"]["n_new"] == 0)
    assert np.all(want["planes"]["best_agree"] == want["planes"]["n_valid"]) and np.all(want["planes"]["n_valid"] > 20)
    assert want["totals"]["n_pairs"] == 3 and np.all(np.abs(want["pairs"]["sum_q"]) <= want["pairs"]["n"])       # (within a quantum)
    # the wall's frame points three tolerances off their plane: nothing confirms that frame plane, and nothing of it is new
    k = PAIR.index(1)
    moved = cloud.copy()
    sh = shifted(cloud, np.where(fid == k, 1, -1), s.eq, 3.0 * TOL)
    for name in "xyz":
        moved[name] = sh[name]
    want = s.check(moved, fid, 3)
    p = want["planes"][k]
    assert (p["best_row"], p["best_plane_id"], p["best_n"], p["best_agree"], p["n_new"]) == (-1, -1, 0, 0, 0) and p["n_valid"] > 20
    others = [j for j in range(3) if j != k]
    assert want["planes"]["best_plane_id"][others].tolist() == [pl[PAIR[j]] for j in others]
    wall = want["pairs"][want["pairs"]["frame_plane"] == k]
    assert len(wall) == 1 and wall["n_agree"][0] == 0 and abs(abs(wall["sum_q"][0]) / (4096.0 * wall["n"][0]) - 3.0 * TOL) < 1e-3


# ---- 64 pixels, 64 entries ---------------------------------------------------------------------------------------------------------------
def strips(rng, w, h, f, n, pitch):
    """n walls x = 2 + 0.05 j, wall j a strip that only the columns [j w / n, (j + 1) w / n) of a w x h view along x (focal length f) see"""
    planes, clouds = [], []
    cx, per = 0.5 * (w - 1), w // n
    for j in range(n):
        d = 2.0 + 0.05 * j
        c0, c1 = j * per, (j + 1) * per - 1
        y = (-(c1 - cx + 0.3) / f * d, -(c0 - cx - 0.3) / f * d)          # (u = y and v = z on a wall x = d)
        z = 0.5 * h / f * d + 0.1
        planes.append([1.0, 0.0, 0.0, -d]); clouds.append(patch(rng, planes[-1], y, (-z, z), pitch, lift=0.001))
    return planes, clouds


@pytest.mark.parametrize("size,f", [((64, 1), 16.0), ((8, 8), 8.0)], ids=["64x1", "8x8"])
def test_64_pixels_of_64_entries_and_of_one(built, size, f):
    """every pixel of one wave with a table entry of its own: the longest key loop, more keys than a workgroup's table takes without
    probing; then all 64 pixels on one entry"""
    w, h = size
    rng = np.random.default_rng(75)
    px = np.arange(64).reshape(h, w)
    iK = pinhole_invK(w, h, f)
    # 64 frame planes against one landmark
    s, pl = make([[1.0, 0.0, 0.0, -2.0]], [patch(rng, [1.0, 0.0, 0.0, -2.0], (-5.0, 5.0), (-1.5, 1.5), 0.03)])
    s.render(w, h, iK, AXIS_T)
    assert np.all(s.r == 0)
    cloud = shifted(s.view["cloud"], s.r, s.eq, rng.choice([0.3, -0.8, 1.2, -2.0], size=(h, w)) * TOL)
    want = s.check(cloud, px, 64)
    assert want["totals"]["n_pairs"] == 64 and np.all(want["pairs"]["n"] == 1) and want["pairs"]["frame_plane"].tolist() == list(range(64))
    want = s.check(cloud, np.full((h, w), 17), 64)
    assert want["totals"]["n_pairs"] == 1 and want["pairs"]["n"][0] == 64 and want["planes"]["n_valid"][17] == 64
    s.m.close(); s.g.close()
    # 8 frame planes x 8 landmarks
    planes, clouds = strips(rng, w, h, f, 8, 0.012)
    s, pl = make(planes, clouds, cell=0.02)
    s.render(w, h, iK, AXIS_T)
    assert np.array_equal(s.r, np.broadcast_to(np.arange(w) // (w // 8), (h, w)))
    k = (px // w if h > 1 else px % 8).astype(np.int32)                  # 8 x 8: the image row; 64 x 1: the column inside its strip
    cloud = shifted(s.view["cloud"], s.r, s.eq, rng.choice([0.3, -0.8, 1.2, -2.0], size=(h, w)) * TOL)
    want = s.check(cloud, k, 8)
    assert want["totals"]["n_pairs"] == 64 and np.all(want["pairs"]["n"] == 1) and np.all(want["rows"]["n_view"] == 8)
    at = s.r == 5
    one = np.where(at, 3, -1).astype(np.int32)
    want = s.check(cloud, one, 8)
    assert want["totals"]["n_pairs"] == 1 and want["pairs"]["n"][0] == 8 and want["totals"]["n_view_only"] == 56
    s.m.close(); s.g.close()


def test_more_entries_than_a_workgroup_table_holds(built):
    """780 x 1: the pixels of ONE workgroup carry some 780 different entries (65 frame planes x 12 landmarks), twelve times the slots of
    its table in LDS: most of them go to memory wave by wave"""
    w, h, f = 780, 1, 48.75
    rng = np.random.default_rng(76)
    planes, clouds = strips(rng, w, h, f, 12, 0.012)
    s, pl = make(planes, clouds, cell=0.02)
    s.render(w, h, pinhole_invK(w, h, f), AXIS_T)
    assert len(np.unique(s.r[s.r >= 0])) == 12
    k = (np.arange(w) % 65).reshape(1, w).astype(np.int32)
    cloud = shifted(s.view["cloud"], s.r, s.eq, rng.normal(size=(h, w)) * TOL)
    want = s.check(cloud, k, 65)
    assert want["totals"]["n_pairs"] > 700 and want["pairs"]["n"].max() <= 2
    s.m.close(); s.g.close()


# ---- many pixels, many landmarks -----------------------------------------------------------------------------------------------------
def test_640x480_of_one_entry(built):
    """one wall fills the view: every workgroup adds to the same four counters"""
    wall = [1.0, 0.0, 0.0, -4.0]
    rng = np.random.default_rng(77)
    s, pl = make([wall], [patch(rng, wall, (-3.6, 3.6), (-2.6, 2.6), 0.04)])
    w, h = 640, 480
    s.render(w, h, pinhole_invK(w, h, 500.0), AXIS_T, reach=2)
    assert np.all(s.r == 0)
    cloud = shifted(s.view["cloud"], s.r, s.eq, rng.normal(size=(h, w)) * TOL)
    want = s.check(cloud, np.zeros((h, w), np.int32), 1)
    assert want["pairs"]["n"].tolist() == [307200] and 0.6 * 307200 < want["pairs"]["n_agree"][0] < 0.75 * 307200
    assert want["planes"]["best_plane_id"].tolist() == [pl[0]] and want["rows"]["n_view"].tolist() == [307200]
    s.m.close(); s.g.close()


def test_640x480_of_50000_cells(built):
    ground, left, right = [0.0, 0.0, 1.0, 1.2], [0.0, 1.0, 0.0, 3.0], [0.0, -1.0, 0.0, 3.0]
    rng = np.random.default_rng(78)
    clouds = [patch(rng, ground, (-3.0, 3.0), (0.0, 8.5), 0.05, keep=0.95), patch(rng, left, (-8.5, 8.5), (-1.2, 1.3), 0.05, keep=0.95),
              patch(rng, right, (-8.5, 8.5), (-1.2, 1.3), 0.05, keep=0.95)]
    s, pl = make([ground, left, right], clouds)
    assert 40000 < s.m.grid_info()["n_cells"] < 60000
    w, h = 640, 480
    s.render(w, h, pinhole_invK(w, h, 500.0), look_at([0.0, 0.0, 0.0], [1.0, 0.05, -0.05]))
    cloud, fid = mixed_frame(rng, s.view["cloud"], s.r, s.eq, 5, TOL)
    want = s.check(cloud, fid, 5)
    assert want["totals"]["n_pairs"] == 15 and want["totals"]["n_both"] > 0.3 * w * h
    s.m.close(); s.g.close()


def test_65_planes_against_300_landmarks(built):
    """300 walls, a cluster of four points each: a table of 66 x 301; the pair list read in ranges"""
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
    w, h = 64, 48
    s.render(w, h, pinhole_invK(w, h, 40.0), AXIS_T, reach=2)
    assert len(s.planes) == 300 and len(np.unique(s.r)) > 100
    rng = np.random.default_rng(79)
    cloud = shifted(s.view["cloud"], s.r, s.eq, rng.normal(size=(h, w)) * TOL)
    fid = rng.integers(-1, 65, size=(h, w)).astype(np.int32)
    want = s.check(cloud, fid, 65)
    n = want["totals"]["n_pairs"]
    assert n > 100 and m.compare_info()["n_rows"] == 300
    cut = n // 3
    np.testing.assert_array_equal(np.concatenate([m.compare_pairs(0, cut), m.compare_pairs(cut, n - cut)]), want["pairs"])
    assert len(m.compare_pairs(n, 0)) == 0 and len(m.compare_pairs(0, 0)) == 0
    for first, count in ((0, n + 1), (n, 1), (n + 1, 0), (-1, 1), (0, -1)):
        with pytest.raises(P.PpsError) as e:
            m.compare_pairs(first, count)
        assert e.value.code == P.PPS_EINVAL
    np.testing.assert_array_equal(m.compare_pairs(), want["pairs"])      # (a refused range leaves the comparison readable)
    m.close(); g.close()


# ---- a real pop-up run ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [1, 2])
def test_a_pop_up_run_and_its_download_compare_alike(three, step):
    s, pl = three
    w, h = 160, 120
    pp, K = _popup(w, h)
    seg, polys, T = synth.corridor_frame(_pose(0), width=w, height=h, K=K)
    assert pp.run(seg, T, polys, step=step, depth_thre=10.0, ceiling_thre=2.5) > 0
    _, cloud, _, pid = pp.download()
    s.render(w, h, pinhole_invK(w, h, 110.0), three_poses()[0])
    rec = s.m.compare(pp, 4, TOL)
    run = read_compare(s.m, rec)
    want = s.check(cloud, pid, 4)                                        # the hook on the downloaded pixels, and the statement
    assert_compare_equal(run, want)
    assert run["planes"].tobytes() == want["planes"].tobytes() and run["pairs"].tobytes() == want["pairs"].tobytes()
    t = want["totals"]
    assert t["n_both"] > 100 and t["n_bad_id"] == 0
    if step == 2:
        odd = (np.arange(w)[None, :] % 2 == 1) | (np.arange(h)[:, None] % 2 == 1)
        assert np.all(pid[odd] == -1) and t["n_both"] + t["n_frame_only"] <= np.count_nonzero(~odd)
    # a run of another size is refused, and so is a context without a run; the comparison stays
    small, _ = _popup(80, 60)
    with pytest.raises(P.PpsError) as e:
        s.m.compare(small, 4, TOL)
    assert e.value.code == P.PPS_ESTATE
    seg2, polys2, T2 = synth.corridor_frame(_pose(0), width=80, height=60, K=_calib(80, 60)[0])
    small.run(seg2, T2, polys2, step=1)
    with pytest.raises(P.PpsError) as e:
        s.m.compare(small, 4, TOL)
    assert e.value.code == P.PPS_EINVAL and "pixels" in str(e.value)
    assert_compare_equal(read_compare(s.m, rec), want)
    small.close(); pp.close()


# ---- state ---------------------------------------------------------------------------------------------------------------------------
def _gone(m):
    for fn in (m.compare_info, m.compare_rows, m.compare_pairs):
        with pytest.raises(P.PpsError) as e:
            fn()
        assert e.value.code == P.PPS_ESTATE


def test_two_comparisons_give_the_same_bytes_and_change_nothing(three):
    s, pl = three
    w, h = 64, 48
    rng = np.random.default_rng(80)
    s.render(w, h, pinhole_invK(w, h, 45.0), three_poses()[1])
    cloud, fid = mixed_frame(rng, s.view["cloud"], s.r, s.eq, 3, TOL)
    m = s.m
    snap = lambda: (tuple(v.tobytes() for v in m.render_download().values()), m.render_info(), tuple(a.tobytes() for a in m.grid_download()),
                    m.grid_info(), m.grid_planes().tobytes(), m.grid_plane_eq().tobytes(), m.download(0).tobytes(), m.chunks().tobytes(), m.info())
    before = snap()
    a = read_compare(m, m.debug_compare(cloud, fid, 3, TOL))
    b = read_compare(m, m.debug_compare(cloud, fid, 3, TOL))
    for k in ("planes", "rows", "pairs"):
        assert a[k].tobytes() == b[k].tobytes(), k
    strip = lambda t: {k: v for k, v in t.items() if k != "sec"}
    assert strip(a["totals"]) == strip(b["totals"]) and snap() == before
    # a frame of the wrong size is refused; the comparison before stays readable
    with pytest.raises(P.PpsError) as e:
        m.debug_compare(cloud.reshape(-1)[:-1], fid.reshape(-1)[:-1], 3, TOL)
    assert e.value.code == P.PPS_EINVAL
    for bad in (dict(nplanes=0), dict(nplanes=66), dict(tol=-1.0), dict(tol=np.nan)):
        with pytest.raises(P.PpsError) as e:
            m.debug_compare(cloud, fid, **{**dict(nplanes=3, tol=TOL), **bad})
        assert e.value.code == P.PPS_EINVAL
    again = read_compare(m, b["planes"])
    assert again["rows"].tobytes() == b["rows"].tobytes() and again["pairs"].tobytes() == b["pairs"].tobytes() and again["totals"] == b["totals"]
    # another tolerance, another count of frame planes: a new comparison replaces the old one
    c = s.check(cloud, fid, 2, 0.0)
    assert c["totals"]["nplanes"] == 2 and m.compare_info()["tol"] == 0.0


def test_what_ends_the_view_ends_the_comparison(built):
    wall = [1.0, 0.0, 0.0, -2.0]
    rng = np.random.default_rng(81)
    s, pl = make([wall], [patch(rng, wall, (-0.5, 0.5), (-0.4, 0.4), 0.04)])
    m = s.m
    w, h = 16, 12
    iK = pinhole_invK(w, h, 10.0)
    frame = lambda: (shifted(s.view["cloud"], s.r, s.eq, 0.01), np.where(s.r >= 0, 0, -1).astype(np.int32))
    _gone(m)
    s.render(w, h, iK, AXIS_T)
    _gone(m)                                                             # a view alone is no comparison
    assert s.check(*frame(), 1)["totals"]["n_both"] > 0
    s.render(w, h, iK, AXIS_T)                                           # a new render
    _gone(m)
    s.check(*frame(), 1)
    m.build_grid(cell=0.05)                                              # a grid call
    _gone(m)
    with pytest.raises(P.PpsError) as e:
        m.debug_compare(*frame(), 1)
    assert e.value.code == P.PPS_ESTATE                                  # (no view either)
    s.refresh(); s.render(w, h, iK, AXIS_T)
    s.check(*frame(), 1)
    with pytest.raises(P.PpsError) as e:
        m.build_grid(cell=0.05, max_cells=1)                             # a grid call that fails
    assert e.value.code == P.PPS_ENOMEM
    _gone(m)
    m.build_grid(cell=0.04)                                              # the tables follow the new grid
    s.refresh(); s.render(w, h, iK, AXIS_T)
    assert s.check(*frame(), 1)["totals"]["n_both"] > 0
    with pytest.raises(P.PpsError):
        m.render(0, h, iK, AXIS_T)                                       # a render that is refused leaves view and comparison
    assert m.compare_info()["n_both"] > 0
    m.close(); s.g.close()
