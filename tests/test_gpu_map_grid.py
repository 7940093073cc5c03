"""GPU: the grid map (pps_map_build_grid, csrc/pps_grid.hip).  Everything grid_download, grid_planes and grid_info return is compared
EXACTLY with the numpy statement of grid_helpers.ref_grid, which reads the map pps_map_build wrote for the same selection, the live node
ids, and the frames / inv_cell the library published; the emitted points are additionally compared with download(1)[src] as raw records.
The frames go in through pps_debug_map_add_points unless stated otherwise.  No tolerance is introduced anywhere."""
import os

import numpy as np
import pytest

import pop_up_slam_amd as P
from grid_helpers import NEWEST, OLDEST, on_plane, one_point_frame, points, ref_grid, scan_frame
from map_helpers import confetti_frame, raw16, runs_frame, wave_pattern_frame
from pop_up_slam_amd import synth
from test_gpu_map import _popup, _pose

pytestmark = pytest.mark.gpu

GROUND, WALL = [0.0, 0.0, -1.0, 0.2], [0.6, -0.8, 0.0, 0.7]
INFO_KEYS = ("n_points", "n_cells", "n_in", "n_dropped", "n_passed_through", "n_planes")
ZEROS = dict(n_points=0, n_cells=0, n_in=0, n_dropped=0, n_passed_through=0, n_planes=0, launches=0, cell=0.0, inv_cell=0.0, sec=(0.0,) * 4)


def _graph(planes):
    """plane landmarks the build can read the estimate of: every node carries a prior, nothing is optimised"""
    g = P.Graph()
    pose = g.add_pose([0, 0, 1, 0, 0, 0, 1])
    g.add_pose_prior(pose, np.zeros(6), synth._ut_diag([1.0] * 6))
    pl = []
    for abcd in planes:
        pl.append(g.add_plane(list(abcd)))
        g.add_plane_prior(pl[-1], g.get_plane(pl[-1]), synth._ut_diag([300.0] * 3))
    return g, pl


def _live(g, m):
    ids = []
    for node in np.unique(m.chunks()["plane_id"]):
        try:
            g.get_plane(int(node)); ids.append(int(node))
        except P.PpsError:
            pass
    return ids


def _grid(m):
    pts, counts, ij, src = m.grid_download()
    info = m.grid_info()
    return dict(planes=m.grid_planes(), pts=pts, counts=counts, ij=ij, src=src, totals={k: info[k] for k in INFO_KEYS}), info


def _check(g, m, sel=None, cell=0.02, rule=NEWEST, min_count=1, max_cells=1 << 26):
    """build_grid against the statement; returns (the expected grid, B)"""
    ret = m.build_grid(sel, cell=cell, rule=rule, min_count=min_count, max_cells=max_cells)
    got, info = _grid(m)
    m.build(sel)
    B = m.download(1)
    want = ref_grid(B, m.built_chunks(), _live(g, m), got["planes"], info["inv_cell"], rule, min_count)
    assert got["totals"] == want["totals"]
    assert ret == (want["totals"]["n_cells"], want["totals"]["n_planes"])
    assert info["cell"] == cell and info["inv_cell"] == 1.0 / cell
    for k in want["planes"].dtype.names:
        np.testing.assert_array_equal(got["planes"][k], want["planes"][k], err_msg=k)
    for p in got["planes"]:                                              # the frames: the library's, from the estimate get_plane returns
        n, e1, e2 = P.map_grid_frame_host(g.get_plane(int(p["plane_id"])))
        np.testing.assert_array_equal(p["n"], n); np.testing.assert_array_equal(p["e1"], e1); np.testing.assert_array_equal(p["e2"], e2)
    np.testing.assert_array_equal(got["src"], want["src"])
    np.testing.assert_array_equal(got["counts"], want["counts"])
    np.testing.assert_array_equal(got["ij"], want["ij"])
    np.testing.assert_array_equal(raw16(got["pts"]), raw16(want["pts"]))
    np.testing.assert_array_equal(raw16(got["pts"]), raw16(B[got["src"]]))
    if want["totals"]["n_in"] > 0:
        assert info["launches"] >= 5 and info["sec"][0] > 0.0 and info["sec"][3] >= info["sec"][0]
    # pieces of the grid: any range, any subset of the outputs
    n = want["totals"]["n_cells"]
    if n > 3:
        a, k = n // 3, n - n // 3 - 1
        pts, counts, ij, src = m.grid_download(a, k)
        np.testing.assert_array_equal(src, want["src"][a:a + k]); np.testing.assert_array_equal(ij, want["ij"][a:a + k])
        np.testing.assert_array_equal(counts, want["counts"][a:a + k]); np.testing.assert_array_equal(raw16(pts), raw16(want["pts"][a:a + k]))
        only = np.zeros(k, dtype=np.int64)
        m._ck(m.L.pps_map_grid_download(m.h, a, k, None, None, None, only.ctypes.data))
        np.testing.assert_array_equal(only, want["src"][a:a + k])
    return want, B


# ---- the smallest grids --------------------------------------------------------------------------------------------------------------
def test_one_point_and_three_points_in_one_cell(built):
    g, pl = _graph([GROUND])
    m = P.Map(g, 16)
    m.debug_add_points(points(on_plane(np.array(GROUND), [[0.013, -0.027]], 0.02)), np.zeros(1, np.int32), 0, pl)
    want, _ = _check(g, m)
    assert want["totals"]["n_cells"] == 1 and want["ij"].tolist() == [[0, -2]] and want["planes"]["ni"][0] == 1
    m3 = P.Map(g, 16)
    uv = [[0.211, 0.305], [0.214, 0.309], [0.218, 0.301]]
    m3.debug_add_points(points(on_plane(np.array(GROUND), uv, [0.0, 0.01, -0.01])), np.zeros(3, np.int32), 0, pl)
    newest, _ = _check(g, m3, rule=NEWEST)
    oldest, _ = _check(g, m3, rule=OLDEST)
    assert newest["counts"].tolist() == [3] == oldest["counts"].tolist()
    assert newest["src"].tolist() == [2] and oldest["src"].tolist() == [0]
    m.close(); m3.close(); g.close()


# ---- a ground and a wall in three overlapping frames ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def overlapping(built):
    g, pl = _graph([GROUND, WALL])
    rng = np.random.default_rng(21)
    m = P.Map(g, 3 * 5000)
    for f in range(3):
        cloud, pid = scan_frame(rng, [GROUND, WALL], 100, 50, (-2.0 + 0.5 * f, -1.0 + 0.2 * f), 0.027)
        m.debug_add_points(cloud, pid, f, pl)
    assert m.info()["n_points"] > 12000
    yield g, m, pl
    m.close(); g.close()


@pytest.mark.parametrize("rule", [NEWEST, OLDEST], ids=["newest", "oldest"])
@pytest.mark.parametrize("cell", [0.05, 0.5])
def test_overlapping_frames(overlapping, cell, rule):
    g, m, pl = overlapping
    want, _ = _check(g, m, cell=cell, rule=rule)
    p = want["planes"]
    assert len(p) == 2 and np.all(p["i0"] < 0) and np.all(p["j0"] < 0) and np.all(p["i0"] + p["ni"] > 0)       # both sides of the origin
    assert want["counts"].max() >= 3                                     # overlapping observations
    assert np.any(np.diff(want["src"]) < 0)                              # cell order is not arrival order


@pytest.mark.parametrize("vote", ["direct"])
def test_overlapping_frames_with_direct_votes(overlapping, vote):
    """PPS_GRID_VOTE=direct: every point sends its own atomics (what tools/map_grid_bench.py measures the in-wave combining against)"""
    g, m, pl = overlapping
    os.environ["PPS_GRID_VOTE"] = vote
    try:
        _check(g, m, cell=0.05, rule=OLDEST)
    finally:
        del os.environ["PPS_GRID_VOTE"]


@pytest.mark.parametrize("min_count", [2, 3])
def test_min_count(overlapping, min_count):
    g, m, pl = overlapping
    want, _ = _check(g, m, cell=0.05, min_count=min_count)
    m.build_grid(cell=0.05, min_count=min_count - 1)
    assert 0 < want["totals"]["n_cells"] < m.grid_info()["n_cells"] and want["counts"].min() == min_count


def test_selection(overlapping):
    g, m, pl = overlapping
    sel = P.map_select(2, every_frame=0, old_age=-100, old_every=2, min_tracked=(0, 0, 0))       # frames 0 and 2
    keep = P.map_select_host(m.chunks(), sel)
    assert 0 < keep.sum() < len(keep)
    want, B = _check(g, m, sel=sel, cell=0.05)
    assert want["totals"]["n_points"] == int(m.chunks()["count"][keep].sum()) == len(B)


# ---- 65 planes -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planes65(built):
    g, pl = _graph([[np.sin(i), np.cos(i), 0.1 * i, -1.0 - 0.1 * i] for i in range(65)])
    yield g, pl
    g.close()


@pytest.mark.parametrize("cell", [40.0, 1e-3], ids=["handful", "alone"])      # 1 mm: (nearly) every point alone in its cell
def test_65_planes(planes65, cell):
    g, pl = planes65
    rng = np.random.default_rng(65)
    m = P.Map(g, 165 + 2 * 4097)
    frames = [wave_pattern_frame(rng), runs_frame(rng, 4097, 65), confetti_frame(rng, 4097, 65)]
    for f, (cloud, pid) in enumerate(frames):
        for k in "xyz":                                                  # sigma 5 cm: a 1 mm cell keeps the boxes below a million cells each
            cloud[k] = cloud[k] * np.float32(0.01)
        m.debug_add_points(cloud, pid, f, pl)
    want, _ = _check(g, m, cell=cell, max_cells=1 << 28)
    assert want["totals"]["n_planes"] == 65 and np.all(want["planes"]["n_in"] > 0)
    if cell == 40.0:
        assert np.all(want["planes"]["count"] <= 4) and want["counts"].max() > 30
    else:
        assert np.count_nonzero(want["counts"] == 1) > 0.95 * want["totals"]["n_cells"] and want["totals"]["n_cells"] > 0.97 * want["totals"]["n_in"] > 5000
    m.close()


# ---- chunk boundaries ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_b", [255, 256, 257, 511, 513])
def test_sizes_at_the_workgroup_edge(built, n_b):
    g, pl = _graph([GROUND, WALL])
    rng = np.random.default_rng(n_b)
    m = P.Map(g, 1024)
    first = n_b // 3
    m.debug_add_points(points(on_plane(np.array(GROUND), rng.uniform(-1, 1, size=(first, 2))), rng), np.zeros(first, np.int32), 0, [pl[0]])
    m.debug_add_points(points(on_plane(np.array(WALL), rng.uniform(-1, 1, size=(n_b - first, 2))), rng), np.zeros(n_b - first, np.int32), 1, [pl[1]])
    want, B = _check(g, m, cell=0.1)
    assert len(B) == n_b and want["totals"]["n_in"] == n_b
    m.close(); g.close()


def test_one_point_chunks(built):
    """300 one-point chunks spread over 7 landmarks: chunk boundaries inside every wave, a workgroup's window of 256 chunks"""
    planes = [GROUND, WALL, [1, 0, 0, -2], [0, 2, 0, 1], [0.1, 0.2, -0.9, 0.5], [0.3, 0.5, 0.81, 1.0], [-0.6, 0.1, 0.3, 0.4]]
    g, pl = _graph(planes)
    rng = np.random.default_rng(300)
    m = P.Map(g, 512)
    for f in range(5):
        cloud, pid = one_point_frame(rng, 60)
        m.debug_add_points(cloud, pid, f, [pl[int(v)] for v in rng.integers(0, 7, size=60)])
    t = m.chunks()
    assert len(t) == 300 and np.all(t["count"] == 1) and len(np.unique(t["plane_id"])) == 7
    for cell, rule in ((0.5, NEWEST), (3.0, OLDEST)):
        want, _ = _check(g, m, cell=cell, rule=rule)
    assert want["counts"].max() > 3
    m.close(); g.close()


# ---- redirect and removal ------------------------------------------------------------------------------------------------------------
def test_redirect_and_removal(built):
    g, pl = _graph([GROUND, WALL, np.array(WALL) + [0.02, 0.01, 0.0, 0.01], [1, 0, 0, -2]])
    rng = np.random.default_rng(44)
    m = P.Map(g, 4 * 1200)
    for f in range(2):
        cloud, pid = scan_frame(rng, [GROUND, WALL, WALL, [1, 0, 0, -2]], 40, 30, (-0.5, -0.4 + 0.1 * f), 0.03)
        m.debug_add_points(cloud, pid, f, pl)
    a, b, c = pl[1], pl[2], pl[3]
    before, _ = _check(g, m, cell=0.05)
    n_b = int(before["planes"]["n_in"][2]); n_c = int(before["planes"]["n_in"][3])
    m.redirect(b, a); g.remove_node(b); g.remove_node(c)
    want, B = _check(g, m, cell=0.05)
    assert want["planes"]["plane_id"].tolist() == [pl[0], a]
    assert want["planes"]["n_in"][1] == before["planes"]["n_in"][1] + n_b                # b's chunks vote in a's grid
    assert want["planes"]["n_chunks"][1] == 4
    assert want["totals"]["n_passed_through"] == n_c > 0                 # c's points are counted and appear nowhere
    gone = np.repeat(m.built_chunks()["plane_id"], m.built_chunks()["count"]) == c
    assert gone.sum() == n_c and not np.isin(np.flatnonzero(gone), want["src"]).any()
    m.close(); g.close()


# ---- dropped points ------------------------------------------------------------------------------------------------------------------
def test_dropped_points(built):
    g, pl = _graph([GROUND, WALL])
    rng = np.random.default_rng(55)
    cloud, pid = scan_frame(rng, [GROUND, WALL], 40, 30, (-0.5, -0.4), 0.03, p_valid=1.0)
    for k in (3, 200, 201, 700, 1100, 1199):                             # the pixels that will go bad belong to a plane
        pid[k] = 0 if k < 600 else 1
    clean = P.Map(g, 1200); clean.debug_add_points(cloud, pid, 0, pl)
    ref, _ = _check(g, clean, cell=0.05)
    bad = [(3, "x", np.nan), (200, "y", np.inf), (201, "z", -np.inf), (700, "x", 1e30), (1100, "y", -1e30), (1199, "z", np.nan)]
    dirty_cloud = cloud.copy()
    for k, name, v in bad:
        dirty_cloud[name][k] = v
        assert pid[k] >= 0
    m = P.Map(g, 1200); m.debug_add_points(dirty_cloud, pid, 0, pl)
    want, _ = _check(g, m, cell=0.05)
    assert want["totals"]["n_dropped"] == len(bad) and want["totals"]["n_in"] == ref["totals"]["n_in"] - len(bad)
    np.testing.assert_array_equal(want["planes"]["ni"], ref["planes"]["ni"])             # the boxes are the ordinary points'
    clean.close(); m.close(); g.close()


# ---- max_cells -----------------------------------------------------------------------------------------------------------------------
def test_max_cells(built):
    g, pl = _graph([GROUND, WALL])
    m = P.Map(g, 64)
    m.debug_add_points(points(on_plane(np.array(GROUND), [[0.1, 0.1], [0.2, 0.3], [0.25, 0.35]])), np.zeros(3, np.int32), 0, [pl[0]])
    m.debug_add_points(points(on_plane(np.array(WALL), [[0.0, 0.0], [1.0e6, 0.5]])), np.zeros(2, np.int32), 1, [pl[1]])
    m.build()
    state = lambda: (m.info(), m.built_chunks().tobytes(), m.download(1).tobytes(), m.download(0).tobytes(), m.chunks().tobytes())
    before = state()
    _check(g, m, cell=1000.0)                                            # a grid first: the failure below must take it away
    m.build()
    assert state() == before
    with pytest.raises(P.PpsError) as e:
        m.build_grid(cell=0.01)
    assert e.value.code == P.PPS_ENOMEM
    assert f"plane node {pl[1]}" in str(e.value) and " x " in str(e.value), str(e.value)
    assert m.grid_info() == ZEROS and len(m.grid_planes()) == 0
    with pytest.raises(P.PpsError):
        m.grid_download(0, 1)
    assert state() == before
    want, _ = _check(g, m, cell=1000.0)                                  # the next call with a larger cell succeeds
    assert want["totals"]["n_cells"] >= 3
    boxes = int(want["planes"]["ni"].astype(np.int64) @ want["planes"]["nj"])
    with pytest.raises(P.PpsError) as e:                                 # exactly one cell too few
        m.build_grid(cell=1000.0, max_cells=boxes - 1)
    assert e.value.code == P.PPS_ENOMEM and m.grid_info() == ZEROS
    _check(g, m, cell=1000.0, max_cells=boxes)                           # the limit itself is allowed
    m.close(); g.close()


# ---- reproducibility -----------------------------------------------------------------------------------------------------------------
def test_reproducible_and_leaves_the_build_alone(overlapping):
    g, m, pl = overlapping
    sel = P.map_select(2, every_frame=0, old_age=-100, old_every=2, min_tracked=(0, 0, 0))
    m.build(sel)
    built = (m.info(), m.built_chunks().tobytes(), m.download(1).tobytes(), m.last_times())
    m.build_grid(cell=0.05)
    first = tuple(a.tobytes() for a in m.grid_download()) + (m.grid_planes().tobytes(),)
    assert (m.info(), m.built_chunks().tobytes(), m.download(1).tobytes(), m.last_times()) == built      # the grid of ALL chunks left the build of two frames alone
    m.build_grid(cell=0.05)
    assert tuple(a.tobytes() for a in m.grid_download()) + (m.grid_planes().tobytes(),) == first
    m.build()                                                            # a build between two grids changes nothing
    m.build_grid(cell=0.05)
    assert tuple(a.tobytes() for a in m.grid_download()) + (m.grid_planes().tobytes(),) == first
    old = g.get_plane(pl[1])
    new = old + np.array([0.05, 0.02, 0.03, 0.1])
    g.set_plane(pl[1], new)
    try:
        assert np.abs(g.get_plane(pl[1]) - old).max() > 0.01
        want, _ = _check(g, m, cell=0.05)                                # the moved landmark: the statement again, at the new estimate
        assert (m.grid_planes().tobytes() != first[-1]) and want["totals"]["n_cells"] > 0
    finally:
        g.set_plane(pl[1], old)


# ---- a real frame, and a large one ---------------------------------------------------------------------------------------------------
def test_popup_frame(built):
    w, h = 160, 120
    pp, K = _popup(w, h)
    spec = synth.small_world(12, 6, seed=3)
    g = P.Graph(); spec.replay(g); g.batch_optimize()
    pl = [i for i, t in enumerate(spec.node_type) if t == synth.NODE_PLANE]
    m = P.Map(g, w * h)
    seg, polys, T = synth.corridor_frame(_pose(0), width=w, height=h, K=K)
    assert pp.run(seg, T, polys, step=2, depth_thre=10.0, ceiling_thre=2.5) > 0
    counts = m.add_frame(pp, 0, pl[:4])
    assert np.all(counts > 0)
    want, _ = _check(g, m, cell=0.05)
    assert want["totals"]["n_planes"] == 4 and want["totals"]["n_cells"] > 100
    m.close(); g.close()


def test_300000_points(built):
    """four flat frames of 320 x 240 over six landmarks at cell = 0.02: the emission scan spans many tiles, the grids many rows"""
    planes = [GROUND, WALL, [1, 0, 0, -2], [0, 2, 0, 1], [0.1, 0.2, -0.9, 0.5], [0.3, 0.5, 0.81, 1.0]]
    g, pl = _graph(planes)
    rng = np.random.default_rng(320)
    m = P.Map(g, 4 * 320 * 240)
    for f in range(4):
        cloud, pid = scan_frame(rng, planes, 320, 240, (-3.0 + 0.4 * f, -2.0 + 0.3 * f), 0.011)
        m.debug_add_points(cloud, pid, f, pl)
    assert m.info()["n_points"] > 250000
    want, _ = _check(g, m, cell=0.02)
    assert int(want["planes"]["ni"].astype(np.int64) @ want["planes"]["nj"]) > 20 * 2048 and np.all(want["planes"]["nj"] > 10)
    assert want["totals"]["n_cells"] > 30000 and want["counts"].max() >= 4
    m.close(); g.close()
