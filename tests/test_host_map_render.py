"""CPU: the rendered view (include/pps.h: pps_map_render and the pps_map_render_* calls) before any kernel runs on a device.

  * every refusal is answered on the host (this suite runs without a device) and leaves the map usable;
  * the two new structs have the layout the ctypes mirrors assume (a C program compiled against the header prints sizes and offsets);
  * pps_map_render_ray_host / pps_map_render_hit_host against the numpy statement (render_helpers), exactly, on random pixels and planes
    and on the edges of every rule of the statement;
  * the kernels of csrc/pps_render.hip themselves, compiled for the host (tests/cpp/render_emu.cpp: one std::thread per GPU thread),
    against the numpy statement of the whole view, exactly."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pop_up_slam_amd as P
from grid_helpers import LIMIT
from render_helpers import assert_view_equal, frame_exact, look_at, pinhole_invK, pose, ref_hit, ref_rays, ref_render, ring_order, rot_xyz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENT = np.eye(4, dtype=np.float32)
IK = pinhole_invK(8, 6)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def _render_rc(m, **kw):
    a = dict(width=8, height=6, invK=IK, T_wc=IDENT, reach=1, z_near=0.0, z_far=float("inf"))
    reserved = kw.pop("reserved", 0)
    a.update(kw)
    v = P.map_view(**a); v.reserved = reserved
    return P.lib().pps_map_render(m.h, C.byref(v), None)


def test_every_refusal_is_answered_without_a_device(built):
    L = P.lib()
    g = P.Graph()
    g.add_pose([0, 0, 1, 0, 0, 0, 1]); g.add_plane([0, 0, 1, 0])
    m = P.Map(g, 1000)
    v = P.map_view(8, 6, IK, IDENT)
    assert (v.width, v.height, v.reach, v.reserved, v.z_near, v.z_far) == (8, 6, 1, 0, 0.0, float("inf"))
    assert list(v.invK) == IK.reshape(9).tolist() and list(v.T_wc) == IDENT.reshape(16).tolist()
    tot = P.PpsMapRenderTotals(); n = C.c_int()
    assert L.pps_map_render(None, C.byref(v), None) == P.PPS_EINVAL
    assert L.pps_map_render(m.h, None, None) == P.PPS_EINVAL
    assert L.pps_map_render_download(None, None, None, None, None) == P.PPS_EINVAL
    assert L.pps_map_render_info(None, C.byref(tot)) == P.PPS_EINVAL and L.pps_map_render_info(m.h, None) == P.PPS_EINVAL
    assert L.pps_map_grid_plane_eq(None, 0, None, C.byref(n)) == P.PPS_EINVAL and L.pps_map_grid_plane_eq(m.h, 0, None, None) == P.PPS_EINVAL
    assert L.pps_map_grid_plane_eq(m.h, 1, None, C.byref(n)) == P.PPS_EINVAL
    state = lambda: (m.info(), m.chunks().tobytes(), m.built_chunks().tobytes(), m.grid_info(), m.grid_planes().tobytes())

    def no_view():
        assert L.pps_map_render_download(m.h, None, None, None, None) == P.PPS_ESTATE
        assert L.pps_map_render_info(m.h, C.byref(tot)) == P.PPS_ESTATE

    bad_T = []
    for k, val in ((0, np.nan), (3, np.inf), (12, 1.0), (15, 2.0), (0, 1.01), (1, 0.5)):
        T = IDENT.copy().reshape(16); T[k] = val; bad_T.append(T)
    bad_K = []
    for k, val in ((0, np.nan), (8, np.inf), (4, -np.inf)):
        K = IK.copy().reshape(9); K[k] = val; bad_K.append(K)
    einval = ([dict(width=w) for w in (0, -1, 4097)] + [dict(height=h) for h in (0, -3, 4097)] + [dict(reach=r) for r in (-1, 5)] +
              [dict(reserved=1), dict(reserved=-1)] + [dict(invK=K) for K in bad_K] + [dict(T_wc=T) for T in bad_T] +
              [dict(z_near=z) for z in (-0.1, np.nan, np.inf)] + [dict(z_far=np.nan), dict(z_near=1.0, z_far=1.0), dict(z_near=2.0, z_far=1.0), dict(z_far=0.0)])

    # no grid yet: the arguments are judged first, then the state
    before = state()
    for kw in einval:
        assert _render_rc(m, **kw) == P.PPS_EINVAL, kw
        assert m.L.pps_map_last_error(m.h) != b""
    assert _render_rc(m) == P.PPS_ESTATE
    no_view()
    assert len(m.grid_plane_eq()) == 0 and state() == before
    # a grid without cells (an empty map builds one without a device) renders every pixel empty, without a device
    assert m.build_grid(cell=0.05) == (0, 0)
    before = state()
    no_view()
    out = m.render(8, 6, IK, IDENT)
    assert out["n_hit"] == 0 and out["totals"] == dict(width=8, height=6, n_planes=0, launches=0, n_hit=0, sec=0.0)
    assert out["cloud"].shape == out["depth"].shape == out["plane_id"].shape == out["cell"].shape == (6, 8)
    assert not out["cloud"].view(np.uint8).any() and not out["depth"].any() and np.all(out["plane_id"] == -1) and np.all(out["cell"] == -1)
    assert L.pps_map_render_download(m.h, None, None, None, None) == P.PPS_OK
    only = np.zeros(48, dtype=np.int32)
    assert L.pps_map_render_download(m.h, None, None, only.ctypes.data_as(C.c_void_p), None) == P.PPS_OK and np.all(only == -1)
    for kw in einval:                                                     # a refusal changes nothing: the view stays
        assert _render_rc(m, **kw) == P.PPS_EINVAL, kw
    assert m.render_info()["width"] == 8 and state() == before
    assert m.render(1, 1, IK, IDENT, reach=0, z_near=0.5, z_far=0.75)["totals"]["width"] == 1
    assert m.render(4096, 1, IK, IDENT, reach=4)["cell"].shape == (1, 4096)
    # a grid call ends the view, whether it succeeds ...
    assert m.build_grid(cell=0.05) == (0, 0)
    no_view()
    m.render(8, 6, IK, IDENT)
    # ... or fails; after a failed one there is no grid to render either
    with pytest.raises(P.PpsError):
        m.build_grid(cell=0.0)
    no_view()
    assert _render_rc(m) == P.PPS_ESTATE
    with pytest.raises(P.PpsError) as e:
        m.render(8, 6, IK, IDENT)
    assert e.value.code == P.PPS_ESTATE and "grid" in str(e.value)
    # the map stays usable
    assert m.build_grid(posed=True) == (0, 0) and m.render(3, 2, IK, IDENT)["n_hit"] == 0
    assert m.build() == (0, 0)
    m.close(); g.close()


def test_host_calls_check_their_pointers(built):
    L = P.lib()
    v = P.map_view(8, 6, IK, IDENT)
    d3 = (C.c_double * 3)(); d4 = (C.c_double * 4)(0, 0, 1, -2); z = C.c_double(); f3 = (C.c_float * 3)(); ij = (C.c_int64 * 2)()
    assert L.pps_map_render_ray_host(None, 0, 0, d3, d3, d3) == P.PPS_EINVAL
    assert L.pps_map_render_ray_host(C.byref(v), 0, 0, None, d3, d3) == P.PPS_EINVAL
    assert L.pps_map_render_hit_host(None, d3, d3, d4, 1.0, 0.0, 1.0, C.byref(z), f3, ij) == -1
    assert L.pps_map_render_hit_host(d3, d3, d3, d4, 1.0, 0.0, 1.0, None, f3, ij) == -1
    for bad in ([0, 0, 0, 1], [np.nan, 0, 1, 0]):
        with pytest.raises(P.PpsError):
            P.map_render_hit_host([0, 0, 0], [0, 0, 1], [0, 0, 1], bad, 1.0)
    L.pps_map_default_view(None, 1, 1, None, None)                       # a NULL view is ignored


# ---- layouts -------------------------------------------------------------------------------------------------------------------------
LAYOUT_C = r'''
#include <stddef.h>
#include <stdio.h>
#include "pps.h"
#define S(t) printf(#t " size %zu\n", sizeof(t))
#define O(t, f) printf(#t " " #f " %zu\n", offsetof(t, f))
int main(void) {
  S(pps_map_view); O(pps_map_view, width); O(pps_map_view, height); O(pps_map_view, reach); O(pps_map_view, reserved); O(pps_map_view, invK);
  O(pps_map_view, T_wc); O(pps_map_view, z_near); O(pps_map_view, z_far);
  S(pps_map_render_totals); O(pps_map_render_totals, width); O(pps_map_render_totals, height); O(pps_map_render_totals, n_planes);
  O(pps_map_render_totals, launches); O(pps_map_render_totals, n_hit); O(pps_map_render_totals, sec);
  return 0;
}
'''


def test_struct_layouts_match_the_ctypes_mirrors(built, tmp_path):
    src = tmp_path / "layout.c"; exe = tmp_path / "layout"
    src.write_text(LAYOUT_C)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    mirrors = {"pps_map_view": P.PpsMapView, "pps_map_render_totals": P.PpsMapRenderTotals}
    seen = 0
    for line in subprocess.check_output([str(exe)], text=True).split("\n"):
        w = line.split()
        if not w:
            continue
        T = mirrors[w[0]]
        if w[1] == "size":
            assert C.sizeof(T) == int(w[2]), line
        else:
            assert getattr(T, w[1]).offset == int(w[2]), line
        seen += 1
    assert seen == 2 + 8 + 6
    assert P.lib().pps_version() == P.PPS_VERSION == 305                 # found by symbol lookup: the version did not move


# ---- one pixel against one landmark --------------------------------------------------------------------------------------------------
def _compare_pairs(view, cols, rows, abcd, inv_cell, z_near=0.0, z_far=np.inf):
    """the two host calls against the statement on the pixels (cols, rows) of `view` and one plane; returns the expected hit flags"""
    iK = np.array(list(view.invK), dtype=np.float32); T = np.array(list(view.T_wc), dtype=np.float32)
    o, ds, dw = ref_rays(np.asarray(cols), np.asarray(rows), iK, T)
    ok, z, xf, i, j = ref_hit(o, ds, dw, abcd, inv_cell, z_near, z_far)
    for k in range(len(cols)):
        go, gds, gdw = P.map_render_ray_host(view, int(cols[k]), int(rows[k]))
        np.testing.assert_array_equal(go, o)
        np.testing.assert_array_equal(gds, [ds[0][k], ds[1][k], ds[2][k]]); np.testing.assert_array_equal(gdw, [dw[0][k], dw[1][k], dw[2][k]])
        hit, gz, gx, gij = P.map_render_hit_host(go, gds, gdw, abcd, inv_cell, z_near, z_far)
        assert hit == bool(ok[k]), (k, cols[k], rows[k])
        if hit:
            assert gz == z[k] and gij == (int(i[k]), int(j[k]))
            np.testing.assert_array_equal(gx.view(np.uint32), np.array([xf[0][k], xf[1][k], xf[2][k]], dtype=np.float32).view(np.uint32))
        else:
            assert gz == 0.0 and not gx.any() and gij == (0, 0)
    return ok


def test_ray_and_hit_host_are_the_numpy_statement(built):
    """40 random planes x 260 random pixels of a randomly posed camera each: 10 400 pairs"""
    rng = np.random.default_rng(81)
    n_pairs = n_hit = n_behind = 0
    for _ in range(40):
        w, h = 640, 480
        T = pose(rot_xyz(*rng.uniform(-np.pi, np.pi, size=3)), rng.normal(size=3) * 2.0)
        view = P.map_view(w, h, pinhole_invK(w, h, rng.uniform(200, 900)), T, z_near=0.1, z_far=rng.choice([8.0, np.inf]))
        nrm = rng.normal(size=3)
        abcd = np.concatenate([nrm * rng.uniform(0.2, 5.0) / np.linalg.norm(nrm), [rng.normal() * 3.0]])
        cols, rows = rng.integers(0, w, size=260), rng.integers(0, h, size=260)
        cell = rng.choice([0.02, 0.05, 1.0 / 3.0])
        ok = _compare_pairs(view, cols, rows, abcd, 1.0 / cell, view.z_near, view.z_far)
        n_pairs += len(ok); n_hit += int(ok.sum()); n_behind += int((~ok).sum())
    assert n_pairs >= 10000 and n_hit > 1500 and n_behind > 1500


def test_hit_host_on_the_edges_of_the_statement(built):
    # den exactly 0: exact binary fractions everywhere.  The camera looks along world x, the pixels of row 2 have ds[1] = 0, so their
    # rays lie in the world plane z = 0.5 and are parallel to the ground z = 2 (n = (0, 0, 1)): den = 0 exactly, h != 0
    iK = np.array([[0.25, 0, -1.0], [0, 0.25, -0.5], [0, 0, 1]], dtype=np.float32)
    T = np.array([[0, 0, 1, 0.25], [-1, 0, 0, 0.5], [0, -1, 0, 0.5], [0, 0, 0, 1]], dtype=np.float32)
    view = P.map_view(8, 6, iK, T)
    ground = np.array([0.0, 0.0, 2.0, -4.0])
    cols = np.arange(8)
    o, ds, dw = ref_rays(cols, np.full(8, 2), iK, T)
    assert np.all(dw[2] == 0.0) and np.all(ds[1] == 0.0)
    ok = _compare_pairs(view, cols, np.full(8, 2), ground, 4.0)
    assert not ok.any()
    # t <= 0: rows above the axis look up at the ground plane z = 2 (a plane is seen from both sides), rows below look away from it
    up = _compare_pairs(view, cols, np.full(8, 0), ground, 4.0); down = _compare_pairs(view, cols, np.full(8, 5), ground, 4.0)
    assert up.all() and not down.any()
    assert _compare_pairs(view, cols, np.full(8, 0), -ground, 4.0).all()                 # the other description of the plane
    # t = 0 exactly: the camera centre lies on the plane
    assert not _compare_pairs(view, cols, np.full(8, 0), np.array([0.0, 0.0, 1.0, -0.5]), 4.0).any()
    # z on both limits: the wall x = 4.25 is hit by every pixel at z = t * ds[2] = 4 exactly (ds[2] = 1, dw[0] = 1, o[0] = 0.25)
    wall = np.array([1.0, 0.0, 0.0, -4.25])
    allpx = (np.tile(np.arange(8), 6), np.repeat(np.arange(6), 8))
    for z_near, z_far, want in ((0.0, 4.0, True), (4.0, 5.0, True), (4.0, np.inf, True), (0.0, np.nextafter(4.0, 0.0), False),
                                (np.nextafter(4.0, 5.0), 9.0, False)):
        ok = _compare_pairs(view, allpx[0], allpx[1], wall, 4.0, z_near, z_far)
        assert ok.all() == want and ok.any() == want, (z_near, z_far)
    # a dropped axis: |i| >= 2^30.  The wall 2^28 m away at 4 cells per metre puts e1 . X at 2^28 * |x/f| * 4: beyond the limit for the
    # outer columns only, and one coarser cell keeps them all
    far = np.array([1.0, 0.0, 0.0, -(2.0 ** 28)])
    ok = _compare_pairs(view, allpx[0], allpx[1], far, 8.0)
    assert ok.any() and not ok.all()
    o, ds, dw = ref_rays(allpx[0], allpx[1], iK, T)
    _, z, xf, i, j = ref_hit(o, ds, dw, far, 8.0)
    l, n, e1, e2 = frame_exact(far)
    u = np.abs(xf[0].astype(np.float64) * e1[0] + xf[1].astype(np.float64) * e1[1]) * 8.0
    v = np.abs(xf[2].astype(np.float64)) * 8.0
    assert np.array_equal(ok, (u < LIMIT) & (v < LIMIT)) and np.any(u >= LIMIT)
    assert _compare_pairs(view, allpx[0], allpx[1], far, 0.5).all()
    # X not finite in fp32: the wall 2^127.5 m away is hit at a finite fp64 point whose x does not fit a float
    huge = np.array([1.0, 0.0, 0.0, -(2.0 ** 128)])
    ok = _compare_pairs(view, allpx[0], allpx[1], huge, 1e-30)
    assert not ok.any()
    _, z, xf, _, _ = ref_hit(o, ds, dw, huge, 1e-30)
    assert np.all(np.isfinite(z)) and np.all(np.isinf(xf[0]))
    assert _compare_pairs(view, allpx[0], allpx[1], np.array([1.0, 0.0, 0.0, -(2.0 ** 100)]), 2.0 ** -80).all()      # ... and one that fits


# ---- the kernels, compiled for the host ----------------------------------------------------------------------------------------------
class RenderArgs(C.Structure):                                           # RenderArgs (csrc/pps_render.h)
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("reach", C.c_int), ("n_rows", C.c_int), ("iK", C.c_float * 9), ("T", C.c_float * 16),
                ("z_near", C.c_double), ("z_far", C.c_double), ("inv_cell", C.c_double), ("rows", C.c_void_p), ("ids", C.c_void_p),
                ("slot", C.c_void_p), ("pts", C.c_void_p), ("cloud", C.c_void_p), ("depth", C.c_void_p), ("plane_id", C.c_void_p),
                ("cell", C.c_void_p), ("n_hit", C.c_void_p)]


ROW_DEV = np.dtype([("n", "<f8", 3), ("dn", "<f8"), ("e1", "<f8", 3), ("e2", "<f8", 3), ("base", "<i8"), ("i0", "<i4"), ("j0", "<i4"),
                    ("ni", "<i4"), ("nj", "<i4")])                       # RenderPlane (csrc/pps_render_ray.h)
vp = lambda a: a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def emu(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("renderemu")
    so = d / "librender_emu.so"
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-fPIC", "-shared", "-pthread", "-ffp-contract=off",
                           "-I", os.path.join(ROOT, "tests", "cpp", "grid_emu"), "-I", os.path.join(ROOT, "pop_up_slam_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "render_emu.cpp"), "-o", str(so)])
    E = C.CDLL(str(so))
    sizes = (C.c_int * 2)(); E.emu_render_sizes(sizes)
    assert list(sizes) == [C.sizeof(RenderArgs), ROW_DEV.itemsize] and ROW_DEV.itemsize == 104
    E.emu_render_slots.argtypes = [C.c_longlong, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p]
    return E


def made_up_grid(rng, landmarks, min_count=1):
    """landmarks: rows (plane node id, abcd, i0, j0, ni, nj, p_occupied) in ascending id.  Makes up the cell arrays a grid call would have
    left -- cnt[] over the boxes back to back, the tile prefix of the emitted cells -- and what its read calls would return: the plane table,
    the plane equations and the grid map (random colours; the coordinates of a grid point play no part in a view)."""
    planes = np.zeros(len(landmarks), dtype=P.GRID_PLANE_DTYPE); eq = np.zeros((len(landmarks), 4))
    cnts = []
    for r, (node, abcd, i0, j0, ni, nj, p_occ) in enumerate(landmarks):
        c = rng.integers(min_count, min_count + 3, size=ni * nj).astype(np.uint32)
        c[rng.random(ni * nj) >= p_occ] = min_count - 1                  # one point short of an emitted cell (0: an empty one)
        cnts.append(c)
        for k, val in (("plane_id", node), ("i0", i0), ("j0", j0), ("ni", ni), ("nj", nj)):
            planes[r][k] = val
        eq[r] = abcd
    cnt = np.concatenate(cnts) if cnts else np.zeros(0, np.uint32)
    keep = cnt >= min_count
    ij, off = [], 0
    for r, c in enumerate(cnts):
        k = np.flatnonzero(c >= min_count)
        planes[r]["offset"], planes[r]["count"] = off, len(k); off += len(k)
        ij.append(np.stack([k % planes[r]["ni"] + planes[r]["i0"], k // planes[r]["ni"] + planes[r]["j0"]], axis=1))
    ij = np.concatenate(ij).astype(np.int32) if ij else np.zeros((0, 2), np.int32)
    pts = np.zeros(int(keep.sum()), dtype=P.POINT_DTYPE)
    pts["rgba"] = rng.integers(0, 1 << 32, size=len(pts), dtype=np.uint64).astype(np.uint32)
    cpw = 2048                                                           # grid_tiling of fewer than 2^31 cells
    tile_prefix = np.concatenate([[0], np.cumsum([int(keep[a:a + cpw].sum()) for a in range(0, len(cnt), cpw)])]).astype(np.int64)
    return dict(planes=planes, eq=eq, cnt=cnt, tile_prefix=tile_prefix, pts=pts, ij=ij, min_count=min_count)


def emu_view(E, G, width, height, invK, T_wc, inv_cell, reach=1, z_near=0.0, z_far=np.inf):
    """drives the emulated kernels the way pps_map_render.cpp does: the rows with a box, the slot table, the view"""
    n_all = len(G["cnt"])
    guard = 3
    slot = np.full(n_all + guard, -7, dtype=np.int32)
    assert E.emu_render_slots(n_all, G["min_count"], vp(G["cnt"]), vp(G["tile_prefix"]), vp(slot)) == 0
    assert np.all(slot[n_all:] == -7)
    keep = G["cnt"] >= G["min_count"]
    np.testing.assert_array_equal(slot[:n_all], np.where(keep, np.cumsum(keep) - 1, -1))
    used = [r for r, p in enumerate(G["planes"]) if int(p["ni"]) * int(p["nj"]) > 0]
    rows = np.zeros(len(used), dtype=ROW_DEV); ids = np.zeros(len(used), dtype=np.int32)
    base = 0
    for k, r in enumerate(used):
        p = G["planes"][r]
        n, e1, e2 = P.map_grid_frame_host(G["eq"][r])
        rows[k]["n"], rows[k]["e1"], rows[k]["e2"] = n, e1, e2
        rows[k]["dn"] = G["eq"][r][3] / np.sqrt(G["eq"][r][0] ** 2 + G["eq"][r][1] ** 2 + G["eq"][r][2] ** 2)
        rows[k]["base"] = base; base += int(p["ni"]) * int(p["nj"])
        for f in ("i0", "j0", "ni", "nj"):
            rows[k][f] = p[f]
        ids[k] = p["plane_id"]
    assert base == n_all
    npx = width * height
    cloud = np.zeros(npx + guard, dtype=P.POINT_DTYPE); cloud["rgba"] = 0xDEADBEEF
    depth = np.full(npx + guard, -7.0, dtype=np.float32); pid = np.full(npx + guard, -7, dtype=np.int32); cell = np.full(npx + guard, -7, dtype=np.int64)
    n_hit = np.zeros(1, dtype=np.uint64)
    a = RenderArgs(width, height, reach, len(used), (C.c_float * 9)(*np.asarray(invK, np.float32).reshape(9)),
                   (C.c_float * 16)(*np.asarray(T_wc, np.float32).reshape(16)), z_near, z_far, inv_cell, vp(rows).value, vp(ids).value,
                   vp(slot).value, vp(G["pts"]).value, vp(cloud).value, vp(depth).value, vp(pid).value, vp(cell).value, vp(n_hit).value)
    assert E.emu_render(C.byref(a)) == 0
    assert np.all(cloud["rgba"][npx:] == 0xDEADBEEF) and np.all(depth[npx:] == -7.0) and np.all(pid[npx:] == -7) and np.all(cell[npx:] == -7)
    sh = (height, width)
    got = dict(cloud=cloud[:npx].reshape(sh), depth=depth[:npx].reshape(sh), plane_id=pid[:npx].reshape(sh), cell=cell[:npx].reshape(sh), n_hit=int(n_hit[0]))
    want = ref_render(width, height, invK, T_wc, G["planes"], G["eq"], inv_cell, G["pts"], G["ij"], reach, z_near, z_far)
    assert_view_equal(got, want)
    return want


GROUND, WALL, WALL2 = [0.0, 0.0, -1.0, 0.2], [0.6, -0.8, 0.0, 0.7], [1.0, 0.0, 0.0, -3.0]


def test_emulated_view_of_a_ground_and_two_walls(emu):
    """17 x 9: partial tiles on both edges; boxes on both sides of the lattice origins; the walls stand in front of each other and of the
    ground in parts of the image, the sky is empty"""
    rng = np.random.default_rng(91)
    G = made_up_grid(rng, [(3, GROUND, -60, -60, 140, 120, 0.9), (5, WALL, -70, -10, 160, 50, 0.9), (9, WALL2, -40, -5, 80, 45, 0.9)])
    T = look_at([0.3, 0.2, 1.2], [3.0, 0.5, 0.6])
    want = emu_view(emu, G, 17, 9, pinhole_invK(17, 9, 9.0), T, 1.0 / 0.05)
    assert set(np.unique(want["plane_id"]).tolist()) == {-1, 3, 5, 9}
    R = rot_xyz(0.2, -0.3, 0.4) @ np.asarray(T[:3, :3], dtype=np.float64)
    want = emu_view(emu, G, 17, 9, pinhole_invK(17, 9, 9.0), pose(R, [0.3, 0.2, 1.2]), 1.0 / 0.05, z_near=0.5, z_far=4.0)
    assert 0 < want["n_hit"] < 17 * 9
    assert emu_view(emu, G, 1, 1, pinhole_invK(1, 1, 9.0), T, 1.0 / 0.05)["n_hit"] == 1


def test_emulated_view_of_300_landmarks(emu):
    """300 landmarks of one cell each, a few of them without a box: the LDS slice of 256 rows wraps, and the nearest of many parallel
    planes answers"""
    rng = np.random.default_rng(92)
    lms = []
    for k in range(300):
        abcd = np.array([1.0, 0.0, 0.0, -(2.0 + 0.01 * ((k * 37) % 300))])        # walls x = 2 .. 5, in no order of depth
        l, n, e1, e2 = frame_exact(abcd)
        y, z = rng.uniform(-1.5, 1.5), rng.uniform(-1.0, 1.0)
        x = -abcd[3]
        i, j = int(np.floor((y * e1[1]) * 2.0)), int(np.floor((z * e2[2]) * 2.0))
        box = (i, j, 1, 1) if k % 41 else (0, 0, 0, 0)                   # every 41st landmark has no box: skipped
        lms.append((100 + 2 * k, abcd, *box, 1.0))
        assert x > 0
    G = made_up_grid(rng, lms)
    T = look_at([0.0, 0.0, 0.0], [1.0, 0.0, 0.0])
    want = emu_view(emu, G, 20, 18, pinhole_invK(20, 18, 6.0), T, 2.0, reach=0)
    ids = np.unique(want["plane_id"][want["plane_id"] >= 0])
    assert len(ids) > 20 and ids.min() < 100 + 2 * 256 < ids.max()       # landmarks of both slices were seen
    emu_view(emu, G, 20, 18, pinhole_invK(20, 18, 6.0), T, 2.0, reach=2)


@pytest.mark.parametrize("reach", [0, 1, 2, 3, 4])
def test_emulated_ring_order(emu, reach):
    """a wall facing the camera whose lattice misses four cells in five: which neighbour answers pins the ring order"""
    rng = np.random.default_rng(93)
    G = made_up_grid(rng, [(7, [1.0, 0.0, 0.0, -2.0], -30, -30, 60, 60, 0.2)], min_count=2)
    T = look_at([0.0, 0.1, -0.05], [1.0, 0.1, -0.05])
    want = emu_view(emu, G, 24, 16, pinhole_invK(24, 16, 14.0), T, 1.0 / 0.08, reach=reach)
    # which offset answered, from the expected view alone: every offset of every ring up to `reach` is seen
    hit = want["plane_id"] >= 0
    l, n, e1, e2 = frame_exact(G["eq"][0])
    xf = [want["cloud"][k][hit].astype(np.float64) for k in "xyz"]
    own = np.stack([np.floor(((xf[0] * e[0] + xf[1] * e[1]) + xf[2] * e[2]) * (1.0 / 0.08)) for e in (e1, e2)], axis=1).astype(np.int64)
    seen = {(int(a), int(b)) for a, b in G["ij"][want["cell"][hit]] - own}
    assert seen <= set(ring_order(reach)) and len(seen) >= min(len(ring_order(reach)), 1 + 8 * min(reach, 2)), seen
    assert hit.sum() < hit.size or reach >= 3                            # with a short reach some pixels stay empty
