"""CPU: the grid map (include/pps.h: pps_map_build_grid and the pps_map_grid_* calls) before any kernel runs on a device.

  * every refusal is answered on the host (this suite runs without a device) and leaves the map as it was;
  * the three new structs have the layout the ctypes mirrors assume (a C program compiled against the header prints sizes and offsets);
  * pps_map_grid_frame_host against an fp64 restatement (4 ulp: the same formulas, numpy's cross product orders two subtractions
    differently) and pps_map_grid_cell_host against the numpy statement of the cell arithmetic, exactly;
  * the kernels of csrc/pps_grid.hip themselves, compiled for the host (tests/cpp/grid_emu.cpp: one std::thread per GPU thread, barriers at
    the wave operations, the passes driven from here the way pps_map_grid.cpp drives them), against the numpy statement of the whole grid
    (grid_helpers.ref_grid), exactly."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pop_up_slam_amd as P
from grid_helpers import LIMIT, NEWEST, OLDEST, PLANE_DTYPE, cell_index, frame_fp64, points, ref_grid, scan_frame
from map_helpers import raw16, split_flat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ulps(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return np.max(np.abs(a - b) / np.maximum(np.spacing(np.maximum(np.abs(a), np.abs(b))), np.finfo(np.float64).tiny))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_is_answered_without_a_device(built):
    L = P.lib()
    g = P.Graph()
    g.add_pose([0, 0, 1, 0, 0, 0, 1]); a = g.add_plane([0, 0, 1, 0])
    prm = P.PpsMapGridParams(); L.pps_map_grid_default_params(C.byref(prm))
    assert (prm.cell, prm.rule, prm.min_count, prm.max_cells) == (0.02, P.GRID_NEWEST, 1, 1 << 26)
    n = C.c_int(); tot = P.PpsMapGridTotals()
    assert L.pps_map_build_grid(None, None, C.byref(prm), None, None) == P.PPS_EINVAL
    assert L.pps_map_grid_planes(None, 0, None, C.byref(n)) == P.PPS_EINVAL
    assert L.pps_map_grid_info(None, C.byref(tot)) == P.PPS_EINVAL
    assert L.pps_map_grid_download(None, 0, 0, None, None, None, None) == P.PPS_EINVAL
    m = P.Map(g, 1000)
    zeros = dict(n_points=0, n_cells=0, n_in=0, n_dropped=0, n_passed_through=0, n_planes=0, launches=0, cell=0.0, inv_cell=0.0, sec=(0.0,) * 4)
    before = (m.info(), m.chunks().tobytes(), m.built_chunks().tobytes())
    assert m.grid_info() == zeros                                        # no grid yet

    def refused(fn):
        with pytest.raises(P.PpsError) as e:
            fn()
        assert e.value.code == P.PPS_EINVAL, e.value
        assert str(e.value) != ""
        assert (m.info(), m.chunks().tobytes(), m.built_chunks().tobytes()) == before
        assert m.grid_info() == zeros and len(m.grid_planes()) == 0      # a call that fails leaves no grid

    for again in range(2):
        for cell in (0.0, -0.02, float("nan"), float("inf"), -float("inf"), 1e-320):       # 1 / 1e-320 is not finite
            refused(lambda: m.build_grid(cell=cell))
        refused(lambda: m.build_grid(rule=2))
        refused(lambda: m.build_grid(rule=-1))
        refused(lambda: m.build_grid(min_count=0))
        refused(lambda: m.build_grid(max_cells=0))
        refused(lambda: m.build_grid(max_cells=-5))
        refused(lambda: m.build_grid(P.map_select(3, old_every=0)))
        refused(lambda: m.build_grid(P.map_select(3, new_every=-2)))
        refused(lambda: m.grid_download(0, 1))                           # ranges outside the (empty) grid
        refused(lambda: m.grid_download(1, 0))
        refused(lambda: m.grid_download(-1, 0))
        refused(lambda: m.grid_download(0, -1))
        # an empty map builds to an empty grid, without a device; prm == NULL means the defaults
        assert m.build_grid(cell=0.05, rule=P.GRID_OLDEST, min_count=2) == (0, 0)
        info = m.grid_info()
        assert info == dict(zeros, cell=0.05, inv_cell=1.0 / 0.05)
        npt = C.c_int64(-1); npl = C.c_int(-1)
        assert L.pps_map_build_grid(m.h, None, None, C.byref(npt), C.byref(npl)) == P.PPS_OK and (npt.value, npl.value) == (0, 0)
        assert m.grid_info() == dict(zeros, cell=0.02, inv_cell=1.0 / 0.02)
        assert L.pps_map_build_grid(m.h, None, None, None, None) == P.PPS_OK          # the outputs may be NULL
        pts, cnt, ij, src = m.grid_download()
        assert len(pts) == len(cnt) == len(ij) == len(src) == 0 and len(m.grid_planes()) == 0
        refused(lambda: m.build_grid(cell=0.0))                          # ... and a refusal after a grid takes that grid away
    with pytest.raises(P.PpsError):
        m.download(2, 0, 0)
    assert m.last_times() == (0.0, 0.0) and m.build() == (0, 0)
    # frames without planes and empty chunks only: still no device.  An empty chunk of a live landmark is an observation: a row, no cell
    assert len(m.debug_add_points(np.zeros(4, P.POINT_DTYPE), np.zeros(4, np.int32), 0, [])) == 0
    assert m.build_grid() == (0, 0) and m.grid_info()["n_planes"] == 0
    m.close(); g.close()


def test_host_calls_check_their_pointers(built):
    L = P.lib()
    d3 = (C.c_double * 3)(); d4 = (C.c_double * 4)(0, 0, 1, 0); f3 = (C.c_float * 3)(); c = C.c_int64(); dr = C.c_int()
    assert L.pps_map_grid_frame_host(None, d3, d3, d3) == P.PPS_EINVAL
    assert L.pps_map_grid_frame_host(d4, None, d3, d3) == P.PPS_EINVAL
    assert L.pps_map_grid_cell_host(None, 1.0, f3, C.byref(c), C.byref(dr)) == P.PPS_EINVAL
    assert L.pps_map_grid_cell_host(d3, 1.0, f3, None, C.byref(dr)) == P.PPS_EINVAL
    for bad in ([0, 0, 0, 1], [np.nan, 0, 1, 0], [np.inf, 0, 0, 0]):
        with pytest.raises(P.PpsError):
            P.map_grid_frame_host(bad)


# ---- layouts -------------------------------------------------------------------------------------------------------------------------
LAYOUT_C = r'''
#include <stddef.h>
#include <stdio.h>
#include "pps.h"
#define S(t) printf(#t " size %zu\n", sizeof(t))
#define O(t, f) printf(#t " " #f " %zu\n", offsetof(t, f))
int main(void) {
  S(pps_map_grid_params); O(pps_map_grid_params, cell); O(pps_map_grid_params, rule); O(pps_map_grid_params, min_count); O(pps_map_grid_params, max_cells);
  S(pps_map_grid_plane); O(pps_map_grid_plane, plane_id); O(pps_map_grid_plane, n_chunks); O(pps_map_grid_plane, i0); O(pps_map_grid_plane, j0);
  O(pps_map_grid_plane, ni); O(pps_map_grid_plane, nj); O(pps_map_grid_plane, offset); O(pps_map_grid_plane, count); O(pps_map_grid_plane, n_in);
  O(pps_map_grid_plane, n); O(pps_map_grid_plane, e1); O(pps_map_grid_plane, e2);
  S(pps_map_grid_totals); O(pps_map_grid_totals, n_points); O(pps_map_grid_totals, n_cells); O(pps_map_grid_totals, n_in); O(pps_map_grid_totals, n_dropped);
  O(pps_map_grid_totals, n_passed_through); O(pps_map_grid_totals, n_planes); O(pps_map_grid_totals, launches); O(pps_map_grid_totals, cell);
  O(pps_map_grid_totals, inv_cell); O(pps_map_grid_totals, sec);
  printf("rules %d %d\n", (int)PPS_GRID_NEWEST, (int)PPS_GRID_OLDEST);
  return 0;
}
'''


def test_struct_layouts_match_the_ctypes_mirrors(built, tmp_path):
    src = tmp_path / "layout.c"; exe = tmp_path / "layout"
    src.write_text(LAYOUT_C)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).split("\n")
    mirrors = {"pps_map_grid_params": P.PpsMapGridParams, "pps_map_grid_plane": P.PpsMapGridPlane, "pps_map_grid_totals": P.PpsMapGridTotals}
    seen = 0
    for line in lines:
        w = line.split()
        if not w or w[0] == "rules":
            continue
        T = mirrors[w[0]]
        if w[1] == "size":
            assert C.sizeof(T) == int(w[2]), line
        else:
            assert getattr(T, w[1]).offset == int(w[2]), line
        seen += 1
    assert seen == 3 + 4 + 12 + 10
    assert "rules 0 1" in lines and (P.GRID_NEWEST, P.GRID_OLDEST) == (0, 1)
    assert P.GRID_PLANE_DTYPE.itemsize == C.sizeof(P.PpsMapGridPlane) and PLANE_DTYPE == P.GRID_PLANE_DTYPE
    for name in P.GRID_PLANE_DTYPE.names:
        assert P.GRID_PLANE_DTYPE.fields[name][1] == getattr(P.PpsMapGridPlane, name).offset


# ---- the frame -----------------------------------------------------------------------------------------------------------------------
def _frame_cases():
    rng = np.random.default_rng(70)
    cases = [("ground", [0, 0, -1, 0]), ("ground up", [0, 0, 1, -0.3]), ("wall x", [1, 0, 0, -2]), ("wall -x", [-1, 0, 0, 2]),
             ("wall y", [0, 1, 0, 1.5]), ("wall -y", [0, -3, 0, 1.5]), ("wall xy", [0.6, -0.8, 0, 0.7]), ("wall scaled", [30, 40, 0, -7])]
    for nz in (0.69, 0.7, 0.6999999, 0.7000001, 0.71, -0.69, -0.71, 0.2, 0.95):          # tilted planes on both sides of |n_z| = 0.7
        phi = rng.uniform(0, 2 * np.pi); r = np.sqrt(1 - nz * nz)
        cases.append((f"tilt {nz}", [r * np.cos(phi), r * np.sin(phi), nz, rng.normal()]))
        s = rng.uniform(0.1, 50)
        cases.append((f"tilt {nz} x {s:.2f}", [s * r * np.cos(phi), s * r * np.sin(phi), s * nz, s * rng.normal()]))
    return cases


@pytest.mark.parametrize("name,abcd", _frame_cases(), ids=[c[0] for c in _frame_cases()])
def test_frame_host(built, name, abcd):
    abcd = np.array(abcd, dtype=np.float64)
    n, e1, e2 = P.map_grid_frame_host(abcd)
    M = np.stack([n, e1, e2])
    assert np.max(np.abs(M @ M.T - np.eye(3))) <= 4 * np.finfo(np.float64).eps           # orthonormal to 4 ulp (of 1)
    assert np.linalg.det(M) > 0.99                                       # n, e1, e2 right-handed: e2 = n x e1
    wn, w1, w2 = frame_fp64(abcd)
    for got, want in ((n, wn), (e1, w1), (e2, w2)):
        near_zero = np.abs(want) < 1e-300
        assert np.all(got[near_zero] == 0.0) and (not np.any(~near_zero) or _ulps(got[~near_zero], want[~near_zero]) <= 4), (got, want)
    if name.startswith("wall"):
        assert e1[2] == 0.0 and n[2] == 0.0                              # a wall's first axis is horizontal, exactly
    if name.startswith("ground"):
        assert abs(n[2]) == 1.0 and e1[0] == 0.0
    # un-normalised input: the same frame as the normalised plane's to rounding, and its n has unit length
    assert abs(np.linalg.norm(n) - 1.0) <= 2 * np.finfo(np.float64).eps
    if abs(abs(n[2]) - 0.7) > 1e-12:                                     # (at the threshold itself a rounding of n_z picks the other axis)
        sn, s1, s2 = P.map_grid_frame_host(abcd / np.linalg.norm(abcd[:3]))
        assert np.max(np.abs(np.stack([sn, s1, s2]) - M)) <= 8 * np.finfo(np.float64).eps
    # the other description of the same plane: n and e1 flip, e2 stays
    fn, f1, f2 = P.map_grid_frame_host(-abcd)
    np.testing.assert_array_equal(fn, -n); np.testing.assert_array_equal(f1, -e1); np.testing.assert_array_equal(f2, e2)


# ---- the cell of a point -------------------------------------------------------------------------------------------------------------
def _cells_host(e, inv_cell, pts):
    got = [P.map_grid_cell_host(e, inv_cell, [p["x"], p["y"], p["z"]]) for p in pts]
    return np.array([c for c, _ in got], dtype=np.int64), np.array([not d for _, d in got])


def test_cell_host_is_the_numpy_statement(built):
    rng = np.random.default_rng(71)
    n_neg = n_edge = 0
    for abcd in ([0, 0, -1, 0], [0.6, -0.8, 0, 0.7], [0.3, 0.5, 0.81, 1.0]):
        _, e1, e2 = P.map_grid_frame_host(abcd)
        for cell in (0.02, 0.05, 0.5, 1.0 / 3.0):
            inv = 1.0 / cell
            pts = points(rng.normal(size=(300, 3)) * 4)                  # random fp32 points, both signs
            for e in (e1, e2):
                got, ok = _cells_host(e, inv, pts)
                want, wok = cell_index(pts, e, inv)
                np.testing.assert_array_equal(got, want); np.testing.assert_array_equal(ok, wok)
                n_neg += int(np.count_nonzero(want < 0))
    assert n_neg > 500                                                   # floor, not truncation: negative coordinates were there
    assert P.map_grid_cell_host([1, 0, 0], 50.0, [-0.01, 0, 0]) == (-1, False)
    # u a few ulp on either side of a multiple of the cell, along a coordinate axis (u is then the fp32 coordinate itself)
    for cell in (0.02, 0.05, 0.5):
        inv = 1.0 / cell
        for k in (-37, -1, 0, 1, 2, 1000, 12345):
            x = np.float32(k * cell)
            xs = [x]
            for _ in range(3):
                xs.append(np.nextafter(xs[-1], np.float32(np.inf)))
            lo = x
            for _ in range(3):
                lo = np.nextafter(lo, np.float32(-np.inf)); xs.append(lo)
            pts = points(np.stack([np.array(xs, dtype=np.float64), np.zeros(7), np.zeros(7)], axis=1))
            got, ok = _cells_host([1.0, 0.0, 0.0], inv, pts)
            want, wok = cell_index(pts, np.array([1.0, 0.0, 0.0]), inv)
            np.testing.assert_array_equal(got, want)
            assert ok.all() and wok.all()
            n_edge += len(set(want.tolist())) > 1
    assert n_edge >= 10                                                  # the seven neighbours of a boundary fall on both sides of it


def test_cell_host_reports_dropped_points(built):
    e = np.array([0.6, 0.8, 0.0])
    for bad in (np.nan, np.inf, -np.inf, 1e30, -1e30):
        for k in range(2):
            xyz = [1.0, 2.0, 3.0]; xyz[k] = bad
            assert P.map_grid_cell_host(e, 50.0, xyz) == (0, True), (bad, k)
            pts = points([xyz]); pts["x"][0], pts["y"][0] = np.float32(xyz[0]), np.float32(xyz[1])
            assert not cell_index(pts, e, 50.0)[1][0]
    assert P.map_grid_cell_host(e, 50.0, [1.0, 2.0, 3.0]) == (int(np.floor((1.0 * 0.6 + 2.0 * 0.8) * 50.0)), False)
    # the limit: |i| >= 2^30 drops the point, 2^30 - 64 (the fp32 below 2^30) is the last kept index at inv_cell = 1
    x = [1.0, 0.0, 0.0]
    assert LIMIT == 2.0 ** 30
    assert P.map_grid_cell_host(x, 1.0, [2.0 ** 30, 0, 0]) == (0, True) and P.map_grid_cell_host(x, 1.0, [-2.0 ** 30, 0, 0]) == (0, True)
    assert P.map_grid_cell_host(x, 1.0, [2.0 ** 30 - 64, 0, 0]) == (2 ** 30 - 64, False)
    assert P.map_grid_cell_host(x, 1.0, [-2.0 ** 30 + 64, 0, 0]) == (-2 ** 30 + 64, False)
    assert P.map_grid_cell_host(x, 1e300, [1e10, 0, 0]) == (0, True)                     # u finite, u * inv_cell not
    for xyz, inv in (([2.0 ** 30, 0, 0], 1.0), ([-2.0 ** 30, 0, 0], 1.0), ([2.0 ** 30 - 64, 0, 0], 1.0), ([1e10, 0, 0], 1e300)):
        c, d = P.map_grid_cell_host(x, inv, xyz)
        wc, wok = cell_index(points([xyz]), np.array(x), inv)
        assert (c, d) == (int(wc[0]), not wok[0])


# ---- the kernels, compiled for the host ----------------------------------------------------------------------------------------------
class SelArgs(C.Structure):                                              # GridSelArgs (csrc/pps_grid.h)
    _fields_ = [("n_out", C.c_longlong), ("n_sel", C.c_int), ("out_off", C.c_void_p), ("src_off", C.c_void_p), ("slot", C.c_void_p),
                ("lm", C.c_void_p), ("plane_est", C.c_void_p), ("plane_ld", C.c_int), ("store", C.c_void_p), ("planes", C.c_void_p),
                ("n_planes", C.c_int), ("inv_cell", C.c_double)]


class EmitArgs(C.Structure):                                             # GridEmitArgs
    _fields_ = [("n_cells_all", C.c_longlong), ("min_count", C.c_uint), ("oldest", C.c_int), ("key", C.c_void_p), ("cnt", C.c_void_p),
                ("tile_count", C.c_void_p), ("tile_prefix", C.c_void_p), ("plane_base", C.c_void_p), ("plane_off", C.c_void_p),
                ("pts", C.c_void_p), ("counts", C.c_void_p), ("ij", C.c_void_p), ("src", C.c_void_p)]


PLANE_DEV = np.dtype([("e1", "<f8", 3), ("e2", "<f8", 3), ("base", "<i8"), ("i0", "<i4"), ("j0", "<i4"), ("ni", "<i4"), ("nj", "<i4")])
EXTENT = np.dtype([("imin", "<i4"), ("imax", "<i4"), ("jmin", "<i4"), ("jmax", "<i4"), ("n_in", "<u8")])
I32_MAX, I32_MIN = np.iinfo(np.int32).max, np.iinfo(np.int32).min


@pytest.fixture(scope="module")
def emu(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("gridemu")
    libs = []
    for name in ("grid_emu", "map_emu"):
        so = d / f"lib{name}.so"
        subprocess.check_call(["g++", "-std=c++20", "-O1", "-fPIC", "-shared", "-pthread", "-ffp-contract=off",
                               "-I", os.path.join(ROOT, "tests", "cpp", name), "-I", os.path.join(ROOT, "pop_up_slam_amd", "csrc"),
                               os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", str(so)])
        libs.append(C.CDLL(str(so)))
    E, M = libs
    sizes = (C.c_int * 4)(); E.emu_grid_sizes(sizes)
    assert list(sizes) == [C.sizeof(SelArgs), C.sizeof(EmitArgs), PLANE_DEV.itemsize, EXTENT.itemsize]
    E.emu_grid_cpw.restype = C.c_longlong; E.emu_grid_cpw.argtypes = [C.c_longlong]; E.emu_grid_tiles.argtypes = [C.c_longlong]
    return E, M


vp = lambda a: a.ctypes.data_as(C.c_void_p)


def emu_grid(emu, store, chunks, plane_of_slot, cell, rule, min_count, combine, ld=9):
    """chunks: rows (plane node id, slot or -1, first point in the store, count > 0).  Builds B with the emulated k_map_build, runs the
    emulated grid passes the way pps_map_grid.cpp drives them, and returns (B, chunk table of B, live ids, what the grid calls would
    return as a dict like ref_grid's)."""
    E, M = emu
    ns = len(chunks)
    counts = np.array([c[3] for c in chunks], dtype=np.int64)
    out_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64); n_out = int(out_off[-1])
    src_off = np.array([c[2] for c in chunks], dtype=np.int64)
    slot = np.array([c[1] for c in chunks], dtype=np.int32)
    live_ids = sorted({c[0] for c in chunks if c[1] >= 0})
    lm = np.array([live_ids.index(c[0]) if c[1] >= 0 else -1 for c in chunks], dtype=np.int32)
    n_slots = len(plane_of_slot)
    est = np.full((4, ld), np.nan); est[:, :n_slots] = np.array(plane_of_slot).T
    guard = 5
    B = np.zeros(n_out + guard, dtype=P.POINT_DTYPE); B["rgba"] = 0xDEADBEEF
    assert M.emu_map_build(C.c_longlong(n_out), ns, vp(out_off), vp(src_off), vp(slot), vp(est), ld, vp(store), vp(B)) == 0
    assert np.all(B["rgba"][n_out:] == 0xDEADBEEF)
    B = B[:n_out]
    table = np.zeros(ns, dtype=P.CHUNK_DTYPE)
    table["plane_id"] = [c[0] for c in chunks]; table["count"] = counts; table["offset"] = out_off[:-1]
    # the frames, from the doubles the kernels project with
    nL = len(live_ids)
    planes = np.zeros(nL, dtype=PLANE_DTYPE); dev = np.zeros(nL, dtype=PLANE_DEV)
    for r, node in enumerate(live_ids):
        sl = next(c[1] for c in chunks if c[0] == node and c[1] >= 0)
        planes[r]["plane_id"] = node
        planes[r]["n"], planes[r]["e1"], planes[r]["e2"] = P.map_grid_frame_host(plane_of_slot[sl])
        dev[r]["e1"], dev[r]["e2"] = planes[r]["e1"], planes[r]["e2"]
    inv_cell = 1.0 / cell
    a = SelArgs(n_out, ns, vp(out_off).value, vp(src_off).value, vp(slot).value, vp(lm).value, vp(est).value, ld, vp(store).value, vp(dev).value,
                nL, inv_cell)
    ext = np.zeros(nL, dtype=EXTENT); ext["imin"] = ext["jmin"] = I32_MAX; ext["imax"] = ext["jmax"] = I32_MIN
    dropped = np.zeros(1, dtype=np.uint64)
    assert E.emu_grid_extent(C.byref(a), vp(ext), vp(dropped)) == 0
    base = np.zeros(nL + 1, dtype=np.int64)
    for r in range(nL):
        if ext[r]["n_in"] > 0:
            dev[r]["i0"], dev[r]["j0"] = ext[r]["imin"], ext[r]["jmin"]
            dev[r]["ni"], dev[r]["nj"] = ext[r]["imax"] - ext[r]["imin"] + 1, ext[r]["jmax"] - ext[r]["jmin"] + 1
        dev[r]["base"] = base[r]
        base[r + 1] = base[r] + int(dev[r]["ni"]) * int(dev[r]["nj"])
    n_all = int(base[-1])
    key = np.zeros(n_all + guard, dtype=np.uint64); cnt = np.zeros(n_all + guard, dtype=np.uint32)
    assert E.emu_grid_vote(C.byref(a), int(rule == OLDEST), int(combine), vp(key), vp(cnt)) == 0
    assert not key[n_all:].any() and not cnt[n_all:].any()               # nothing behind the boxes
    assert int(cnt.sum()) == int(ext["n_in"].sum())
    nT = E.emu_grid_tiles(n_all) if n_all else 0
    tile_count = np.full(nT + 1, -7, dtype=np.int32); tile_prefix = np.full(nT + 2, -7, dtype=np.int64); plane_off = np.full(nL + 2, -7, dtype=np.int64)
    e = EmitArgs(n_all, min_count, int(rule == OLDEST), vp(key).value, vp(cnt).value, vp(tile_count).value, vp(tile_prefix).value, vp(base).value,
                 vp(plane_off).value, None, None, None, None)
    n_cells = 0
    if n_all:
        assert E.emu_grid_count(C.byref(e), nL) == 0
        assert tile_count[nT] == -7 and tile_prefix[nT + 1] == -7 and plane_off[nL + 1] == -7
        n_cells = int(plane_off[nL])
        assert n_cells == int(np.count_nonzero(cnt >= min_count)) == int(tile_prefix[nT])
    else:
        plane_off[:] = 0
    pts = np.zeros(n_cells + guard, dtype=P.POINT_DTYPE); pts["rgba"] = 0xDEADBEEF
    ocnt = np.zeros(n_cells + guard, dtype=np.uint32); ij = np.full((n_cells + guard, 2), -7, dtype=np.int32); src = np.full(n_cells + guard, -7, dtype=np.int64)
    if n_cells:
        e.pts, e.counts, e.ij, e.src = vp(pts).value, vp(ocnt).value, vp(ij).value, vp(src).value
        assert E.emu_grid_emit(C.byref(a), C.byref(e)) == 0
    assert np.all(pts["rgba"][n_cells:] == 0xDEADBEEF) and not ocnt[n_cells:].any() and np.all(ij[n_cells:] == -7) and np.all(src[n_cells:] == -7)
    for r in range(nL):
        planes[r]["n_chunks"] = sum(1 for c in chunks if c[0] == live_ids[r] and c[1] >= 0)
        planes[r]["n_in"] = ext[r]["n_in"]
        for k in ("i0", "j0", "ni", "nj"):
            planes[r][k] = dev[r][k]
        planes[r]["offset"] = plane_off[r]; planes[r]["count"] = plane_off[r + 1] - plane_off[r]
    through = int(counts[slot < 0].sum())
    totals = dict(n_points=n_out, n_cells=n_cells, n_in=int(ext["n_in"].sum()), n_dropped=int(dropped[0]), n_passed_through=through, n_planes=nL)
    got = dict(planes=planes, pts=pts[:n_cells], counts=ocnt[:n_cells], ij=ij[:n_cells], src=src[:n_cells], totals=totals)
    return B, table, live_ids, got, inv_cell


def assert_grid_equal(got, want, B):
    assert got["totals"] == want["totals"]
    for k in want["planes"].dtype.names:
        np.testing.assert_array_equal(got["planes"][k], want["planes"][k], err_msg=k)
    np.testing.assert_array_equal(got["src"], want["src"])
    np.testing.assert_array_equal(got["counts"], want["counts"])
    np.testing.assert_array_equal(got["ij"], want["ij"])
    np.testing.assert_array_equal(raw16(got["pts"]), raw16(want["pts"]))
    np.testing.assert_array_equal(raw16(got["pts"]), raw16(B[got["src"]]))


GROUND, WALL, TILTED = [0.0, 0.0, -1.0, 0.2], [0.6, -0.8, 0.0, 0.7], [0.3, 0.5, 0.81, 1.0]


def _store_of(frames, node_of_plane, slot_of_node):
    """flat frames [(cloud, pid, n frame planes)] -> (store, chunk rows) the way add_frame lays them out, empty chunks left out"""
    parts, rows, off = [], [], 0
    for cloud, pid, nplanes in frames:
        for k, chunk in enumerate(split_flat(cloud, pid, nplanes)):
            if len(chunk):
                node = node_of_plane[k]
                rows.append((node, slot_of_node.get(node, -1), off, len(chunk)))
                parts.append(chunk); off += len(chunk)
    return np.concatenate(parts), rows


@pytest.mark.parametrize("combine", [1, 0], ids=["runs", "direct"])
@pytest.mark.parametrize("rule", [NEWEST, OLDEST], ids=["newest", "oldest"])
def test_emulated_grid_of_overlapping_frames(emu, rule, combine):
    """a ground and a wall in three overlapping frames of 1 400 pixels on both sides of the frames' origins; the planes the points are
    projected onto are a little off the ones the frames were made with, like an estimate after optimisation"""
    rng = np.random.default_rng(11)
    frames = [scan_frame(rng, [GROUND, WALL], 50, 28, (-0.9 + 0.3 * f, -0.5 + 0.1 * f), 0.031) + (2,) for f in range(3)]
    store, rows = _store_of(frames, [10, 12], {10: 1, 12: 0})
    est = [np.array(WALL) + [0.01, 0.0, 0.02, 0.01], np.array(GROUND) + [0.01, -0.02, 0.0, 0.0]]
    for cell, min_count in ((0.05, 1), (0.5, 1), (0.05, 2), (0.05, 3)):
        B, table, live, got, inv = emu_grid(emu, store, rows, est, cell, rule, min_count, combine)
        want = ref_grid(B, table, live, got["planes"], inv, rule, min_count)
        assert_grid_equal(got, want, B)
        p = want["planes"]
        assert np.all(p["i0"] < 0) and np.all(p["j0"] < 0) and np.all(p["i0"] + p["ni"] > 0)      # cells on both sides of the origin
        if (cell, min_count) == (0.05, 1):
            assert want["counts"].max() >= 3 and want["totals"]["n_cells"] > 1000
            moved = np.flatnonzero(want["counts"] > 1)
            assert np.any(want["src"][moved] != ref_grid(B, table, live, got["planes"], inv, 1 - rule, 1)["src"][moved])    # the rule matters
        if min_count == 3:
            assert 0 < want["totals"]["n_cells"] < ref_grid(B, table, live, got["planes"], inv, rule, 2)["totals"]["n_cells"]


@pytest.mark.parametrize("combine", [1, 0], ids=["runs", "direct"])
def test_emulated_grid_of_one_point_chunks(emu, combine):
    """300 one-point chunks over 7 landmarks, one of them gone (its points pass through), with NaN, inf and 1e30 among the raw points:
    chunk boundaries inside every wave, more landmarks in a wave than the extent pass reduces in turns"""
    rng = np.random.default_rng(12)
    n = 300
    store = points(rng.normal(size=(n, 3)) * 2.0, rng)
    for k, bad in zip((5, 70, 140, 141, 290), (np.nan, np.inf, -np.inf, 1e30, -1e30)):
        store["xyz"[k % 3]][k] = bad
    nodes = rng.integers(0, 7, size=n)
    nodes[[5, 70, 140, 141, 290]] = [0, 1, 2, 4, 3]                      # four bad points on live landmarks, one passes through with the gone one
    slot_of = {0: 3, 1: 0, 2: 5, 3: -1, 4: 1, 5: 2, 6: 4}
    rows = [(20 + int(v), slot_of[int(v)], k, 1) for k, v in enumerate(nodes)]
    est = [TILTED, GROUND, WALL, [1.0, 0.0, 0.0, -2.0], [0.0, 2.0, 0.0, 1.0], [0.1, 0.2, -0.9, 0.5]]
    bad_live = sum(1 for k in (5, 70, 140, 141, 290) if nodes[k] != 3)
    assert bad_live == 4
    for cell, rule in ((0.5, NEWEST), (4.0, OLDEST), (0.04, NEWEST)):
        B, table, live, got, inv = emu_grid(emu, store, rows, est, cell, rule, 1, combine)
        want = ref_grid(B, table, live, got["planes"], inv, rule, 1)
        assert_grid_equal(got, want, B)
        assert want["totals"]["n_dropped"] == bad_live and want["totals"]["n_passed_through"] == int(np.count_nonzero(nodes == 3))
        assert want["totals"]["n_planes"] == 6
        if cell == 4.0:
            assert want["counts"].max() > 5                              # a handful of cells per landmark
        if cell == 0.04:
            assert np.all(want["counts"] == 1)                           # no two points share a cell


def test_emulated_tiling(emu):
    E, _ = emu
    for n in [1, 2047, 2048, 2049, 1 << 26, (1 << 31) - 1, (1 << 31) + 5, 1 << 40] + [int(v) for v in np.random.default_rng(3).integers(1, 1 << 45, size=300)]:
        cpw, nT = E.emu_grid_cpw(n), E.emu_grid_tiles(n)
        assert cpw % 256 == 0 and (nT - 1) * cpw < n <= nT * cpw and nT <= (1 << 20) + 1, n
        assert cpw == 2048 or n > 2048 << 20
