"""CPU: the compared views (include/pps.h: pps_map_compare and the pps_map_compare_* calls) before any kernel runs on a device.

  * the four new structs have the layout the numpy dtypes and the ctypes mirror assume (a strict C99 program compiled against the header);
  * every refusal that needs no device is answered on the host (this suite runs without one) and changes nothing;
  * pps_map_compare_point_host against the numpy statement (compare_helpers.ref_point), exactly, on random points and planes and on the
    edges of every rule of the statement;
  * the numpy statement of the whole comparison (compare_helpers.ref_compare) against a plain Python loop over the pixels;
  * the kernels of csrc/pps_compare.hip themselves, compiled for the host (tests/cpp/compare_emu.cpp: one std::thread per GPU thread,
    real atomics), on made-up images and plane tables at the shapes the device test uses, against ref_compare, exactly."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import pop_up_slam_amd as P
from compare_helpers import (Q_MAX, assert_compare_equal, check_ties, made_up_view, mixed_frame, plane_table, ref_compare, ref_point, shifted,
                             ties_frame)
from render_helpers import frame_exact, pinhole_invK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENT = np.eye(4, dtype=np.float32)
IK = pinhole_invK(8, 6)
GROUND, WALL, TILTED = [0.0, 0.0, -1.0, 0.2], [0.6, -0.8, 0.0, 0.7], [0.3, 0.5, 0.81, 1.0]

# ---- layouts -------------------------------------------------------------------------------------------------------------------------
FIELDS = {"pps_map_compare_plane": ["n_valid", "n_new", "best_row", "best_plane_id", "best_n", "best_agree"],
          "pps_map_compare_row": ["n_view", "n_unseen"],
          "pps_map_compare_pair": ["frame_plane", "row", "plane_id", "reserved", "n", "n_agree", "sum_q", "sum_q2"],
          "pps_map_compare_totals": ["width", "height", "nplanes", "n_rows", "n_both", "n_frame_only", "n_view_only", "n_neither", "n_bad_id",
                                     "n_pairs", "launches", "reserved", "tol", "sec"]}
LAYOUT_C = ("#include <stddef.h>\n#include <stdio.h>\n#include \"pps.h\"\nint main(void) {\n" +
            "".join(f'  printf("{t} size %lu\\n", (unsigned long)sizeof({t}));\n' +
                    "".join(f'  printf("{t} {f} %lu\\n", (unsigned long)offsetof({t}, {f}));\n' for f in fs) for t, fs in FIELDS.items()) +
            "  return 0;\n}\n")


def test_struct_layouts_match_the_mirrors(built, tmp_path):
    src = tmp_path / "layout.c"; exe = tmp_path / "layout"
    src.write_text(LAYOUT_C)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    dtypes = {"pps_map_compare_plane": P.MAP_COMPARE_PLANE_DTYPE, "pps_map_compare_row": P.MAP_COMPARE_ROW_DTYPE,
              "pps_map_compare_pair": P.MAP_COMPARE_PAIR_DTYPE}
    seen = 0
    for line in subprocess.check_output([str(exe)], text=True).split("\n"):
        w = line.split()
        if not w:
            continue
        if w[0] in dtypes:
            d = dtypes[w[0]]
            assert (d.itemsize if w[1] == "size" else d.fields[w[1]][1]) == int(w[2]), line
        else:
            T = P.PpsMapCompareTotals
            assert (C.sizeof(T) if w[1] == "size" else getattr(T, w[1]).offset) == int(w[2]), line
        seen += 1
    assert seen == 4 + sum(len(f) for f in FIELDS.values())
    assert [d.itemsize for d in dtypes.values()] == [40, 16, 48]
    assert P.lib().pps_version() == P.PPS_VERSION == 305                 # found by symbol lookup: the version did not move


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_that_needs_no_device(built):
    L = P.lib()
    g = P.Graph()
    g.add_pose([0, 0, 1, 0, 0, 0, 1]); g.add_plane([0, 0, 1, 0])
    m = P.Map(g, 1000)
    cloud = np.zeros(48, dtype=P.POINT_DTYPE); pid = np.zeros(48, dtype=np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rec = np.zeros(65, dtype=P.MAP_COMPARE_PLANE_DTYPE)
    hook = lambda npx=48, nplanes=1, tol=0.05: L.pps_debug_map_compare_points(m.h, vp(cloud), vp(pid), npx, nplanes, tol, vp(rec))
    tot = P.PpsMapCompareTotals(); n = C.c_int(); fake = C.c_void_p(1)

    def none_present():
        assert L.pps_map_compare_info(m.h, C.byref(tot)) == P.PPS_ESTATE
        assert L.pps_map_compare_rows(m.h, 0, None, C.byref(n)) == P.PPS_ESTATE
        assert L.pps_map_compare_pairs(m.h, 0, 0, None) == P.PPS_ESTATE

    # NULL pointers
    assert L.pps_map_compare(None, fake, 1, 0.05, None) == P.PPS_EINVAL and L.pps_map_compare(m.h, None, 1, 0.05, None) == P.PPS_EINVAL
    assert L.pps_debug_map_compare_points(None, vp(cloud), vp(pid), 48, 1, 0.05, None) == P.PPS_EINVAL
    assert L.pps_debug_map_compare_points(m.h, None, vp(pid), 48, 1, 0.05, None) == P.PPS_EINVAL
    assert L.pps_debug_map_compare_points(m.h, vp(cloud), None, 48, 1, 0.05, None) == P.PPS_EINVAL
    assert L.pps_map_compare_info(None, C.byref(tot)) == P.PPS_EINVAL and L.pps_map_compare_info(m.h, None) == P.PPS_EINVAL
    assert L.pps_map_compare_rows(None, 0, None, C.byref(n)) == P.PPS_EINVAL and L.pps_map_compare_rows(m.h, 0, None, None) == P.PPS_EINVAL
    assert L.pps_map_compare_rows(m.h, 1, None, C.byref(n)) == P.PPS_EINVAL and L.pps_map_compare_rows(m.h, -1, None, C.byref(n)) == P.PPS_EINVAL
    assert L.pps_map_compare_pairs(None, 0, 0, None) == P.PPS_EINVAL
    einval = [dict(nplanes=k) for k in (0, -1, 66, 1 << 30)] + [dict(tol=t) for t in (np.nan, np.inf, -np.inf, -1e-300, -0.05)]
    state = lambda: (m.info(), m.chunks().tobytes(), m.grid_info(), m.grid_planes().tobytes())
    # no render: the arguments are judged first, then the state
    before = state()
    for kw in einval:
        assert hook(**kw) == P.PPS_EINVAL, kw
        assert m.L.pps_map_last_error(m.h) != b""
    assert hook() == P.PPS_ESTATE and b"render" in m.L.pps_map_last_error(m.h)
    assert hook(npx=7) == P.PPS_ESTATE                                   # (no view to have a size)
    with pytest.raises(P.PpsError) as e:
        m.debug_compare(cloud, pid, 1)
    assert e.value.code == P.PPS_ESTATE
    none_present()
    assert m.build_grid(cell=0.05) == (0, 0)                             # a grid, still no render
    assert hook() == P.PPS_ESTATE
    # a render (of a grid without cells: made on the host): now the frame's size is judged too
    m.render(8, 6, IK, IDENT)
    view = m.render_download(); info = m.render_info(); before = state()
    for kw in einval + [dict(npx=k) for k in (0, -1, 47, 49, 6, 8, 1 << 40)]:
        assert hook(**kw) == P.PPS_EINVAL, kw
    for nplanes, tol in ((0, 0.05), (66, 0.05), (1, np.nan), (1, -1.0)):
        assert L.pps_map_compare(m.h, fake, nplanes, tol, None) == P.PPS_EINVAL   # (judged before the context is looked at)
    with pytest.raises(P.PpsError) as e:
        m.debug_compare(cloud[:47], pid[:47], 1)
    assert e.value.code == P.PPS_EINVAL and "width * height" in str(e.value)
    with pytest.raises(ValueError):
        m.debug_compare(cloud, pid[:47], 1)
    none_present()
    assert state() == before and m.render_info() == info and all(m.render_download()[k].tobytes() == view[k].tobytes() for k in view)
    # a grid call ends the view and with it anything that could be compared
    assert m.build_grid(cell=0.05) == (0, 0)
    assert hook() == P.PPS_ESTATE
    none_present()
    m.close(); g.close()


def test_point_host_checks_its_pointers(built):
    L = P.lib()
    d4 = (C.c_double * 4)(0, 0, 1, -2); f3 = (C.c_float * 3)(); e = C.c_double(); q = C.c_int64()
    assert L.pps_map_compare_point_host(None, f3, 0.1, C.byref(e), C.byref(q)) == -1
    assert L.pps_map_compare_point_host(d4, None, 0.1, C.byref(e), C.byref(q)) == -1
    assert L.pps_map_compare_point_host(d4, f3, 0.1, None, C.byref(q)) == -1
    assert L.pps_map_compare_point_host(d4, f3, 0.1, C.byref(e), None) == -1
    for bad in ([0, 0, 0, 1], [np.nan, 0, 1, 0], [np.inf, 0, 0, 1], [1e200, 1e200, 0, 1]):
        with pytest.raises(P.PpsError):
            P.map_compare_point_host(bad, [0, 0, 0], 0.1)
    assert P.map_compare_point_host([0, 0, 2, -4], [5, 6, 2.5], 0.5) == (True, 0.5, 2048)


# ---- one point against one plane -----------------------------------------------------------------------------------------------------
def _check_points(abcd, xyz, tol):
    """the host call against the statement, bit for bit; returns (agree, e, q) of the statement"""
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    agree, e, q = ref_point(np.asarray(abcd, dtype=np.float64), xyz[:, 0], xyz[:, 1], xyz[:, 2], tol)
    for i, p in enumerate(xyz):
        a, ee, qq = P.map_compare_point_host(abcd, p, tol)
        assert a == bool(agree[i]) and qq == int(q[i]), (abcd, p, tol)
        assert np.float64(ee).tobytes() == np.float64(e[i]).tobytes() or (math.isnan(ee) and np.isnan(e[i])), (abcd, p, tol)
    return agree, e, q


def test_point_host_on_random_points_and_planes(built):
    rng = np.random.default_rng(51)
    n_agree = n_sat = total = 0
    for _ in range(40):
        abcd = rng.normal(size=4) * rng.choice([1e-3, 1.0, 50.0])
        l, n, _, _ = frame_exact(abcd)
        on = -(abcd[3] / l) * n + rng.normal(size=(260, 3)) * rng.choice([0.5, 5.0, 200.0])
        on -= ((on @ n) + abcd[3] / l)[:, None] * n                      # on the plane, then off it by a little or a lot
        pts = on + (rng.normal(size=260) * rng.choice([0.01, 0.05, 1.0, 300.0], size=260))[:, None] * n
        agree, e, q = _check_points(abcd, pts, 0.05)
        n_agree += int(agree.sum()); n_sat += int((np.abs(q) == Q_MAX).sum()); total += len(q)
    assert total >= 10000 and 0.2 * total < n_agree < 0.8 * total and n_sat > 100


def test_point_host_on_the_edges_of_every_rule(built):
    flat = [0.0, 0.0, 1.0, 0.0]                                          # e = z exactly
    z = lambda s: [0.25, -3.0, s / 4096.0]
    # ties go to even
    ties = [0.5, -0.5, 1.5, -1.5, 2.5, -2.5]
    _, e, q = _check_points(flat, [z(s) for s in ties], 0.05)
    assert e.tolist() == [s / 4096.0 for s in ties] and q.tolist() == [0, 0, 2, -2, 2, -2]
    # saturation: the last value that rounds, and the first that does not
    _, _, q = _check_points(flat, [z(s) for s in (524287.5, -524287.5, 524288.0, -524288.0, 524287.0, -524287.0, 1e9, -1e9)], 0.05)
    assert q.tolist() == [Q_MAX, -Q_MAX, Q_MAX, -Q_MAX, Q_MAX - 1, -(Q_MAX - 1), Q_MAX, -Q_MAX]
    # |e| = tol exactly agrees, the next double does not; tol = 0 takes points on the plane alone
    t = float(np.float32(0.05))
    for p, tol, want in ((z(4096.0 * t), t, True), (z(-4096.0 * t), t, True), (z(4096.0 * t), np.nextafter(t, 0.0), False), (z(0.0), 0.0, True),
                         (z(-0.0), 0.0, True), (z(4096.0 * float(np.float32(1e-45))), 0.0, False)):
        agree, _, _ = _check_points(flat, [p], tol)
        assert bool(agree[0]) is want, (p, tol)
    # coordinates that are huge or not numbers: q saturates, a NaN goes to the top and never agrees (0 * inf is one)
    junk = [[1e30, 0, 0], [0, 0, 1e30], [0, 0, -1e30], [np.inf, 0, 0], [0, 0, np.inf], [0, 0, -np.inf], [np.nan, 0, 0], [0, 0, np.nan], [np.inf, -np.inf, np.inf]]
    agree, e, q = _check_points(flat, junk, 1e308)
    assert q.tolist() == [0, Q_MAX, -Q_MAX, Q_MAX, Q_MAX, -Q_MAX, Q_MAX, Q_MAX, Q_MAX]
    assert agree.tolist() == [True, True, True, False, False, False, False, False, False] and np.isnan(e[3]) and e[5] == -np.inf
    agree, _, q = _check_points(TILTED, junk, 0.05)
    assert not agree.any() and set(np.abs(q).tolist()) == {Q_MAX}
    # the frame takes another axis at |n_z| = 0.7: n and dn are the same on both sides
    rng = np.random.default_rng(52)
    pts = rng.normal(size=(50, 3))
    for nz in (0.7, np.nextafter(0.7, 0.0), np.nextafter(0.7, 1.0), -0.7, 0.69, 0.71):
        s = math.sqrt(1.0 - nz * nz)
        _check_points([s * 0.6, s * 0.8, nz, -0.3], pts, 0.05)
        _check_points([2.5 * s, 0.0, 2.5 * nz, 4.0], pts, 0.05)


# ---- the statement against a loop ----------------------------------------------------------------------------------------------------
def _mixed_frame(rng, h, w, planes, eq, nplanes, tol, junk=True):
    """a made-up view and a frame for it (compare_helpers.mixed_frame)"""
    r = rng.integers(-1, len(planes), size=(h, w))
    view_id, on = made_up_view(rng, r, planes, eq)
    return (view_id,) + mixed_frame(rng, on, r, eq, nplanes, tol, junk)


def _loop_compare(view_id, planes, eq, cloud, fid, nplanes, tol):
    """the statement again, one pixel at a time in plain Python: table[(k, r)] = [n, n_agree, sum_q, sum_q2] and the classes"""
    table, cls, bad = {}, dict(both=0, frame=0, view=0, neither=0), 0
    ids = planes["plane_id"].tolist()
    for v, c, k in zip(view_id.reshape(-1).tolist(), cloud.reshape(-1), fid.reshape(-1).tolist()):
        frame = 0 <= k < nplanes and bool((int(c["rgba"]) >> 24) & 1)
        bad += k < -1 or k >= nplanes
        seen = v != -1
        cls["both" if frame and seen else "frame" if frame else "view" if seen else "neither"] += 1
        if not (frame and seen):
            continue
        r = ids.index(v)
        agree, _, q = ref_point(eq[r], c["x"], c["y"], c["z"], tol)
        t = table.setdefault((k, r), [0, 0, 0, 0])
        t[0] += 1; t[1] += int(agree); t[2] += int(q); t[3] += int(q) ** 2
    return table, cls, bad


def test_ref_compare_against_a_plain_loop():
    rng = np.random.default_rng(53)
    planes, eq = plane_table([3, 4, 9]), np.array([GROUND, WALL, TILTED])
    view_id, cloud, fid = _mixed_frame(rng, 7, 9, planes, eq, 4, 0.05)
    want = ref_compare(view_id, planes, eq, cloud, fid, 4, 0.05)
    table, cls, bad = _loop_compare(view_id, planes, eq, cloud, fid, 4, 0.05)
    t = want["totals"]
    assert (t["n_both"], t["n_frame_only"], t["n_view_only"], t["n_neither"], t["n_bad_id"]) == (cls["both"], cls["frame"], cls["view"], cls["neither"], bad)
    assert bad == 6 and min(cls.values()) > 0 and (t["width"], t["height"], t["n_pairs"]) == (9, 7, len(table))
    got = {(int(p["frame_plane"]), int(p["row"])): [int(p[f]) for f in ("n", "n_agree", "sum_q", "sum_q2")] for p in want["pairs"]}
    assert got == table and list(got) == sorted(got)
    assert all(planes["plane_id"][p["row"]] == p["plane_id"] for p in want["pairs"])
    for k in range(4):
        mine = {r: v for (kk, r), v in table.items() if kk == k and v[1] >= 1}
        best = min(mine, key=lambda r: (-mine[r][1], -mine[r][0], r)) if mine else -1
        p = want["planes"][k]
        assert p["best_row"] == best and p["best_plane_id"] == (planes["plane_id"][best] if best >= 0 else -1)
        assert (p["best_n"], p["best_agree"]) == ((mine[best][0], mine[best][1]) if mine else (0, 0))
        assert p["n_valid"] - p["n_new"] == sum(v[0] for (kk, r), v in table.items() if kk == k)
    for r in range(3):
        assert want["rows"]["n_view"][r] == np.count_nonzero(view_id == planes["plane_id"][r])
    assert want["rows"]["n_unseen"].sum() == cls["view"] and want["planes"]["n_new"].sum() == cls["frame"]
    assert np.any(np.abs(want["pairs"]["sum_q"]) > 0) and np.any(want["pairs"]["n_agree"] < want["pairs"]["n"])


# ---- the kernels, compiled for the host ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("compareemu")
    so = d / "libcompare_emu.so"
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-fPIC", "-shared", "-pthread", "-ffp-contract=off",
                           "-I", os.path.join(ROOT, "tests", "cpp", "grid_emu"), "-I", os.path.join(ROOT, "pop_up_slam_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "compare_emu.cpp"), "-o", str(so)])
    E = C.CDLL(str(so))
    E.emu_compare.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double] + [C.c_void_p] * 9
    sizes = (C.c_int * 4)(); E.emu_compare_sizes(sizes)
    E.block_bytes, E.planes_at, E.slots, E.px_per_group = list(sizes)
    assert E.planes_at == 48 and E.block_bytes >= 48 + 65 * 40
    return E


def emu_compare(E, view_id, planes, eq, cloud, fid, nplanes, tol):
    """every output of the emulated kernels, as ref_compare returns them"""
    h, w = np.shape(view_id)
    n_rows = len(planes)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    view_id = np.ascontiguousarray(view_id, dtype=np.int32); cloud = np.ascontiguousarray(cloud); fid = np.ascontiguousarray(fid, dtype=np.int32)
    ids = np.ascontiguousarray(planes["plane_id"], dtype=np.int32); eq = np.ascontiguousarray(eq, dtype=np.float64).reshape(-1)
    table = np.full(4 * (nplanes + 1) * (n_rows + 1) + 1, 0x5555, dtype=np.uint64)          # (the call clears it)
    block = np.zeros(E.block_bytes, dtype=np.uint8)
    rows = np.zeros(n_rows, dtype=P.MAP_COMPARE_ROW_DTYPE); pairs = np.zeros(nplanes * n_rows, dtype=P.MAP_COMPARE_PAIR_DTYPE)
    assert E.emu_compare(h * w, nplanes, n_rows, tol, vp(cloud), vp(fid), vp(view_id), vp(ids), vp(eq), vp(table), vp(block), vp(rows), vp(pairs)) == 0
    head = block[:48].view(np.int64)
    totals = dict(width=w, height=h, nplanes=nplanes, n_rows=n_rows, n_both=int(head[0]), n_frame_only=int(head[1]), n_view_only=int(head[2]),
                  n_neither=int(head[3]), n_bad_id=int(head[4]), n_pairs=int(head[5]))
    assert not pairs[totals["n_pairs"]:].view(np.uint8).any()            # nothing written behind the list
    return dict(planes=block[48:48 + 40 * nplanes].view(P.MAP_COMPARE_PLANE_DTYPE).copy(), rows=rows, pairs=pairs[:totals["n_pairs"]], totals=totals)


def emu_check(E, view_id, planes, eq, cloud, fid, nplanes, tol=0.05):
    want = ref_compare(view_id, planes, eq, cloud, fid, nplanes, tol)
    assert_compare_equal(emu_compare(E, view_id, planes, eq, cloud, fid, nplanes, tol), want)
    return want


THREE = (plane_table([3, 4, 9]), np.array([GROUND, WALL, TILTED]))


@pytest.mark.parametrize("size", [(1, 1), (5, 3), (17, 9), (64, 48), (257, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_emulated_three_planes(emu, size):
    w, h = size
    rng = np.random.default_rng(54 + w)
    view_id, cloud, fid = _mixed_frame(rng, h, w, *THREE, 4, 0.05, junk=w * h > 40)
    want = emu_check(emu, view_id, *THREE, cloud, fid, 4)
    if w * h > 1000:
        assert want["totals"]["n_pairs"] == 12 and want["totals"]["n_bad_id"] == 6 and np.all(want["planes"]["best_row"] >= 0)


def _one_point_each(rng, r, fid, planes, eq, tol=0.05):
    view_id, on = made_up_view(rng, r, planes, eq)
    return view_id, shifted(on, r, eq, rng.choice([0.3, -0.8, 1.2, -2.0], size=np.shape(r)) * tol), np.asarray(fid, dtype=np.int32)


@pytest.mark.parametrize("shape", [(1, 64), (8, 8)], ids=["64x1", "8x8"])
def test_emulated_64_pixels_of_64_entries_and_of_one(emu, shape):
    rng = np.random.default_rng(55)
    one = (plane_table([7]), np.array([WALL]))
    k = np.arange(64).reshape(shape)
    view_id, cloud, fid = _one_point_each(rng, np.zeros(shape, int), k, *one)
    want = emu_check(emu, view_id, *one, cloud, fid, 64)
    assert want["totals"]["n_pairs"] == 64 and np.all(want["pairs"]["n"] == 1)
    eight = (plane_table(list(range(10, 90, 10))), np.array([[1.0, 0.1 * j, 0.0, -2.0 - j] for j in range(8)]))
    view_id, cloud, fid = _one_point_each(rng, k % 8, k // 8, *eight)
    want = emu_check(emu, view_id, *eight, cloud, fid, 8)
    assert want["totals"]["n_pairs"] == 64 and np.all(want["pairs"]["n"] == 1)
    view_id, cloud, fid = _one_point_each(rng, np.full(shape, 5), np.full(shape, 3), *eight)
    want = emu_check(emu, view_id, *eight, cloud, fid, 8)
    assert want["totals"]["n_pairs"] == 1 and want["pairs"]["n"][0] == 64 and want["pairs"][0]["row"] == 5


def test_emulated_more_entries_than_the_workgroup_table_holds(emu):
    """one workgroup's pixels with more distinct entries than its table in LDS has slots: the rest goes to memory wave by wave"""
    rng = np.random.default_rng(56)
    n = min(emu.px_per_group, 65 * 12)
    assert n > 4 * emu.slots
    tab = (plane_table(list(range(100, 112))), np.array([[0.2 * j, 1.0, 0.3, 1.0 + j] for j in range(12)]))
    k = rng.permutation(n).reshape(1, n)
    view_id, cloud, fid = _one_point_each(rng, k % 12, k // 12, *tab)
    want = emu_check(emu, view_id, *tab, cloud, fid, 65)
    assert want["totals"]["n_pairs"] == n and want["totals"]["n_both"] == n


def test_emulated_margins_and_junk(emu):
    rng = np.random.default_rng(57)
    view_id, cloud, fid = _mixed_frame(rng, 12, 40, *THREE, 3, 0.05)
    want = emu_check(emu, view_id, *THREE, cloud, fid, 3)
    t = want["totals"]
    assert min(t["n_both"], t["n_frame_only"], t["n_view_only"], t["n_neither"]) > 10 and t["n_bad_id"] == 6
    assert np.any(np.abs(want["pairs"]["sum_q"]) >= Q_MAX)               # a point at infinity saturates
    # a view without a hit, and a plane table without a row
    none = np.full((12, 40), -1)
    emu_check(emu, made_up_view(rng, none, *THREE)[0], *THREE, cloud, fid, 3)
    empty = (plane_table([]), np.zeros((0, 4)))
    want = emu_check(emu, made_up_view(rng, none, *empty)[0], *empty, cloud, fid, 3)
    assert want["totals"]["n_pairs"] == 0 and want["totals"]["n_both"] == 0 and len(want["rows"]) == 0


def test_emulated_best_landmark_ties(emu):
    rng = np.random.default_rng(58)
    tab = (plane_table([5, 6, 8]), np.array([GROUND, WALL, TILTED]))
    r = rng.permutation(np.arange(20 * 21) % 3).reshape(20, 21)
    view_id, on = made_up_view(rng, r, *tab)
    cloud, fid = ties_frame(rng, on, r, tab[1], 0.05)
    check_ties(emu_check(emu, view_id, *tab, cloud, fid, 4), [5, 6, 8])


def test_emulated_65_planes_against_300_landmarks(emu):
    rng = np.random.default_rng(59)
    tab = (plane_table(list(range(2, 902, 3))), np.array([[1.0, 0.0, 0.0, -2.0 - 0.01 * ((j * 37) % 300)] for j in range(300)]))
    r = rng.integers(-1, 300, size=(48, 64))
    view_id, on = made_up_view(rng, r, *tab)
    cloud = shifted(on, r, tab[1], rng.normal(size=r.shape) * 0.05)
    fid = rng.integers(-1, 65, size=r.shape).astype(np.int32)
    want = emu_check(emu, view_id, *tab, cloud, fid, 65)
    assert want["totals"]["n_pairs"] > 2500 and len(want["rows"]) == 300 and np.all(want["planes"]["n_valid"] > 0)


def test_emulated_160x120_of_one_entry(emu):
    """every workgroup adds to the same four counters (19 workgroups here: a thread per GPU thread makes 640 x 480 take half a minute on
    the host; the device test has that size)"""
    rng = np.random.default_rng(60)
    one = (plane_table([7]), np.array([WALL]))
    r = np.zeros((120, 160), int)
    view_id, on = made_up_view(rng, r, *one)
    cloud = shifted(on, r, one[1], rng.normal(size=r.shape) * 0.05)
    want = emu_check(emu, view_id, *one, cloud, np.zeros(r.shape, np.int32), 1)
    assert want["pairs"]["n"].tolist() == [19200] and 0.5 * 19200 < want["pairs"]["n_agree"][0] < 0.8 * 19200
