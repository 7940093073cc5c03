"""CPU: the posed map (include/pps.h: pps_map_set_frame_pose .. pps_map_move_point_host) before any kernel runs on a device.

  * pps_map_motion_host / pps_map_move_point_host against the numpy restatement of map_posed_helpers, within the bounds the statement's
    arithmetic allows; the restatement itself is held to the same bounds against its evaluation in longdouble, so a case that is badly
    conditioned fails here and not on the device;
  * every PPS_EINVAL of the frame records is answered without a device and leaves the record as it was;
  * the layout of pps_map_frame against a C program compiled with the header;
  * the property the feature exists for: points stored with a wrong capture pose return to where the true pose puts them, while the
    projection alone leaves them a decimetre away inside the plane;
  * k_map_motion and k_map_build_posed themselves, compiled for the host (tests/cpp/map_posed_emu.cpp: one std::thread per GPU thread,
    barriers at the wave operations), against the host functions, bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pop_up_slam_amd as P
import map_posed_helpers as H
from map_helpers import project_to_plane, random_points, raw16, xyz_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_T, ERR_AXIS, ERR_ANGLE = [0.25, -0.12, 0.11], [0.2, 1.0, -0.3], np.deg2rad(5.0)       # |ERR_T| = 0.3 m


def _cases(rng, n):
    """(T0 fp32 4x4, tq) pairs: a capture pose 0.3 m / 5 degrees off a random pose, the estimate another such step away"""
    out = []
    for _ in range(n):
        true = H.random_pose(rng)
        T0 = H.T_of(H.compose(true, ERR_T, rng.normal(size=3), ERR_ANGLE)).astype(np.float32)
        out.append((T0, H.compose(true, rng.normal(size=3) * 0.05, rng.normal(size=3), 0.01)))
    return out


# ---- host functions against the restatement ------------------------------------------------------------------------------------------
def test_motion_host_against_the_restatement(built):
    rng = np.random.default_rng(1)
    for T0, tq in _cases(rng, 50):
        D = P.map_motion_host(T0, tq)
        want, ld = H.motion(T0, tq), H.motion(T0, tq, np.longdouble)
        bound = H.motion_bound(T0, tq)
        assert np.max(np.abs((want.astype(np.longdouble) - ld).astype(np.float64))) <= bound      # the case is well conditioned
        assert np.max(np.abs(D - want)) <= bound
        R = D[:9].reshape(3, 3)
        assert np.max(np.abs(R @ R.T - np.eye(3))) < 1e-6                # a rotation, to the rigidity of an fp32 T0


def test_move_point_host_against_the_restatement(built):
    rng = np.random.default_rng(2)
    pts = xyz_of(random_points(rng, 64))
    for T0, tq in _cases(rng, 12):
        D = P.map_motion_host(T0, tq)
        n = rng.normal(size=3); abcd = np.concatenate([n / np.linalg.norm(n), [rng.uniform(-3, 3)]]) * rng.uniform(0.5, 2.0)
        for d, pl in ((D, abcd), (D, None), (None, abcd), (None, None)):
            got = np.stack([P.map_move_point_host(d, pl, p) for p in pts])
            want, ld = H.move_points(d, pl, pts), H.move_points(d, pl, pts, np.longdouble)
            bound = H.point_abs_bound(d, pts)
            assert np.max(np.abs((want.astype(np.longdouble) - ld).astype(np.float64)), axis=1).max() <= bound.min()
            H.assert_points_within(got, want, bound)
            if d is None and pl is None:
                np.testing.assert_array_equal(got.view(np.uint32), pts.view(np.uint32))               # the stored bits
            if d is None and pl is not None:                             # pps_map_build's point: the reference map_helpers holds it to
                H.assert_points_within(got, project_to_plane(pl, pts), 0.0)


def test_move_point_host_passes_odd_values_through(built):
    odd = np.array([np.nan, -0.0, np.inf], dtype=np.float32)
    np.testing.assert_array_equal(P.map_move_point_host(None, None, odd).view(np.uint32), odd.view(np.uint32))
    L = P.lib()
    out = np.zeros(3, dtype=np.float32)
    assert L.pps_map_move_point_host(None, None, None, out.ctypes.data_as(C.POINTER(C.c_float))) == P.PPS_EINVAL
    assert L.pps_map_motion_host(None, None, None) == P.PPS_EINVAL


# ---- the argument contract -----------------------------------------------------------------------------------------------------------
def test_frame_records_without_a_device(built):
    g = P.Graph()
    pose = g.add_pose([0, 0, 1, 0, 0, 0, 1]); pose2 = g.add_pose([1, 0, 1, 0, 0, 0, 1]); plane = g.add_plane([0, 0, 1, 0])
    m = P.Map(g, 100)
    cloud = random_points(np.random.default_rng(3), 4)
    for f in range(3):
        m.debug_add_points(cloud, np.zeros(4, np.int32), 10 + f, [])     # frames without planes: no pixel is read, no device
    fr = m.frames()
    assert fr["frame"].tolist() == [0, 1, 2] and fr["frame_seq_id"].tolist() == [10, 11, 12] and fr["pose_id"].tolist() == [-1] * 3
    assert not fr["T_wc"].any()
    T = H.T_of(H.random_pose(np.random.default_rng(4))).astype(np.float32)
    m.set_frame_pose(1, pose, T)
    before = m.frames().tobytes()

    def refused(fn):
        with pytest.raises(P.PpsError) as e:
            fn()
        assert e.value.code == P.PPS_EINVAL and str(e.value) != ""
        assert m.frames().tobytes() == before

    bad = []
    t = T.copy(); t[0, 0] = np.nan; bad.append(t)
    t = T.copy(); t[1, 3] = np.inf; bad.append(t)
    t = T.copy(); t[:3, :3] *= np.float32(1.001); bad.append(t)          # R^T R - I = 2e-3
    t = T.copy(); t[0, 1] += np.float32(0.01); bad.append(t)
    t = T.copy(); t[3, 3] = 2.0; bad.append(t)
    t = T.copy(); t[3, 0] = 1e-3; bad.append(t)
    bad.append(np.zeros((4, 4), np.float32))
    for frame in (0, 1):
        for t in bad:
            refused(lambda: m.set_frame_pose(frame, pose, t))
        refused(lambda: m.set_frame_pose(frame, plane, T))               # a plane node as pose
        refused(lambda: m.set_frame_pose(frame, 99, T))
        refused(lambda: m.set_frame_pose(frame, -2, T))
    refused(lambda: m.set_frame_pose(3, pose, T))                        # unknown frames
    refused(lambda: m.set_frame_pose(-1, pose, T))
    refused(lambda: m.set_frame_pose(0, pose, None))                     # a debug frame has no run to take T_wc from
    t = T.copy(); t[:3, :3] *= np.float32(1.00002)                       # R^T R - I = 4e-5: rigid to fp32
    m.set_frame_pose(0, pose, t)
    with pytest.raises(P.PpsError):
        P.map_motion_host(bad[2], [0, 0, 0, 0, 0, 0, 1])
    # overwrite, clear
    m.set_frame_pose(1, pose2, t)
    fr = m.frames()
    assert fr["pose_id"].tolist() == [pose, pose2, -1]
    np.testing.assert_array_equal(fr["T_wc"][1], t); np.testing.assert_array_equal(fr["T_wc"][0], t)
    m.set_frame_pose(1, -1)
    fr = m.frames()
    assert fr["pose_id"].tolist() == [pose, -1, -1] and not fr["T_wc"][1].any()
    g.remove_node(pose2)
    before = m.frames().tobytes()
    refused(lambda: m.set_frame_pose(2, pose2, T))                       # a removed pose node
    # NULL handles and outputs
    L = P.lib(); n = C.c_int()
    assert L.pps_map_set_frame_pose(None, 0, pose, None) == P.PPS_EINVAL
    assert L.pps_map_frames(None, 0, None, C.byref(n)) == P.PPS_EINVAL
    assert L.pps_map_frames(m.h, 2, None, C.byref(n)) == P.PPS_EINVAL
    assert L.pps_map_build_posed(None, None, None, None) == P.PPS_EINVAL
    assert L.pps_map_build_grid_posed(None, None, None, None, None) == P.PPS_EINVAL
    assert L.pps_map_frame_motions(None, 0, None, None, C.byref(n)) == P.PPS_EINVAL
    assert L.pps_map_posed_last(None, None, None, None) == P.PPS_EINVAL
    # a posed build of nothing needs no device; an invalid selection is refused like pps_map_build's
    assert m.build(posed=True) == (0, 0) and m.build_grid(posed=True) == (0, 0)
    D, moved = m.frame_motions()
    assert D.shape == (0, 12) and len(moved) == 0
    assert m.posed_last() == dict(sec=(0.0, 0.0), launches=0, n_unposed_frames=0)
    with pytest.raises(P.PpsError) as e:
        m.build(P.map_select(5, old_every=0), posed=True)
    assert e.value.code == P.PPS_EINVAL
    m.close(); g.close()


def test_frame_struct_layout(built, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pps.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu\\n", sizeof(pps_map_frame), offsetof(pps_map_frame, frame_seq_id), offsetof(pps_map_frame, pose_id),\n'
                   '         offsetof(pps_map_frame, reserved), offsetof(pps_map_frame, T_wc));\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    d = P.FRAME_DTYPE
    assert got == [d.itemsize, d.fields["frame_seq_id"][1], d.fields["pose_id"][1], d.fields["reserved"][1], d.fields["T_wc"][1]]


# ---- the property the feature exists for ---------------------------------------------------------------------------------------------
def test_points_return_to_where_the_true_pose_puts_them(built):
    """A wall seen from a sensor two metres away.  The frame is captured with T0 = T* o E (E: 0.3 m, 5 degrees); its stored points are
    p = T0 s.  With the estimate T* and the true plane the moved point is T* s to the bound of the restatement test; the projection alone
    stays off by the in-plane part of (T0 - T*) s.

    s is DEFINED by the stored fp32 records, s = T0^-1 p in longdouble, so "stored points are T0 s" holds without a rounding of its own.
    What remains between the statement and T* s is that an fp32 T0 is rigid to fp32 only: R R0^T R0 s differs from R s by |R0^T R0 - I| |s|.
    The scene lies where every world coordinate is 8 m or more from the origin and the sensor within 3 m of its points, and the test
    asserts that this term stays below half an fp32 ulp there; the bound itself is not widened."""
    rng = np.random.default_rng(5)
    true = np.concatenate([[12.0, -10.5, 9.0], H.quat_from_axis_angle([0.1, 0.2, 1.0], 0.7)])
    wall = np.array([0.6, -0.8, 0.0, 0.0]); wall[3] = -(wall[:3] @ (true[:3] + 2.0 * wall[:3]))          # two metres in front of the sensor
    n = wall[:3]
    e1 = np.array([0.8, 0.6, 0.0]); e2 = np.array([0.0, 0.0, 1.0])
    uv = rng.uniform(-1.0, 1.0, size=(500, 2))
    w0 = (true[:3] + 2.0 * n) + uv[:, :1] * e1 + uv[:, 1:] * e2
    Tt = H.T_of(true)
    s0 = (w0 - Tt[:3, 3]) @ Tt[:3, :3]                                    # R*^T (w - t*)
    T0 = H.T_of(H.compose(true, ERR_T, ERR_AXIS, ERR_ANGLE)).astype(np.float32)
    p32 = (s0 @ T0[:3, :3].astype(np.float64).T + T0[:3, 3].astype(np.float64)).astype(np.float32)       # the stored records
    s = H.inverse_affine_ld(T0, p32)
    R_ld = H.quat_to_R(true[3:], np.longdouble)
    truth = np.stack([R_ld[i, 0] * s[:, 0] + R_ld[i, 1] * s[:, 1] + R_ld[i, 2] * s[:, 2] + np.longdouble(true[i]) for i in range(3)], axis=1)
    off = (truth @ n.astype(np.longdouble) + np.longdouble(wall[3])).astype(np.float64)
    assert np.max(np.abs(off)) < 1e-5                                     # T* s lies on the wall up to the rounding of the records
    truth = (truth - off[:, None].astype(np.longdouble) * n.astype(np.longdouble)).astype(np.float64)
    assert np.min(np.abs(truth)) >= 8.0 and np.max(np.abs(truth)) < 32.0
    R0 = T0[:3, :3].astype(np.float64)
    nonrigid = np.linalg.norm(R0.T @ R0 - np.eye(3), 2) * np.max(np.linalg.norm(p32.astype(np.float64) - T0[:3, 3], axis=1))
    assert nonrigid < 0.5 * float(np.spacing(np.float32(8.0))), nonrigid
    D = P.map_motion_host(T0, true)
    moved = np.stack([P.map_move_point_host(D, wall, p) for p in p32])
    H.assert_points_within(moved, truth, H.point_abs_bound(D, p32))
    plain = np.stack([P.map_move_point_host(None, wall, p) for p in p32]).astype(np.float64)
    d = (T0.astype(np.float64)[:3, :3] - Tt[:3, :3]) @ s0.T + (T0.astype(np.float64)[:3, 3] - Tt[:3, 3])[:, None]          # (T0 - T*) s
    in_plane = d.T - np.outer(d.T @ n, n)
    assert np.min(np.linalg.norm(in_plane, axis=1)) > 0.1
    assert np.min(np.linalg.norm(plain - truth, axis=1)) > 0.1
    assert np.max(np.abs(np.linalg.norm(plain - truth, axis=1) - np.linalg.norm(in_plane, axis=1))) < 1e-5


# ---- the kernels, compiled for the host ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu(built, tmp_path_factory):
    so = tmp_path_factory.mktemp("posedemu") / "libmap_posed_emu.so"
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-fPIC", "-shared", "-pthread", "-ffp-contract=off",
                           "-I", os.path.join(ROOT, "tests", "cpp", "map_emu"), "-I", os.path.join(ROOT, "pop_up_slam_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "map_posed_emu.cpp"), "-o", str(so)])
    E = C.CDLL(str(so))
    assert E.emu_frame_rec_size() == FRAME_DEV.itemsize
    return E


FRAME_DEV = np.dtype([("T", "<f4", 16), ("pose_slot", "<i4"), ("pad", "<i4")])
vp = lambda a: a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("counts", [[255], [100, 156, 1], [200, 57, 300, 4], [1] * 300 + [211, 2]], ids=["255", "257", "561", "one-point"])
def test_emulated_kernels_against_the_host_functions(emu, counts):
    """chunk c belongs to frame c // 2 (c // 20 among the one-point chunks: a wave sees several frames, a workgroup more chunks than its
    window); every third frame has no motion, every fifth chunk's landmark is gone"""
    rng = np.random.default_rng(len(counts))
    ns = len(counts); per = 20 if ns > 100 else 2
    frame = np.arange(ns) // per; nf = int(frame[-1]) + 1
    ld_pose, ld_plane, n_plane = nf + 3, 7, 5
    pose_est = np.full((7, ld_pose), np.nan)
    plane_est = np.full((4, ld_plane), np.nan)
    planes = [np.concatenate([v / np.linalg.norm(v), [rng.uniform(-2, 2)]]) for v in rng.normal(size=(n_plane, 3))]
    plane_est[:, :n_plane] = np.array(planes).T
    recs = np.zeros(nf, dtype=FRAME_DEV)
    cases = _cases(rng, nf)
    perm = rng.permutation(nf)
    for f, (T0, tq) in enumerate(cases):
        if f % 3 == 2:
            recs[f]["pose_slot"] = -1
        else:
            recs[f]["T"] = T0.reshape(16); recs[f]["pose_slot"] = perm[f]; pose_est[:, perm[f]] = tq
    counts = np.asarray(counts, dtype=np.int64)
    out_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64); n_out = int(out_off[-1])
    store = random_points(rng, n_out + 50)
    src_off = (out_off[:-1] + 50 - np.arange(ns) % 7).astype(np.int64)   # chunks overlap in the store: only the table says where one starts
    slot = np.where(np.arange(ns) % 5 == 4, -1, rng.integers(0, n_plane, size=ns)).astype(np.int32)
    fidx = frame.astype(np.int32)
    motion = np.full((nf + 1, 12), np.nan); moved = np.full(nf + 1, -7, dtype=np.int32)
    assert emu.emu_map_motion(nf, vp(recs), vp(pose_est), ld_pose, vp(motion), vp(moved)) == 0
    assert np.isnan(motion[nf]).all() and moved[nf] == -7
    for f, (T0, tq) in enumerate(cases):
        if f % 3 == 2:
            assert moved[f] == 0 and motion[f].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
        else:
            assert moved[f] == 1
            np.testing.assert_array_equal(motion[f].view(np.uint64), P.map_motion_host(T0, tq).view(np.uint64))
    guard = 5
    B = np.zeros(n_out + guard, dtype=P.POINT_DTYPE); B["rgba"] = 0xDEADBEEF
    assert emu.emu_map_build_posed(C.c_longlong(n_out), ns, vp(out_off), vp(src_off), vp(slot), vp(plane_est), ld_plane, vp(store), vp(B),
                                   vp(fidx), vp(motion), vp(moved)) == 0
    assert np.all(B["rgba"][n_out:] == 0xDEADBEEF)
    want = np.zeros(n_out, dtype=P.POINT_DTYPE)
    for c in range(ns):
        raw = store[src_off[c]:src_off[c] + counts[c]]
        D = motion[frame[c]] if moved[frame[c]] else None
        pl = planes[slot[c]] if slot[c] >= 0 else None
        seg = want[out_off[c]:out_off[c + 1]]
        seg["rgba"] = raw["rgba"]
        xyz = np.stack([P.map_move_point_host(D, pl, p) for p in xyz_of(raw)])
        seg["x"], seg["y"], seg["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    np.testing.assert_array_equal(raw16(B[:n_out]), raw16(want))
    # without any motion the posed kernel writes k_map_build's bytes
    moved0 = np.zeros(nf, dtype=np.int32)
    B0 = np.zeros(n_out, dtype=P.POINT_DTYPE); B1 = np.zeros(n_out, dtype=P.POINT_DTYPE)
    assert emu.emu_map_build_posed(C.c_longlong(n_out), ns, vp(out_off), vp(src_off), vp(slot), vp(plane_est), ld_plane, vp(store), vp(B0),
                                   vp(fidx), vp(motion), vp(moved0)) == 0
    assert emu.emu_map_build(C.c_longlong(n_out), ns, vp(out_off), vp(src_off), vp(slot), vp(plane_est), ld_plane, vp(store), vp(B1)) == 0
    np.testing.assert_array_equal(raw16(B0), raw16(B1))
