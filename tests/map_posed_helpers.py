"""What tests/test_host_map_posed.py and tests/test_gpu_map_posed.py share: the posed map (include/pps.h: pps_map_build_posed) restated in
numpy from the text of the statement, and the bounds the tests hold the library to.  None of it calls the code under test.

numpy rounds every elementwise product and sum once, so with dtype = float64 the functions below follow the statement operation for
operation; with dtype = longdouble they give the same quantities with 11 more bits, which is how the tests check that a case is well
conditioned (the fp64 evaluation stays inside the bound of the longdouble one)."""
import numpy as np

EPS64 = float(np.finfo(np.float64).eps)


def quat_to_R(q, dtype=np.float64):
    """Eigen::Matrix3d(q) for q = (x, y, z, w), no renormalisation, in the operation order of csrc/pps_geom.h"""
    x, y, z, w = (dtype(v) for v in q)
    two = dtype(2); one = dtype(1)
    tx, ty, tz = two * x, two * y, two * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[one - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, one - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, one - (txx + tyy)]], dtype=dtype)


def motion(T0, tq, dtype=np.float64):
    """D (12,): R_D = R R0^T with every entry (a*b + c*d) + e*f, t_D = t - R_D t0 summed the same way; T0 4x4 fp32, tq = (t, q)"""
    T0 = np.asarray(T0, dtype=np.float32).reshape(4, 4).astype(dtype)
    tq = np.asarray(tq, dtype=np.float64).astype(dtype)
    R = quat_to_R(tq[3:], dtype)
    R0, t0, t = T0[:3, :3], T0[:3, 3], tq[:3]
    D = np.zeros(12, dtype=dtype)
    for i in range(3):
        for j in range(3):
            D[3 * i + j] = (R[i, 0] * R0[j, 0] + R[i, 1] * R0[j, 1]) + R[i, 2] * R0[j, 2]
        D[9 + i] = t[i] - ((D[3 * i] * t0[0] + D[3 * i + 1] * t0[1]) + D[3 * i + 2] * t0[2])
    return D


def move_points(D, abcd, xyz32, dtype=np.float64):
    """the points of the posed map BEFORE the cast to fp32, (n, 3) in dtype: moved by D (None: not moved), projected onto abcd (None: not)"""
    p = np.asarray(xyz32, dtype=np.float32).reshape(-1, 3).astype(dtype)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    if D is not None:
        D = np.asarray(D).astype(dtype)
        x, y, z = (((D[0] * x + D[1] * y) + D[2] * z) + D[9], ((D[3] * x + D[4] * y) + D[5] * z) + D[10], ((D[6] * x + D[7] * y) + D[8] * z) + D[11])
    if abcd is not None:
        a = np.asarray(abcd, dtype=np.float64).astype(dtype)
        l = np.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
        nx, ny, nz, dd = a[0] / l, a[1] / l, a[2] / l, -a[3] / l
        s = (nx * x + ny * y + nz * z) - dd
        x, y, z = x - nx * s, y - ny * s, z - nz * s
    return np.stack([x, y, z], axis=1)


def motion_bound(T0, tq):
    """16 eps64 (1 + |t| + |t0|): the ten-odd roundings on entries of magnitude <= 1 + |t|"""
    T0 = np.asarray(T0, dtype=np.float64).reshape(4, 4)
    return 16 * EPS64 * (1 + np.linalg.norm(np.asarray(tq, dtype=np.float64)[:3]) + np.linalg.norm(T0[:3, 3]))


def point_abs_bound(D, xyz32):
    """64 eps64 (1 + |p| + |t_D|) per point: the absolute term for coordinates that cancel towards zero"""
    p = np.asarray(xyz32, dtype=np.float64).reshape(-1, 3)
    tD = 0.0 if D is None else float(np.linalg.norm(np.asarray(D, dtype=np.float64)[9:]))
    with np.errstate(all="ignore"):
        return 64 * EPS64 * (1 + np.linalg.norm(p, axis=1) + tD)


def assert_points_within(got32, want, abs_term):
    """map_helpers.assert_within_one_ulp, widened by abs_term (per point, or a scalar): every coordinate of got32 lies between the fp32
    neighbour below float32(want - abs_term) and the one above float32(want + abs_term)"""
    want = np.asarray(want, dtype=np.float64).reshape(-1, 3)
    a = np.broadcast_to(np.asarray(abs_term, dtype=np.float64).reshape(-1, 1), want.shape)
    lo = np.nextafter((want - a).astype(np.float32), np.float32(-np.inf))
    hi = np.nextafter((want + a).astype(np.float32), np.float32(np.inf))
    got32 = np.asarray(got32, dtype=np.float32).reshape(-1, 3)
    ok = (got32 >= lo) & (got32 <= hi)
    assert np.all(ok), (int(np.count_nonzero(~ok)), float(np.max(np.abs(got32.astype(np.float64) - want))))


# ---- poses ---------------------------------------------------------------------------------------------------------------------------
def quat_from_axis_angle(axis, angle):
    a = np.asarray(axis, dtype=np.float64); a = a / np.linalg.norm(a)
    return np.concatenate([a * np.sin(angle / 2), [np.cos(angle / 2)]])


def quat_mul(a, b):
    ax, ay, az, aw = a; bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz])


def T_of(tq):
    """4x4 float64 of a pose (t, q)"""
    T = np.eye(4); T[:3, :3] = quat_to_R(np.asarray(tq)[3:]); T[:3, 3] = np.asarray(tq)[:3]
    return T


def compose(tq, err_t, err_axis, err_angle):
    """tq o E for E = (err_t, rotation of err_angle about err_axis) in the frame of tq"""
    tq = np.asarray(tq, dtype=np.float64)
    q = quat_mul(tq[3:], quat_from_axis_angle(err_axis, err_angle))
    return np.concatenate([tq[:3] + quat_to_R(tq[3:]) @ np.asarray(err_t, dtype=np.float64), q / np.linalg.norm(q)])


def random_pose(rng, spread=5.0):
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    return np.concatenate([rng.normal(size=3) * spread, q])


def inverse_affine_ld(T32, p):
    """T^-1 p in longdouble for the 4x4 fp32 matrix T taken as exact (Cramer's rule on its 3x3 block: T is rigid to fp32 only, so the
    transpose is not its inverse); p (n, 3)"""
    T = np.asarray(T32, dtype=np.float32).reshape(4, 4).astype(np.longdouble)
    A = T[:3, :3]; b = np.asarray(p).astype(np.longdouble) - T[:3, 3]
    c = np.array([[A[1, 1] * A[2, 2] - A[1, 2] * A[2, 1], A[0, 2] * A[2, 1] - A[0, 1] * A[2, 2], A[0, 1] * A[1, 2] - A[0, 2] * A[1, 1]],
                  [A[1, 2] * A[2, 0] - A[1, 0] * A[2, 2], A[0, 0] * A[2, 2] - A[0, 2] * A[2, 0], A[0, 2] * A[1, 0] - A[0, 0] * A[1, 2]],
                  [A[1, 0] * A[2, 1] - A[1, 1] * A[2, 0], A[0, 1] * A[2, 0] - A[0, 0] * A[2, 1], A[0, 0] * A[1, 1] - A[0, 1] * A[1, 0]]], dtype=np.longdouble)
    det = A[0, 0] * c[0, 0] + A[0, 1] * c[1, 0] + A[0, 2] * c[2, 0]
    inv = c / det
    return np.stack([inv[i, 0] * b[:, 0] + inv[i, 1] * b[:, 1] + inv[i, 2] * b[:, 2] for i in range(3)], axis=1)
