"""The geometry of the factor graph stated in arbitrary precision (mpmath, 60 digits) -> tests/golden/mp_geometry_cases.json.

TEST INFRASTRUCTURE.  Everything else the suite compares with (oracle/pps_oracle.c, oracle/numpy_ref.py, the other fixtures) is a
double-precision restatement of the formulas the product also uses.  This file states the QUANTITIES instead, from their definitions:

  rotation of a stored quaternion   R(q) = the quadratic form Eigen::Quaterniond::toRotationMatrix defines (q is used as stored: a
                                    stored double quaternion is unit only to round-off and nothing re-normalises it)
  retractions                       pose: t + d[0:3], q * Exp(d[3:6]);  plane: normalise(Exp(d) * pi) as a quaternion;  the true Exp
  planes                            transform_to(T) = normalise(T^T pi), transform_from(T) = normalise(T^-T pi)
  plane logarithm                   e = Log(p * conj(m)) under the double cover: dq <- -dq if w < 0, then 2 atan2(|v|, w) v / |v|, 0 at v = 0
  Euler angles (ZYX)                read from the rotation MATRIX: atan2(R10, R00), asin(-R20), atan2(R21, R22); differences wrapped to [-pi, pi)
  residuals                         plane observation, re-popping plane observation (Pose3d_Plane3d_Factor2), plane prior, pose prior,
                                    odometry; whitened by a packed upper-triangular U; optionally r <- sign(r) sqrt(rho(r)) per component
  J*                                d r / d (tangent of the retraction): central difference with h = 1e-25 at 60 digits
  J_cd                              the same difference with the reference's step (the double 1e-4) in exact arithmetic: what
                                    numericalDiff would return without round-off
  u(X)                              the conditioning unit: sum_k |X(x with x_k (1 + 2^-52)) - X(x)| + 2^-52 max |X|, entry by entry, one scalar
                                    input at a time -- the error any double-precision algorithm is entitled to from rounded inputs and a
                                    rounded output.  (Stored to three significant digits: it is a unit, not a reference value.)

    python -m oracle.mp_ref --write      # rewrites the cases of the fixture (keeps its "measured" block)
    python -m oracle.mp_ref --measure    # re-measures the CPU oracle against the fixture: rewrites "measured" only

"measured" holds, per case kind and quantity, rho = max |X_oracle - X*| / u(X) of the CPU oracle (oracle/pps_oracle.c) and
K = max(8, 4 rho): the bound the device is held to (tests/test_gpu_mp_geometry.py).  For the numeric Jacobians the unit is
u(J_cd) + u(r) / 1e-4: the round-off of the two residuals of a central difference is divided by the step.
"""
from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "mp_geometry_cases.json")

CD_STEP = 0.0001                      # isamlib/numericalDiff.cpp:34, the double
K_FLOOR, K_FACTOR, K_CAP = 8.0, 4.0, 256.0
COST_NONE, COST_HUBER, COST_PSEUDO_HUBER, COST_CAUCHY = range(4)
POSE, PLANE = 0, 1
# kind -> (node types, residual dimension)
KINDS = {"plane_obs": ((POSE, PLANE), 3), "plane_obs2": ((POSE, PLANE), 3), "plane_prior": ((PLANE,), 3),
         "pose_prior": ((POSE,), 6), "odometry": ((POSE, POSE), 6)}


def _ctx():
    import mpmath
    m = mpmath.mp.clone()
    m.dps = 60
    return m


M = None            # the mpmath context: created by the first call that needs it (the GPU test imports nothing of this)


def _m():
    global M
    if M is None:
        M = _ctx()
    return M


# ---- algebra (lists of mpf; quaternions stored x, y, z, w) -------------------------------------------------------------------------
def mpv(v):
    return [_m().mpf(x) for x in v]


def norm(v):
    return _m().sqrt(sum(x * x for x in v))


def normalise(v):
    n = norm(v)
    return [x / n for x in v]


def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return [aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
            aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz]


def qconj(q):
    return [-q[0], -q[1], -q[2], q[3]]


def qexp(d):
    """Exp of a rotation vector as a unit quaternion"""
    th = norm(d)
    if th == 0:
        return mpv([0, 0, 0, 1])
    s = _m().sin(th / 2) / th
    return [s * d[0], s * d[1], s * d[2], _m().cos(th / 2)]


def rotmat(q):
    x, y, z, w = q
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
            [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
            [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]


def matT_vec(R, v):
    return [R[0][i] * v[0] + R[1][i] * v[1] + R[2][i] * v[2] for i in range(3)]


def mat_vec(R, v):
    return [R[i][0] * v[0] + R[i][1] * v[1] + R[i][2] * v[2] for i in range(3)]


def dot(a, b):
    return sum(x * y for x, y in zip(a, b))


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def pose_retract(p, d):
    return [p[0] + d[0], p[1] + d[1], p[2] + d[2]] + qmul(p[3:], qexp(d[3:]))


def plane_retract(pl, d):
    return normalise(qmul(qexp(d), pl))


def transform_to(pl, pose):
    """the plane in the frame of the pose T = [R t; 0 1]: normalise(T^T pi)"""
    R = rotmat(pose[3:])
    return normalise(matT_vec(R, pl[:3]) + [dot(pose[:3], pl[:3]) + pl[3]])


def transform_from(pl, pose):
    """the inverse: normalise(T^-T pi), T^-1 = [R^T  -R^T t]"""
    R = rotmat(pose[3:])
    n = mat_vec(R, pl[:3])
    return normalise(n + [pl[3] - dot(matT_vec(R, pose[:3]), pl[:3])])


def plane_dq(p, m):
    return qmul(p, qconj(m))


def plane_log(p, m):
    dq = plane_dq(p, m)
    if dq[3] < 0:
        dq = [-x for x in dq]
    nv = norm(dq[:3])
    if nv == 0:
        return mpv([0, 0, 0])
    ang = 2 * _m().atan2(nv, dq[3])
    return [ang * x / nv for x in dq[:3]]


def euler_zyx(R):
    return [_m().atan2(R[1][0], R[0][0]), _m().asin(-R[2][0]), _m().atan2(R[2][1], R[2][2])]


def wrap(a):
    pi = _m().pi
    return a - 2 * pi * _m().floor((a + pi) / (2 * pi))


def euler_to_quat(yaw, pitch, roll):
    """R = Rz(yaw) Ry(pitch) Rx(roll)"""
    m = _m()
    qz = [0, 0, m.sin(yaw / 2), m.cos(yaw / 2)]
    qy = [0, m.sin(pitch / 2), 0, m.cos(pitch / 2)]
    qx = [m.sin(roll / 2), 0, 0, m.cos(roll / 2)]
    return qmul(qmul(qz, qy), qx)


def wall_plane(pose, ray):
    """Pose3d_Plane3d_Factor2's measurement: the ground z = 0 of the world seen from the pose, the two rays of the edge's end points cut
    with it, and the plane through the two points that stands on the ground at a right angle; a unit 4-vector in the sensor frame"""
    R = rotmat(pose[3:])
    g = matT_vec(R, mpv([0, 0, -1])) + [-pose[2]]                         # T^T (0, 0, -1, 0)
    P = []
    for j in range(2):
        r = ray[3 * j:3 * j + 3]
        f = -g[3] / dot(g[:3], r)
        P.append([f * x for x in r])
    n = cross([P[1][i] - P[0][i] for i in range(3)], g[:3])
    return normalise(n + [-dot(n, P[0])])


def unpack_ut(ut, m):
    U = [[0] * m for _ in range(m)]
    k = 0
    for i in range(m):
        for j in range(i, m):
            U[i][j] = ut[k]
            k += 1
    return U


def rho(kind, b, d):
    m = _m()
    if kind == COST_HUBER:
        return d * d if abs(d) < b else 2 * b * abs(d) - b * b
    if kind == COST_PSEUDO_HUBER:
        return 2 * b * b * (m.sqrt(1 + d * d / (b * b)) - 1)
    if kind == COST_CAUCHY:                                               # a product of two logarithms: Graph.set_cost_function
        return m.log(m.pi / b) * m.log(1 + d * d / (b * b))
    return d * d


def basic_error(kind, a, b, meas, ray):
    if kind == "plane_obs":
        return plane_log(transform_to(b, a), meas)
    if kind == "plane_obs2":
        return plane_log(transform_to(b, a), wall_plane(a, ray))
    if kind == "plane_prior":
        return plane_log(a, meas)
    if kind == "pose_prior":
        y = euler_zyx(rotmat(a[3:]))
        return [a[i] - meas[i] for i in range(3)] + [wrap(y[i] - meas[3 + i]) for i in range(3)]
    R1, R2 = rotmat(a[3:]), rotmat(b[3:])
    R12 = [[sum(R1[k][i] * R2[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
    t12 = matT_vec(R1, [b[i] - a[i] for i in range(3)])
    y = euler_zyx(R12)
    return [t12[i] - meas[i] for i in range(3)] + [wrap(y[i] - meas[3 + i]) for i in range(3)]


def residual(kind, a, b, meas, ut, ray, cost):
    e = basic_error(kind, a, b, meas, ray)
    m = len(e)
    U = unpack_ut(ut, m)
    r = [sum(U[i][j] * e[j] for j in range(i, m)) for i in range(m)]
    if cost is not None and cost[0] != COST_NONE:
        bb = _m().mpf(cost[1])
        r = [(-1 if x < 0 else 1) * _m().sqrt(rho(cost[0], bb, x)) for x in r]
    return r


def jacobian(kind, a, b, meas, ut, ray, cost, h):
    """m x (columns of node a | columns of node b), row-major flat; central differences of step h through the retraction"""
    types = KINDS[kind][0]
    cols = []
    for n, t in enumerate(types):
        dim = 6 if t == POSE else 3
        x = a if n == 0 else b
        for j in range(dim):
            ys = []
            for s in (1, -1):
                d = [0] * dim
                d[j] = s * h
                xs = pose_retract(x, d) if t == POSE else plane_retract(x, d)
                ys.append(residual(kind, xs if n == 0 else a, b if n == 0 else xs, meas, ut, ray, cost))
            cols.append([(p - q) / (2 * h) for p, q in zip(*ys)])
    return [cols[c][i] for i in range(len(cols[0])) for c in range(len(cols))]


# ---- one case ------------------------------------------------------------------------------------------------------------------------
_INPUTS = ("a", "b", "meas", "ut", "ray")


def _quantities_at(kind, args, cost, numeric):
    m = _m()
    a, b, meas, ut, ray = args
    out = {"r": residual(kind, a, b, meas, ut, ray, cost), "J": jacobian(kind, a, b, meas, ut, ray, cost, m.mpf(10) ** -25)}
    if numeric:
        out["J_cd"] = jacobian(kind, a, b, meas, ut, ray, cost, m.mpf(CD_STEP))
    return out


def _unit(x0, perturbed):
    m = _m()
    e52 = m.mpf(2) ** -52
    floor = e52 * max(abs(v) for v in x0)
    return [sum(abs(p[i] - x0[i]) for p in perturbed) + floor for i in range(len(x0))]


def _u3(x):
    """a unit to three significant digits"""
    return float("%.2e" % float(x))


def finish_case(c):
    """c: name, kind, tags, numeric, cost, a, b, meas, ut, ray as doubles -> adds r, J, J_cd and their units"""
    m = _m()
    e52 = m.mpf(2) ** -52
    args = [mpv(c[k]) if c.get(k) is not None else None for k in _INPUTS]
    q0 = _quantities_at(c["kind"], args, c.get("cost"), c["numeric"])
    pert = {k: [] for k in q0}
    for n, arr in enumerate(args):
        if arr is None:
            continue
        for k in range(len(arr)):
            if arr[k] == 0:
                continue
            keep = arr[k]
            arr[k] = keep * (1 + e52)
            qp = _quantities_at(c["kind"], args, c.get("cost"), c["numeric"])
            arr[k] = keep
            for name in q0:
                pert[name].append(qp[name])
    for name in ("r", "J", "J_cd"):
        if name in q0:
            c[name] = [float(v) for v in q0[name]]
            c["u_" + name] = [_u3(v) for v in _unit(q0[name], pert[name])]
        else:
            c[name] = None
            c["u_" + name] = None
    if c["kind"] == "plane_obs2":                                        # the re-popped measurement itself
        a, ray = args[0], args[4]
        w0, wp = wall_plane(a, ray), []
        for arr in (a, ray):
            for k in range(len(arr)):
                if arr[k] == 0:
                    continue
                keep = arr[k]
                arr[k] = keep * (1 + e52)
                wp.append(wall_plane(a, ray))
                arr[k] = keep
        c["wall"] = [float(v) for v in w0]
        c["u_wall"] = [_u3(v) for v in _unit(w0, wp)]
    return c


def finish_exmap(c):
    m = _m()
    e52 = m.mpf(2) ** -52
    f = pose_retract if c["kind"] == "exmap_pose" else plane_retract
    x, d = mpv(c["x"]), mpv(c["d"])
    o0 = f(x, d)
    pert = []
    for arr in (x, d):
        for k in range(len(arr)):
            if arr[k] == 0:
                continue
            keep = arr[k]
            arr[k] = keep * (1 + e52)
            pert.append(f(x, d))
            arr[k] = keep
    c["out"] = [float(v) for v in o0]
    c["u_out"] = [_u3(v) for v in _unit(o0, pert)]
    return c


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
def _f(v):
    return [float(x) for x in v]


def _diag_ut(d):
    m = len(d)
    out = []
    for i in range(m):
        out += [d[i]] + [0.0] * (m - 1 - i)
    return out


def _pose(t, ypr):
    m = _m()
    return _f(mpv(t) + normalise(euler_to_quat(*[m.mpf(x) for x in ypr])))


def _unit_plane(v):
    return _f(normalise(mpv(v)))


def _meas_for_dq(p, dq):
    """the measurement m with p * conj(m) = dq, for a unit p"""
    return _f(qmul(qconj(dq), p))


def _dq_tilt(tilt, axis):
    m = _m()
    return qexp([m.mpf(tilt) * x for x in normalise(mpv(axis))])


def _dq_w(w, axis):
    m = _m()
    w = m.mpf(w)
    s = m.sqrt(1 - w * w)
    return [s * x for x in normalise(mpv(axis))] + [w]


def _compose(p1, t_rel, q_rel):
    """p1 (+) rel, as doubles"""
    p1 = mpv(p1)
    R1 = rotmat(p1[3:])
    t2 = [p1[i] + mat_vec(R1, t_rel)[i] for i in range(3)]
    return _f(t2 + normalise(qmul(p1[3:], q_rel)))


def _rel_vector(p1, p2):
    p1, p2 = mpv(p1), mpv(p2)
    R1, R2 = rotmat(p1[3:]), rotmat(p2[3:])
    R12 = [[sum(R1[k][i] * R2[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
    return matT_vec(R1, [p2[i] - p1[i] for i in range(3)]) + euler_zyx(R12), R12


def _case(name, kind, a, b, meas, ut, ray=None, cost=None, numeric=True, tags=()):
    return {"name": name, "kind": kind, "tags": list(tags), "numeric": bool(numeric), "cost": cost,
            "a": _f(a), "b": None if b is None else _f(b), "meas": None if meas is None else _f(meas), "ut": _f(ut),
            "ray": None if ray is None else _f(ray)}


UT3 = _diag_ut([1.5, 0.8, 1.2])
UT6 = _diag_ut([2.0, 1.5, 2.5, 4.0, 5.0, 3.0])
AXIS = [0.3, -0.5, 0.8]
TILTS = ["0.3", "1e-3", "1e-6", "1e-9", "1e-11", "3e-12", "1e-13"]
NEAR_PI_W = ["1e-1", "-1e-1", "1.000000001e-3", "-1.000000001e-3", "1e-6", "-1e-6", "1e-9", "-1e-9"]
PITCH_GAPS = ["1e-2", "1e-4", "1e-6"]


def build_cases():
    m = _m()
    cases = []
    pose0 = _pose([0.7, -1.3, 0.4], [0.5, -0.2, 0.3])
    plane0 = _unit_plane([0.6, -0.3, 0.2, 1.5])
    ident = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    half = [0.5, 0.5, 0.5, -0.5]

    def plane_pair(kind, name, pose, plane, dq, negate=False, ut=UT3, tags=(), numeric=True):
        p = transform_to(mpv(plane), mpv(pose)) if kind == "plane_obs" else mpv(plane)
        ms = _meas_for_dq(p, dq)
        if negate:
            ms = [-x for x in ms]
        if kind == "plane_obs":
            return _case("%s/%s" % (kind, name), kind, pose, plane, ms, ut, tags=tags, numeric=numeric)
        return _case("%s/%s" % (kind, name), kind, plane, None, ms, ut, tags=tags, numeric=numeric)

    # the plane logarithm, on the observation and on the prior
    for kind in ("plane_obs", "plane_prior"):
        for t in TILTS:
            cases.append(plane_pair(kind, "tilt_" + t, pose0, plane0, _dq_tilt(t, AXIS), tags=["tilt_" + t]))
        if kind == "plane_obs":
            cases.append(_case(kind + "/tilt_zero", kind, ident, half, half, UT3, tags=["tilt_zero"]))
        else:
            cases.append(_case(kind + "/tilt_zero", kind, half, None, half, UT3, tags=["tilt_zero"]))
        cases.append(plane_pair(kind, "meas_negated", pose0, plane0, _dq_tilt("0.2", AXIS), negate=True, tags=["meas_negated"]))
        for w in NEAR_PI_W:
            cases.append(plane_pair(kind, "near_pi_w_" + w, pose0, plane0, _dq_w(w, AXIS), tags=["near_pi_w_" + w],
                                    numeric=abs(float(w)) >= 1e-3))
        # plane shapes
        cases.append(plane_pair(kind, "d_zero", pose0, _unit_plane([0.6, -0.3, 0.74, 0.0]), _dq_tilt("0.05", AXIS), tags=["d_zero"]))
        cases.append(plane_pair(kind, "d_dominant", pose0, _unit_plane([0.6e-3, -0.3e-3, 0.742e-3, 1.0]), _dq_tilt("0.05", AXIS),
                                tags=["d_dominant"]))
    far = _pose([1200.0, -800.0, 950.0], [0.5, -0.2, 0.3])
    cases.append(plane_pair("plane_obs", "translation_1e3", far, plane0, _dq_tilt("0.05", AXIS), tags=["translation_1e3"]))
    # axis-aligned corridor configurations: walls along the axes, yaw a multiple of a quarter turn, the measurement off in distance only
    cases.append(_case("plane_obs/corridor_yaw0", "plane_obs", [1.0, 2.0, 0.0, 0.0, 0.0, 0.0, 1.0], _unit_plane([0.0, 1.0, 0.0, -3.0]),
                       _unit_plane([0.0, 1.0, 0.0, -0.9]), UT3, tags=["corridor"]))
    cases.append(_case("plane_obs/corridor_yaw90", "plane_obs", _pose([1.0, 2.0, 0.0], [m.pi / 2, 0, 0]), _unit_plane([1.0, 0.0, 0.0, -3.0]),
                       _unit_plane([0.0, -1.0, 0.0, -2.1]), UT3, tags=["corridor"]))
    # whitening: every entry of U non-zero, magnitudes from 1e-3 to 1e3
    ut3w = [1e3, -1e-3, 0.5, 2e-2, 30.0, 1e-3]
    cases.append(plane_pair("plane_obs", "whitening", pose0, plane0, _dq_tilt("1e-3", AXIS), ut=ut3w, tags=["whitening_3"]))

    # Pose3d_Plane3d_Factor2: camera frame z forward / y down, world z up
    def obs2(name, pose, ray, tilt, tag):
        ms = wall_plane(mpv(pose), mpv(ray))
        seen = qmul(_dq_tilt(tilt, AXIS), ms)                                # the landmark as seen: p * conj(m) = Exp(tilt)
        land = _f(transform_from(seen, mpv(pose)))
        return _case("plane_obs2/" + name, "plane_obs2", pose, land, _f(ms), UT3, ray=ray, tags=[tag])
    cases.append(obs2("ordinary", _pose([1.0, 2.0, 1.5], [-m.pi / 2 + 0.1, 0.05, -m.pi / 2 - 0.08]),
                      [0.3, 0.4, 1.0, -0.2, 0.35, 1.0], "0.02", "factor2_ordinary"))
    cases.append(obs2("ray_near_parallel", _pose([1.0, 2.0, 1.5], [-m.pi / 2, 0, -m.pi / 2]),
                      [0.3, 0.0008, 1.0, -0.2, 0.35, 1.0], "0.02", "factor2_ray_near_parallel"))
    cases.append(obs2("camera_height_1e-2", _pose([1.0, 2.0, 0.01], [-m.pi / 2 + 0.1, 0.05, -m.pi / 2 - 0.08]),
                      [0.3, 0.4, 1.0, -0.2, 0.35, 1.0], "0.02", "factor2_camera_height_1e-2"))

    # Euler residuals
    off6 = mpv([0.05, -0.03, 0.04, 0.012, -0.017, 0.009])
    hp = m.pi / 2

    def prior(name, t, ypr, tags, numeric=True, meas_ypr=None, ut=UT6):
        pose = _pose(t, ypr)
        y = euler_zyx(rotmat(mpv(pose)[3:]))
        ms = [mpv(t)[i] + off6[i] for i in range(3)] + ([y[i] + off6[3 + i] for i in range(3)] if meas_ypr is None else list(meas_ypr))
        return _case("pose_prior/" + name, "pose_prior", pose, None, ms, ut, tags=tags, numeric=numeric)

    def odo(name, p1, t_rel, q_rel, tags, numeric=True, meas_ypr=None, ut=UT6, same=False):
        p2 = list(p1) if same else _compose(p1, mpv(t_rel), q_rel)
        v, R12 = _rel_vector(p1, p2)
        ms = [v[i] + off6[i] for i in range(3)] + ([v[3 + i] + off6[3 + i] for i in range(3)] if meas_ypr is None else list(meas_ypr))
        return _case("odometry/" + name, "odometry", p1, p2, ms, ut, tags=tags, numeric=numeric), R12

    p1 = _pose([2.0, -1.0, 0.5], [0.3, 0.1, -0.2])
    cases.append(prior("ordinary", [2.0, -1.0, 0.5], [0.3, 0.1, -0.2], ["ordinary"]))
    cases.append(odo("ordinary", p1, [1.0, 0.2, -0.1], euler_to_quat(m.mpf("0.2"), m.mpf("-0.1"), m.mpf("0.15")), ["ordinary"])[0])
    for sgn, sname in ((1, "plus"), (-1, "minus")):
        for gap in PITCH_GAPS:
            pitch = sgn * (hp - m.mpf(gap))
            tag = "pitch_%s_%s" % (sname, gap)
            num = float(gap) > 1e-4
            cases.append(prior(tag, [2.0, -1.0, 0.5], [0.4, pitch, -0.7], [tag], numeric=num))
            cases.append(odo(tag, p1, [1.0, 0.2, -0.1], euler_to_quat(m.mpf("0.4"), pitch, m.mpf("-0.7")), [tag], numeric=num)[0])
        # yaw / roll within 1e-6 of +-pi, the measurement on the other side of the wrap
        near = sgn * (m.pi - m.mpf("0.5e-6"))
        other = -sgn * (m.pi - m.mpf("0.4e-6"))
        for which, idx in (("yaw", 0), ("roll", 2)):
            ypr = [m.mpf("0.4"), m.mpf("0.3"), m.mpf("-0.7")]
            ypr[idx] = near
            my = [ypr[0] + off6[3], ypr[1] + off6[4], ypr[2] + off6[5]]
            my[idx] = other
            tag = "%s_wrap_%s" % (which, sname)
            cases.append(prior(tag, [2.0, -1.0, 0.5], ypr, [tag], meas_ypr=my))
            cases.append(odo(tag, p1, [1.0, 0.2, -0.1], euler_to_quat(*ypr), [tag], meas_ypr=my)[0])
    # relative rotations above 120 degrees: the three branches of a matrix -> quaternion conversion that the trace does not take
    for k, (axis, deg) in enumerate((([1.0, 0.1, 0.05], 170), ([0.08, 1.0, -0.06], 175), ([-0.05, 0.07, 1.0], 179))):
        ang = m.mpf(deg) * m.pi / 180
        c, R12 = odo("half_turn_axis%d" % k, p1, [1.0, 0.2, -0.1], qexp([ang * x for x in normalise(mpv(axis))]), ["r_to_quat_branch_%d" % k])
        d = [R12[0][0], R12[1][1], R12[2][2]]
        assert sum(d) < 0 and max(range(3), key=lambda i: d[i]) == k, (k, d)
        cases.append(c)
    for tr, tname in (("5e-10", "plus"), ("-5e-10", "minus")):
        ang = m.acos((m.mpf(tr) - 1) / 2)
        c, R12 = odo("trace_zero_" + tname, p1, [1.0, 0.2, -0.1], qexp([ang * x for x in normalise(mpv([0.5, 0.6, -0.62]))]),
                     ["trace_near_zero"])
        assert abs(R12[0][0] + R12[1][1] + R12[2][2]) < 1e-9
        cases.append(c)
    cases.append(odo("identical_poses", p1, None, None, ["identical_poses"], same=True)[0])
    pfar = _pose([12345.678, -9876.54, 23456.7], [0.3, 0.1, -0.2])
    cases.append(odo("translation_1e4", pfar, [1.0, 0.2, -0.1], euler_to_quat(m.mpf("0.2"), m.mpf("-0.1"), m.mpf("0.15")),
                     ["translation_1e4"])[0])
    ut6w = [1e3, -1e-3, 0.5, 2e-2, -30.0, 1e-3, 50.0, 3e-3, -0.7, 1e-2, 200.0, 2.0, 1e-3, -8.0, 0.3, 700.0, -5e-3, 0.06,
            1e-3, 40.0, 1e3]
    small = [x / 50 for x in off6]
    c = odo("whitening", p1, [1.0, 0.2, -0.1], euler_to_quat(m.mpf("0.2"), m.mpf("-0.1"), m.mpf("0.15")), ["whitening_6"], ut=ut6w)[0]
    v, _ = _rel_vector(c["a"], c["b"])
    c["meas"] = _f([v[i] + small[i] for i in range(6)])
    cases.append(c)

    # robust costs at b = 1: one whitened component at 0.5, just inside and just outside 1, and 5
    targets = (("0.5", "0.5"), ("0.999", "0.998999999"), ("1.001", "1.001000001"), ("5", "5"))
    for cost, cname in ((COST_HUBER, "huber"), (COST_PSEUDO_HUBER, "pseudo_huber"), (COST_CAUCHY, "cauchy")):
        for tname, tval in targets:
            tag = "robust_%s_%s" % (cname, tname)
            c = plane_pair("plane_obs", tag, pose0, plane0, _dq_tilt("1.0", [0.6, 0.3, -0.74]))
            e = basic_error("plane_obs", mpv(c["a"]), mpv(c["b"]), mpv(c["meas"]), None)
            c["ut"] = _f(_diag_ut([m.mpf(tval) / e[0], 0.4, 0.4]))
            c.update(name="robust_plane_obs/" + tag, cost=[cost, 1.0], tags=[tag])
            cases.append(c)
            c = odo(tag, p1, [1.0, 0.2, -0.1], euler_to_quat(m.mpf("0.2"), m.mpf("-0.1"), m.mpf("0.15")), [tag])[0]
            c["meas"][0] -= 0.65
            e = basic_error("odometry", mpv(c["a"]), mpv(c["b"]), mpv(c["meas"]), None)
            c["ut"] = _f(_diag_ut([m.mpf(tval) / e[0], 1.5, 2.5, 4.0, 5.0, 3.0]))
            c.update(name="robust_odometry/" + tag, cost=[cost, 1.0])
            cases.append(c)
    for c in cases:
        check_conditions(c)
    return cases


def check_conditions(c):
    """what a case must satisfy to be compared in the numeric mode: a central difference that straddles a discontinuity is decided by rounding"""
    if not c["numeric"]:
        return
    m = _m()
    kind = c["kind"]
    a, b, meas, ut, ray = [mpv(c[k]) if c.get(k) is not None else None for k in _INPUTS]
    if kind in ("plane_obs", "plane_obs2", "plane_prior"):
        p = a if kind == "plane_prior" else transform_to(b, a)
        ms = wall_plane(a, ray) if kind == "plane_obs2" else meas
        dq = plane_dq(normalise(p), normalise(ms))
        assert abs(dq[3]) >= m.mpf("1e-3"), (c["name"], dq[3])
    else:
        e = basic_error(kind, a, b, meas, ray)
        for x in e[3:]:
            assert m.pi - abs(x) >= m.mpf("1e-3"), (c["name"], x)
    if c.get("cost") and c["cost"][0] == COST_HUBER:
        e = residual(kind, a, b, meas, ut, ray, None)
        for x in e:
            assert abs(abs(x) - c["cost"][1]) >= m.mpf("1e-3"), (c["name"], x)


def build_exmaps():
    m = _m()
    out = []
    pose0 = _pose([0.7, -1.3, 0.4], [0.5, -0.2, 0.3])
    plane0 = _unit_plane([0.6, -0.3, 0.2, 1.5])
    ax = normalise(mpv(AXIS))
    for name, th in (("0", 0), ("1e-6", "1e-6"), ("0.9999e-4", "0.9999e-4"), ("1.0001e-4", "1.0001e-4"), ("0.5", "0.5"),
                     ("pi-1e-3", m.pi - m.mpf("1e-3")), ("2pi+0.1", 2 * m.pi + m.mpf("0.1"))):
        th = m.mpf(th)
        out.append({"name": "exmap_pose/theta_" + name, "kind": "exmap_pose", "tags": ["pose_theta_" + name], "x": pose0,
                    "d": [0.1, -0.2, 0.3] + _f([th * x for x in ax]), "theta": float(th)})
    for name, half in (("0", 0), ("0.5", "0.25"),
                       ("below_eps", "2.0e-16"), ("above_eps", "2.4e-16"),
                       ("below_sqrt_eps", "1.48e-8"), ("above_sqrt_eps", "1.50e-8"),
                       ("below_root4_eps", "1.21e-4"), ("above_root4_eps", "1.23e-4")):
        th = 2 * m.mpf(half)
        out.append({"name": "exmap_plane/half_theta_" + name, "kind": "exmap_plane", "tags": ["plane_half_theta_" + name], "x": plane0,
                    "d": _f([th * x for x in ax]), "theta": float(th)})
    return out


def generate():
    return {"cases": [finish_case(c) for c in build_cases()], "exmaps": [finish_exmap(c) for c in build_exmaps()]}


ABOUT = ("written by `python -m oracle.mp_ref --write` (mpmath, 60 digits): inputs are doubles, r / J (the exact Jacobian) / J_cd (central "
         "differences of step 1e-4 in exact arithmetic) are rounded to double, u_* are conditioning units to three digits; `measured` "
         "(rho of the CPU oracle and the bound K per kind and quantity) is written by --measure")


def dump(fx, path=FIXTURE):
    with open(path, "w") as f:
        f.write("{\n \"about\": %s,\n \"dps\": 60,\n \"cases\": [\n" % json.dumps(ABOUT))
        f.write(",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in fx["cases"]))
        f.write("\n ],\n \"exmaps\": [\n")
        f.write(",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in fx["exmaps"]))
        f.write("\n ],\n \"measured\": %s\n}\n" % json.dumps(fx.get("measured", {}), indent=1, sort_keys=True))


def load(path=FIXTURE):
    with open(path) as f:
        return json.load(f)


# ---- what a double-precision implementation is measured with -------------------------------------------------------------------------
def case_group(c):
    """the kind a case is measured and bounded under (the name's first part: robust cases are kinds of their own)"""
    return c["name"].split("/")[0]


def ratios(c, r=None, J_analytic=None, J_numeric=None):
    """{quantity: max |got - reference| / unit} for what is given; numeric: unit u(J_cd) + u(r) / step, row by row"""
    import numpy as np
    out = {}
    if r is not None:
        out["r"] = float(np.max(np.abs(np.asarray(r) - c["r"]) / c["u_r"]))
    if J_analytic is not None:
        out["J_analytic"] = float(np.max(np.abs(np.asarray(J_analytic).ravel() - c["J"]) / c["u_J"]))
    if J_numeric is not None and c["numeric"]:
        ncol = len(c["J"]) // len(c["r"])
        unit = np.asarray(c["u_J_cd"]) + np.repeat(np.asarray(c["u_r"]) / CD_STEP, ncol)
        out["J_numeric"] = float(np.max(np.abs(np.asarray(J_numeric).ravel() - c["J_cd"]) / unit))
    return out


def exmap_ratio(c, got):
    """the pose retraction mirrors the reference's series term 0.5 + theta^2 / 48 below theta = 1e-4 (the true series has a minus sign):
    theta^3 / 24 of the quaternion is that term's, not round-off, and is taken off before the ratio"""
    import numpy as np
    err = np.abs(np.asarray(got) - c["out"])
    if c["kind"] == "exmap_pose" and c["theta"] < 1e-4:
        err = np.maximum(err - c["theta"] ** 3 / 24.0, 0.0)
    return float(np.max(err / c["u_out"]))


def bound(rho_max):
    return min(K_CAP, max(K_FLOOR, K_FACTOR * rho_max))


def _phi(kind, b, d):
    import numpy as np
    d = np.asarray(d, dtype=np.float64)
    if kind == COST_HUBER:
        rh = np.where(np.abs(d) < b, d * d, 2.0 * b * np.abs(d) - b * b)
    elif kind == COST_PSEUDO_HUBER:
        rh = 2.0 * d * d / (np.sqrt(1.0 + d * d / (b * b)) + 1.0)
    else:
        rh = np.log(np.pi / b) * np.log1p(d * d / (b * b))
    return np.where(d < 0, -1.0, 1.0) * np.sqrt(rh), rh


def _dphi(kind, b, d):
    import numpy as np
    d = np.asarray(d, dtype=np.float64)
    _, rh = _phi(kind, b, d)
    if kind == COST_HUBER:
        return np.where(np.abs(d) < b, 1.0, b / np.sqrt(np.maximum(rh, 1e-300)))
    if kind == COST_PSEUDO_HUBER:
        return np.abs(d) / (np.sqrt(1.0 + d * d / (b * b)) * np.sqrt(rh))
    return np.log(np.pi / b) * np.abs(d) / ((b * b + d * d) * np.sqrt(rh))


def oracle_eval(c):
    """the CPU oracle (oracle/pps_oracle.c) on one case: (r, J analytic, J numeric).  The oracle has no cost functions: for a robust case
    the chain rule (analytic) and the central differences through the cost (numeric) are taken here, in double precision, around its
    whitened residuals."""
    import numpy as np
    from oracle import oracle_py as O
    g = O.OracleGraph()
    types = KINDS[c["kind"]][0]
    ids = [g.add_pose(c["a"]) if types[0] == POSE else g.add_plane(c["a"])]
    if len(types) == 2:
        ids.append(g.add_pose(c["b"]) if types[1] == POSE else g.add_plane(c["b"]))
    kind = c["kind"]
    if kind == "plane_obs":
        f = g.add_plane_obs(ids[0], ids[1], c["meas"], c["ut"])
    elif kind == "plane_obs2":
        f = g.add_plane_obs2(ids[0], ids[1], c["meas"], c["ray"], c["ut"])
    elif kind == "plane_prior":
        f = g.add_plane_prior(ids[0], c["meas"], c["ut"])
    elif kind == "pose_prior":
        f = g.add_pose_prior(ids[0], c["meas"], c["ut"])
    else:
        f = g.add_odometry(ids[0], ids[1], c["meas"], c["ut"])
    Ja, r = g.factor_jacobian(f, analytic=1)
    Jn, _ = g.factor_jacobian(f, analytic=0)
    if not c.get("cost"):
        return r, Ja, Jn
    ck, cb = c["cost"]
    Ja = _dphi(ck, cb, r)[:, None] * Ja
    cols = []
    for n, t in enumerate(types):
        x0 = np.array(c["a"] if n == 0 else c["b"])
        for j in range(6 if t == POSE else 3):
            ys = []
            for s in (CD_STEP, -CD_STEP):
                d = np.zeros(6 if t == POSE else 3)
                d[j] = s
                if t == POSE:
                    g.set_pose(ids[n], O.pose_exmap(x0, d))
                else:
                    g.set_plane(ids[n], O.plane_exmap(x0, d))
                ys.append(_phi(ck, cb, g.factor_error(f, 1))[0])
            (g.set_pose if t == POSE else g.set_plane)(ids[n], x0)
            cols.append((ys[0] - ys[1]) / (CD_STEP + CD_STEP))
    return _phi(ck, cb, r)[0], Ja, np.array(cols).T


def oracle_exmap(c):
    from oracle import oracle_py as O
    return O.pose_exmap(c["x"], c["d"]) if c["kind"] == "exmap_pose" else O.plane_exmap(c["x"], c["d"])


def measure(fx):
    """rho of the CPU oracle per kind and quantity, the worst case's name, and K"""
    worst = {}
    for c in fx["cases"]:
        r, Ja, Jn = oracle_eval(c)
        analytic = None if c["kind"] == "plane_obs2" else Ja          # a re-popping observation has central differences in both modes
        for q, v in ratios(c, r, analytic, Jn).items():
            key = case_group(c) + "." + q
            if key not in worst or v > worst[key][0]:
                worst[key] = (v, c["name"])
    for c in fx["exmaps"]:
        v = exmap_ratio(c, oracle_exmap(c))
        key = c["kind"] + ".out"
        if key not in worst or v > worst[key][0]:
            worst[key] = (v, c["name"])
    out = {}
    for k, (v, n) in sorted(worst.items()):
        v = float("%.3g" % v)
        out[k] = {"rho_oracle": v, "worst_case": n, "K": float("%.3g" % bound(v))}
    return out


def main(argv):
    if "--write" in argv:
        fx = generate()
        if os.path.exists(FIXTURE):
            fx["measured"] = load().get("measured", {})
        dump(fx)
        print("wrote %d cases, %d retractions: %d bytes" % (len(fx["cases"]), len(fx["exmaps"]), os.path.getsize(FIXTURE)))
    if "--measure" in argv:
        fx = load()
        fx["measured"] = measure(fx)
        dump(fx)
        for k, v in fx["measured"].items():
            print("%-32s rho %-10g K %-6g %s" % (k, v["rho_oracle"], v["K"], v["worst_case"]))
    if "--write" not in argv and "--measure" not in argv:
        print(__doc__)


if __name__ == "__main__":
    main(sys.argv[1:])
