"""The yardstick of the robust cost functions (Slam::set_cost_function): a numpy restatement on top of oracle/numpy_ref.py.

Factor::error (isam/Factor.h:67-77) replaces every whitened component by sign(r) sqrt(rho(r)), sign(0) = +1, in every evaluation: the
central differences (eps = 1e-4 through the exmaps), weighted_errors and chi2.  RobustGraph overrides numpy_ref.Graph.error with exactly
that; factor_jacobian, chi2, the Gauss-Newton step and levenberg_marquardt (the constants of Properties.h) are inherited unchanged.
rho restates isam/robust.h; pseudo-Huber and Cauchy are written in their cancellation-free forms (the same functions).
analytic=True restates JAC_ANALYTIC: the chain rule, row i of the squared error's Jacobian scaled by phi'(r_i) -- NOT the central
differences through phi, whose O(eps^2) truncation grows with (eps |J| / b)^2 and passes 2e-5 once b is within two decades of the step."""
import numpy as np

from oracle import numpy_ref as NR

NONE, HUBER, PSEUDO_HUBER, CAUCHY = range(4)


def rho(kind, b, d):
    d = np.asarray(d, dtype=np.float64)
    if kind == HUBER:
        return np.where(np.abs(d) < b, d * d, 2.0 * b * np.abs(d) - b * b)
    if kind == PSEUDO_HUBER:                     # 2 b^2 (sqrt(1 + d^2 / b^2) - 1)
        return 2.0 * d * d / (np.sqrt(1.0 + d * d / (b * b)) + 1.0)
    if kind == CAUCHY:                           # log(pi / b) * log(1 + d^2 / b^2): a product, as the reference writes it
        return np.log(np.pi / b) * np.log1p(d * d / (b * b))
    return d * d


def phi(kind, b, d):
    d = np.asarray(d, dtype=np.float64)
    return np.where(d < 0, -1.0, 1.0) * np.sqrt(rho(kind, b, d))


def dphi(kind, b, d):
    """phi' = rho' / (2 sqrt(rho)) taken with the sign of d; at d = 0 the limit"""
    d = np.asarray(d, dtype=np.float64)
    r = rho(kind, b, d)
    with np.errstate(divide="ignore", invalid="ignore"):
        if kind == HUBER:
            return np.where(np.abs(d) < b, 1.0, b / np.sqrt(r))
        if kind == PSEUDO_HUBER:
            return np.where(r > 0, np.abs(d) / (np.sqrt(1.0 + d * d / (b * b)) * np.sqrt(r)), 1.0)
        if kind == CAUCHY:
            k = np.log(np.pi / b)
            return np.where(r > 0, k * np.abs(d) / ((b * b + d * d) * np.sqrt(r)), np.sqrt(k) / b)
    return np.ones_like(d)


def repop_wall_plane(pose, ray6):
    """isam::get_wall_plane_equation (src/isam_plane3d.cpp:20-55) restated: the ground plane (0, 0, -1, 0) in the sensor frame, the two
    ground rays cut with it, the wall through the two points and perpendicular to the ground; a unit 4-vector"""
    from scipy.spatial.transform import Rotation as Rot
    R = Rot.from_quat(pose[3:]).as_matrix()
    gn = R.T @ np.array([0.0, 0.0, -1.0]); gd = -pose[2]
    pts = [(-gd / (gn @ ray6[3 * j:3 * j + 3])) * ray6[3 * j:3 * j + 3] for j in range(2)]
    n = np.cross(pts[1] - pts[0], gn)
    out = np.concatenate([n, [-(n @ pts[0])]])
    return out / np.linalg.norm(out)


class OpsSpec:
    """the op list of tests/test_gpu_factor2.py (_mixed_graph) as the spec numpy_ref.Graph reads, + rays {factor index: ray6}"""

    def __init__(self, ops):
        nt, ni, ft, fn, fm, fw, self.rays = [], [], [], [], [], [], {}
        for op in ops:
            kind = op[0]
            if kind in ("pose", "plane"):
                v = np.zeros(7); v[:len(op[1])] = op[1]
                nt.append(0 if kind == "pose" else 1); ni.append(v)
                continue
            m, w = np.zeros(6), np.zeros(21)
            meas, ut = (op[-2], op[-1]) if kind != "obs2" else (op[3], op[5])
            m[:len(meas)] = meas; w[:len(ut)] = ut
            if kind == "obs2":
                self.rays[len(ft)] = np.asarray(op[4], dtype=np.float64)
            ft.append({"pp": NR.F_POSE_PRIOR, "odo": NR.F_ODOMETRY, "obs": NR.F_PLANE_OBS, "obs2": NR.F_PLANE_OBS, "lp": NR.F_PLANE_PRIOR}[kind])
            fn.append((op[1], op[2]) if kind in ("odo", "obs", "obs2") else (op[1], -1))
            fm.append(m); fw.append(w)
        self.node_type = np.array(nt, dtype=np.int32); self.node_init = np.array(ni)
        self.f_type = np.array(ft, dtype=np.int32); self.f_nodes = np.array(fn, dtype=np.int32)
        self.f_meas = np.array(fm); self.f_sqrtinf = np.array(fw)


class RobustGraph(NR.Graph):
    def __init__(self, spec, kind=NONE, b=1.0, analytic=False):
        super().__init__(spec)
        self.kind, self.b, self.analytic = kind, b, analytic
        self.rays = dict(getattr(spec, "rays", {}))

    def factor_jacobian(self, k, x):
        if not self.analytic or self.kind == NONE:
            return super().factor_jacobian(k, x)
        kind, self.kind = self.kind, NONE
        try:
            Hs, rs = super().factor_jacobian(k, x)          # the squared error's central differences (what JAC_ANALYTIC is held to, 2e-5)
        finally:
            self.kind = kind
        return dphi(kind, self.b, rs)[:, None] * Hs, phi(kind, self.b, rs)

    def basic_error(self, k, x):
        """+ Pose3d_Plane3d_Factor2 (rays: factor index -> the edge's two ground rays): the measured plane is re-popped at the pose"""
        ray = getattr(self, "rays", {}).get(k)
        if ray is None:
            return super().basic_error(k, x)
        a, b = self.f_nodes[k]
        return NR.res_plane_obs(x[a], x[b], repop_wall_plane(x[a], ray))

    def error(self, k, x):
        e = super().error(k, x)
        return e if self.kind == NONE else phi(self.kind, self.b, e)

    def whitened(self, k, x):
        """the whitened residual before the cost function"""
        return NR.Graph.error(self, k, x)

    def state_error(self, other_x):
        """(largest pose translation error, largest plane error up to sign) against another state list"""
        ep = el = 0.0
        for i, t in enumerate(self.node_type):
            a, o = np.asarray(self.x[i]), np.asarray(other_x[i])
            if t == 0:
                ep = max(ep, float(np.linalg.norm(a[:3] - o[:3])))
            else:
                el = max(el, float(min(np.abs(a - o).max(), np.abs(a + o).max())))
        return ep, el


def corrupt_one_observation(spec, which=7, tilt=0.9, shift=2.5):
    """ONE plane observation's measurement replaced by a grossly wrong plane: the normal tilted by `tilt` rad, the distance moved by `shift`"""
    ks = [k for k, t in enumerate(spec.f_type) if t == NR.F_PLANE_OBS]
    k = ks[which % len(ks)]
    m = spec.f_meas[k, :4].copy()
    n = m[:3] / np.linalg.norm(m[:3])
    ax = np.cross(n, [1.0, 0.0, 0.0]) if abs(n[0]) < 0.9 else np.cross(n, [0.0, 1.0, 0.0])
    ax /= np.linalg.norm(ax)
    n2 = n * np.cos(tilt) + np.cross(ax, n) * np.sin(tilt) + ax * (ax @ n) * (1 - np.cos(tilt))
    out = spec.f_meas.copy()
    out[k, :4] = np.concatenate([n2, [m[3] / np.linalg.norm(m[:3]) + shift]])
    import copy
    s2 = copy.copy(spec)
    s2.f_meas = out
    return s2, k
