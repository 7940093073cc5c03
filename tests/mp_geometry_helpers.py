"""What tests/test_host_mp_geometry.py and tests/test_gpu_mp_geometry.py share: the arbitrary-precision fixture
(tests/golden/mp_geometry_cases.json, written by oracle/mp_ref.py), the case kinds it has to hold, and the comparison of one
double-precision result with it.  Nothing here needs mpmath."""
import numpy as np

from oracle import mp_ref as MP

# every tag the fixture must carry, per kind of factor (oracle/mp_ref.py: build_cases / build_exmaps)
_LOG = ["tilt_" + t for t in MP.TILTS] + ["tilt_zero", "meas_negated"] + ["near_pi_w_" + w for w in MP.NEAR_PI_W] + ["d_zero", "d_dominant"]
_EULER = ["ordinary"] + ["pitch_%s_%s" % (s, g) for s in ("plus", "minus") for g in MP.PITCH_GAPS] + \
         ["%s_wrap_%s" % (a, s) for a in ("yaw", "roll") for s in ("plus", "minus")]
_ROBUST = ["robust_%s_%s" % (c, t) for c in ("huber", "pseudo_huber", "cauchy") for t in ("0.5", "0.999", "1.001", "5")]
REQUIRED = {
    "plane_obs": _LOG + ["translation_1e3", "corridor", "whitening_3"],
    "plane_prior": _LOG,
    "plane_obs2": ["factor2_ordinary", "factor2_ray_near_parallel", "factor2_camera_height_1e-2"],
    "pose_prior": _EULER,
    "odometry": _EULER + ["r_to_quat_branch_0", "r_to_quat_branch_1", "r_to_quat_branch_2", "trace_near_zero", "identical_poses",
                          "translation_1e4", "whitening_6"],
    "robust_plane_obs": _ROBUST,
    "robust_odometry": _ROBUST,
    "exmap_pose": ["pose_theta_" + t for t in ("0", "1e-6", "0.9999e-4", "1.0001e-4", "0.5", "pi-1e-3", "2pi+0.1")],
    "exmap_plane": ["plane_half_theta_" + t for t in ("0", "0.5", "below_eps", "above_eps", "below_sqrt_eps", "above_sqrt_eps",
                                                      "below_root4_eps", "above_root4_eps")],
}
# the only cases a central difference of step 1e-4 may not be compared on: it would straddle the double cover or the gimbal
ANALYTIC_ONLY = {"near_pi_w_1e-6", "near_pi_w_-1e-6", "near_pi_w_1e-9", "near_pi_w_-1e-9",
                 "pitch_plus_1e-4", "pitch_plus_1e-6", "pitch_minus_1e-4", "pitch_minus_1e-6"}


def load():
    return MP.load()


def present_tags(fx):
    out = {}
    for c in fx["cases"] + fx["exmaps"]:
        out.setdefault(MP.case_group(c), set()).update(c["tags"])
    return out


def K_of(fx, c, quantity):
    return fx["measured"]["%s.%s" % (MP.case_group(c), quantity)]["K"]


def check_case(fx, c, r, J_analytic, J_numeric, worst, who, say=None):
    """assert |got - reference| <= K unit for every quantity given; worst[kind.quantity] collects the largest ratio seen"""
    got = MP.ratios(c, r, J_analytic, J_numeric)
    for q, v in got.items():
        key = "%s.%s" % (MP.case_group(c), q)
        worst[key] = max(worst.get(key, 0.0), v)
        assert v <= K_of(fx, c, q), "%s: %s of %s is %.3g units off, bound K = %g" % (who, q, c["name"], v, K_of(fx, c, q))
    if say:
        say("%-48s %s" % (c["name"], "  ".join("%s %.3g" % kv for kv in got.items())))
    return got


def check_exmap(fx, c, got, worst, who):
    v = MP.exmap_ratio(c, got)
    key = c["kind"] + ".out"
    worst[key] = max(worst.get(key, 0.0), v)
    assert v <= K_of(fx, c, "out"), "%s: %s is %.3g units off, bound K = %g" % (who, c["name"], v, K_of(fx, c, "out"))
    return v


def structural_zeros(c, J):
    """angle rows against translation columns of a pose factor: nothing on that path is rounded, the entries are 0 exactly"""
    J = np.asarray(J)
    if c["kind"] == "odometry":
        return bool(np.all(J[3:, 0:3] == 0.0) and np.all(J[3:, 6:9] == 0.0))
    if c["kind"] == "pose_prior":
        return bool(np.all(J[3:, 0:3] == 0.0))
    return True


def table(worst, fx):
    rows = ["%-30s %-12s %-12s %s" % ("kind.quantity", "rho", "rho(oracle)", "K")]
    for k in sorted(worst):
        rows.append("%-30s %-12.3g %-12.3g %g" % (k, worst[k], fx["measured"][k]["rho_oracle"], fx["measured"][k]["K"]))
    return "\n".join(rows)
