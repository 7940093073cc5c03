"""Residuals, retractions and Jacobians against an arbitrary-precision statement (oracle/mp_ref.py, mpmath at 60 digits) -- on the host.

tests/golden/mp_geometry_cases.json holds, per case, the inputs as doubles, the exact whitened residual r*, the exact Jacobian J* with
respect to the retraction's tangent, the central differences J_cd of step 1e-4 in exact arithmetic, and the conditioning unit u of each:
the error a double-precision algorithm is entitled to from rounded inputs and a rounded output.  Held to it here, in units of u:
  the CPU oracle (oracle/pps_oracle.c) -- its worst ratio rho per kind and quantity is the fixture's "measured" block, and fixes
      K = max(8, 4 rho) <= 256, the bound of everything else (tests/test_gpu_mp_geometry.py holds the device to the same K);
  oracle/numpy_ref.py (scipy rotations);
  a host build of the shipped headers csrc/pps_lin.h / pps_geom.h / pps_cost.h (tests/cpp/mp_geom_host.cpp, no multiply-add contraction):
      lin_*<0>, lin_*<1>, their ROBUST forms and the two retractions.  `pytest -s` prints its ratio per case.
A closed-form Jacobian that is off by 1e-9 of an entry -- a wrong small-angle branch of dlog_dq, a sign in jac_odometry -- is 1e6 units off."""
import ctypes as C
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import mp_geometry_helpers as H
from oracle import mp_ref as MP
from oracle import numpy_ref as NR
from oracle import oracle_py as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp = C.POINTER(C.c_double)
_KIND = {"plane_obs": 0, "odometry": 1, "pose_prior": 2, "plane_prior": 3, "plane_obs2": 4}
_SHAPE = {"plane_obs": (3, (6, 3)), "plane_obs2": (3, (6, 3)), "odometry": (6, (6, 6)), "pose_prior": (6, (6,)), "plane_prior": (3, (3,))}


@pytest.fixture(scope="module")
def fx():
    return H.load()


@pytest.fixture(scope="module")
def host():
    src = os.path.join(ROOT, "tests", "cpp", "mp_geom_host.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "libmp_geom_host.so")
    deps = [src] + [os.path.join(ROOT, "pop_up_slam_amd", "csrc", h) for h in ("pps_lin.h", "pps_geom.h", "pps_cost.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-ffp-contract=off",
                               "-I" + os.path.join(ROOT, "pop_up_slam_amd", "csrc"), src, "-o", out])
    lib = C.CDLL(out)
    lib.mp_geom_eval.restype = None
    lib.mp_geom_eval.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double] + [_dp] * 6
    lib.mp_geom_exmap.restype = None
    lib.mp_geom_exmap.argtypes = [C.c_int] + [_dp] * 3
    lib.mp_geom_repop_wall_plane.restype = None
    lib.mp_geom_repop_wall_plane.argtypes = [_dp] * 3
    return lib


def _arr(v, n):
    a = np.zeros(n)
    if v is not None:
        a[:len(v)] = v
    return a


def _host_eval(lib, c, mode):
    """(J m x cols, r) of one case from the host build, laid out as pps_eval_factor returns it"""
    m, dims = _SHAPE[c["kind"]]
    a, b, ms, w, ray = _arr(c["a"], 7), _arr(c["b"], 7), _arr(c["meas"], 6), _arr(c["ut"], 21), _arr(c["ray"], 6)
    out = np.zeros(m * sum(dims) + m)
    cost = c["cost"] or [0, 1.0]
    lib.mp_geom_eval(_KIND[c["kind"]], mode, int(cost[0]), float(cost[1]), *[x.ctypes.data_as(_dp) for x in (a, b, ms, w, ray, out)])
    blocks, k = [], 0
    for d in dims:
        blocks.append(out[k:k + m * d].reshape(m, d))
        k += m * d
    return np.hstack(blocks), out[k:k + m].copy()


def test_fixture_holds_every_case_kind(fx):
    have = H.present_tags(fx)
    for kind, tags in H.REQUIRED.items():
        assert kind in have, kind
        missing = [t for t in tags if t not in have[kind]]
        assert not missing, (kind, missing)
    for c in fx["cases"]:
        if not c["numeric"]:
            assert set(c["tags"]) & H.ANALYTIC_ONLY, c["name"]                 # every other case is compared in both modes
        assert (c["J_cd"] is not None) == c["numeric"]
        assert H.structural_zeros(c, np.reshape(c["J"], (len(c["r"]), -1))), c["name"]
    assert os.path.getsize(MP.FIXTURE) < 500_000
    # each kind and quantity has its measured rho and its bound; no bound above the cap
    for key, v in fx["measured"].items():
        assert v["K"] == float("%.3g" % MP.bound(v["rho_oracle"])) and 8.0 <= v["K"] <= 256.0, key
    want = {"%s.%s" % (MP.case_group(c), q) for c in fx["cases"] for q in ("r", "J_analytic", "J_numeric")} - {"plane_obs2.J_analytic"}
    assert set(fx["measured"]) == want | {"exmap_pose.out", "exmap_plane.out"}


def test_fixture_regenerates_bit_for_bit(fx):
    """every committed double is what the 60-digit statement rounds to: inputs, references and units"""
    try:
        import mpmath  # noqa: F401
    except ImportError:
        pytest.skip("mpmath is not installed: the committed fixture cannot be regenerated here")
    new = MP.generate()
    for part in ("cases", "exmaps"):
        assert [c["name"] for c in new[part]] == [c["name"] for c in fx[part]]
        for a, b in zip(new[part], fx[part]):
            assert a.keys() == b.keys(), a["name"]
            for k in a:
                va, vb = a[k], b[k]
                if isinstance(va, list) and va and isinstance(va[0], float):
                    assert np.array(va).tobytes() == np.array(vb, dtype=np.float64).tobytes(), (a["name"], k)
                else:
                    assert va == vb, (a["name"], k)


def test_cpu_oracle_within_its_measured_ratios(fx):
    """factor_jacobian in both modes, factor_error, ora_pose_exmap, ora_plane_exmap, repop_wall_plane: inside K = max(8, 4 rho) of the
    rho the generator's --measure recorded -- and that record is what the oracle gives (to the 30 % another libm may move a ratio)"""
    worst = {}
    for c in fx["cases"]:
        r, Ja, Jn = MP.oracle_eval(c)
        H.check_case(fx, c, r, None if c["kind"] == "plane_obs2" else Ja, Jn, worst, "oracle")
        if c["kind"] in ("odometry", "pose_prior") and not c["cost"]:
            assert H.structural_zeros(c, Ja), c["name"]
        if c["kind"] == "plane_obs2":
            got = O.repop_wall_plane(c["a"], c["ray"])
            ref = np.array(c["wall"])
            err = np.minimum(np.abs(got - ref), np.abs(got + ref))
            assert np.all(err <= H.K_of(fx, c, "r") * np.array(c["u_wall"])), c["name"]
    for c in fx["exmaps"]:
        H.check_exmap(fx, c, MP.oracle_exmap(c), worst, "oracle")
    for key, v in fx["measured"].items():
        assert worst[key] <= max(1.3 * v["rho_oracle"], v["rho_oracle"] + 0.5), (key, worst[key], v)
        if v["K"] > MP.K_FLOOR:                              # a bound above the floor has to be earned by the oracle, today
            assert worst[key] >= 0.7 * v["rho_oracle"], (key, worst[key], v)
    print("\nCPU oracle against the 60-digit statement, worst ratio per kind and quantity\n" + H.table(worst, fx))


def test_oracle_factor_error_equals_the_residual(fx):
    for c in fx["cases"]:
        if c["cost"]:
            continue
        g = O.OracleGraph()
        if c["kind"] == "plane_prior":
            f = g.add_plane_prior(g.add_plane(c["a"]), c["meas"], c["ut"])
        elif c["kind"] == "pose_prior":
            f = g.add_pose_prior(g.add_pose(c["a"]), c["meas"], c["ut"])
        elif c["kind"] == "odometry":
            f = g.add_odometry(g.add_pose(c["a"]), g.add_pose(c["b"]), c["meas"], c["ut"])
        elif c["kind"] == "plane_obs":
            f = g.add_plane_obs(g.add_pose(c["a"]), g.add_plane(c["b"]), c["meas"], c["ut"])
        else:
            f = g.add_plane_obs2(g.add_pose(c["a"]), g.add_plane(c["b"]), c["meas"], c["ray"], c["ut"])
        r = g.factor_error(f, 1)
        assert np.all(np.abs(r - c["r"]) <= H.K_of(fx, c, "r") * np.array(c["u_r"])), c["name"]
        chi = float(np.sum(np.square(c["r"])))
        assert abs(g.chi2() - chi) <= H.K_of(fx, c, "r") * float(np.sum(2 * np.abs(c["r"]) * c["u_r"])) + 4e-16 * chi, c["name"]


def _numpy_ref_graph(c):
    types = MP.KINDS[c["kind"]][0]
    node_init = np.zeros((len(types), 7))
    node_init[0, :len(c["a"])] = c["a"]
    if len(types) == 2:
        node_init[1, :len(c["b"])] = c["b"]
    ft = {"pose_prior": NR.F_POSE_PRIOR, "odometry": NR.F_ODOMETRY, "plane_obs": NR.F_PLANE_OBS, "plane_prior": NR.F_PLANE_PRIOR}[c["kind"]]
    spec = SimpleNamespace(node_type=np.array([0 if t == MP.POSE else 1 for t in types], dtype=np.int32), node_init=node_init,
                           f_type=np.array([ft], dtype=np.int32), f_nodes=np.array([[0, 1 if len(types) == 2 else -1]], dtype=np.int32),
                           f_meas=_arr(c["meas"], 6)[None, :], f_sqrtinf=_arr(c["ut"], 21)[None, :])
    return NR.Graph(spec)


def test_numpy_ref_against_the_statement(fx):
    """oracle/numpy_ref.py -- scipy's Rotation for every rotation, Euler angle and logarithm -- is the other restatement the fixtures of
    this suite come from: its residuals and its central differences, every case it has a factor for (no cost functions, no re-popping)"""
    worst = {}
    for c in fx["cases"]:
        if c["cost"] or c["kind"] == "plane_obs2":
            continue
        g = _numpy_ref_graph(c)
        Jn, r = g.factor_jacobian(0, g.x)
        H.check_case(fx, c, r, None, Jn, worst, "numpy_ref")
    print("\noracle/numpy_ref.py against the 60-digit statement\n" + H.table(worst, fx))


def test_host_build_of_the_shipped_headers(fx, host):
    """lin_*<0> against J_cd, lin_*<1> against J*, the residual of both against r*, plain and ROBUST, the re-popping loop, the retractions"""
    worst, lines = {}, []
    for c in fx["cases"]:
        Jn, r0 = _host_eval(host, c, 0)
        Ja, r1 = _host_eval(host, c, 1)
        repop = c["kind"] == "plane_obs2"
        H.check_case(fx, c, r0, None, Jn, worst, "host MODE 0", lines.append)
        H.check_case(fx, c, r1, None if repop else Ja, Ja if repop else None, worst, "host MODE 1", lines.append)
        if not c["cost"]:
            assert H.structural_zeros(c, Ja) and H.structural_zeros(c, Jn), c["name"]
        if repop:
            got = np.zeros(4)
            host.mp_geom_repop_wall_plane(_arr(c["a"], 7).ctypes.data_as(_dp), _arr(c["ray"], 6).ctypes.data_as(_dp), got.ctypes.data_as(_dp))
            ref = np.array(c["wall"])
            assert np.all(np.minimum(np.abs(got - ref), np.abs(got + ref)) <= H.K_of(fx, c, "r") * np.array(c["u_wall"])), c["name"]
    for c in fx["exmaps"]:
        got = np.zeros(len(c["x"]))
        host.mp_geom_exmap(0 if c["kind"] == "exmap_pose" else 1, _arr(c["x"], len(c["x"])).ctypes.data_as(_dp),
                           _arr(c["d"], len(c["d"])).ctypes.data_as(_dp), got.ctypes.data_as(_dp))
        v = H.check_exmap(fx, c, got, worst, "host")
        lines.append("%-48s out %.3g" % (c["name"], v))
    # the zero tilt really is one: dq = (0, 0, 0, 1), residual exactly 0
    for c in fx["cases"]:
        if "tilt_zero" in c["tags"]:
            assert np.all(_host_eval(host, c, 1)[1] == 0.0) and np.all(np.array(c["r"]) == 0.0)
    print("\nhost build of csrc/pps_lin.h, ratio per case (MODE 0 line, then MODE 1 line)\n" + "\n".join(lines))
    print("\nhost build, worst ratio per kind and quantity\n" + H.table(worst, fx))
