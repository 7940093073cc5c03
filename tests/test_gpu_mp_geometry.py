"""GPU: residuals, retractions and Jacobians of the device against the arbitrary-precision statement of oracle/mp_ref.py.

Reads tests/golden/mp_geometry_cases.json only (no mpmath here).  Every case is one factor on one or two nodes of its own, all in ONE
graph; pps_eval_factor in JAC_NUMERIC and JAC_ANALYTIC, in the lane form and the thread-per-factor form of K1; the re-popping
observations through k_linearize_repop; the robust cases on graphs of their own after set_cost_function; pps_debug_exmap for the
retractions.  Bounds, in conditioning units u (the fixture's, fixed by the statement alone) and K = max(8, 4 rho of the CPU oracle) <= 256
(the fixture's "measured" block -- never taken from the device or from a host build of the shipped headers):
    |r - r*| <= K u(r)      |J_analytic - J*| <= K u(J*)      |J_numeric - J_cd| <= K (u(J_cd) + u(r) / 1e-4)      |exmap - exmap*| <= K u
    chi2() = sum |r*|^2 to sum 2 |r*| u(r)
and the angle rows of a pose factor against its translation columns are exactly 0.  `pytest -s` prints the device's worst ratio per
kind and quantity (profiles/mp_geometry_device_rho.txt is one such run)."""
import numpy as np
import pytest

import mp_geometry_helpers as H
import pop_up_slam_amd as P
from oracle import mp_ref as MP

pytestmark = pytest.mark.gpu

K1_FORMS = ["lanes", "threads"]
COSTS = {MP.COST_HUBER: "huber", MP.COST_PSEUDO_HUBER: "pseudo_huber", MP.COST_CAUCHY: "cauchy"}


@pytest.fixture(scope="module")
def fx():
    return H.load()


def _form(monkeypatch, form):
    if form == "threads":
        monkeypatch.setenv("PPS_K1_THREAD_FORM", "1")
    else:
        monkeypatch.delenv("PPS_K1_THREAD_FORM", raising=False)


def _add(g, c):
    """the case's own nodes and its factor -> factor id"""
    kind = c["kind"]
    if kind == "plane_prior":
        return g.add_plane_prior(g.add_plane(c["a"]), c["meas"], c["ut"])
    if kind == "pose_prior":
        return g.add_pose_prior(g.add_pose(c["a"]), c["meas"], c["ut"])
    if kind == "odometry":
        return g.add_odometry(g.add_pose(c["a"]), g.add_pose(c["b"]), c["meas"], c["ut"])
    if kind == "plane_obs":
        return g.add_plane_obs(g.add_pose(c["a"]), g.add_plane(c["b"]), c["meas"], c["ut"])
    return g.add_plane_obs2(g.add_pose(c["a"]), g.add_plane(c["b"]), c["meas"], c["ray"], c["ut"])


def _check_graph(fx, g, cases, fids, worst, who):
    want = sum(float(np.sum(np.square(c["r"]))) for c in cases)
    tol = sum(float(np.sum(2.0 * np.abs(c["r"]) * np.array(c["u_r"]))) for c in cases)
    got = g.chi2()
    print("%s: chi2 %.17g, statement %.17g, difference %.3g, allowed %.3g" % (who, got, want, got - want, tol))
    assert abs(got - want) <= tol, (who, got, want, tol)
    for c, f in zip(cases, fids):
        Jn, r0 = g.eval_factor(f, P.JAC_NUMERIC)
        Ja, r1 = g.eval_factor(f, P.JAC_ANALYTIC)
        repop = c["kind"] == "plane_obs2"                    # central differences in both modes: the measurement moves with the pose
        H.check_case(fx, c, r0, None, Jn, worst, who + " JAC_NUMERIC")
        H.check_case(fx, c, r1, None if repop else Ja, Ja if repop else None, worst, who + " JAC_ANALYTIC")
        if not c["cost"]:
            assert H.structural_zeros(c, Ja), (who, c["name"])
        if "tilt_zero" in c["tags"]:
            assert np.all(r0 == 0.0) and np.all(r1 == 0.0), (who, c["name"])


@pytest.mark.parametrize("form", K1_FORMS)
def test_factors_against_the_statement(built, monkeypatch, fx, form):
    _form(monkeypatch, form)
    have = H.present_tags(fx)
    for kind, tags in H.REQUIRED.items():
        assert not [t for t in tags if t not in have.get(kind, ())], kind
    worst = {}
    plain = [c for c in fx["cases"] if not c["cost"]]
    g = P.Graph()
    fids = [_add(g, c) for c in plain]
    assert g.num_nodes() > 100 and sum(c["kind"] == "plane_obs2" for c in plain) == 3
    _check_graph(fx, g, plain, fids, worst, form)
    for kind, name in COSTS.items():
        rob = [c for c in fx["cases"] if c["cost"] and c["cost"][0] == kind]
        assert len(rob) == 8 and all(c["cost"][1] == 1.0 for c in rob)
        g = P.Graph()
        fids = [_add(g, c) for c in rob]
        g.set_cost_function(kind, 1.0)
        _check_graph(fx, g, rob, fids, worst, "%s %s" % (form, name))
    assert set(worst) == set(fx["measured"]) - {"exmap_pose.out", "exmap_plane.out"}
    print("\ndevice (%s form) against the 60-digit statement, worst ratio per kind and quantity\n%s" % (form, H.table(worst, fx)))


def test_retractions_against_the_statement(built, fx):
    worst = {}
    for kind, code in (("exmap_pose", 0), ("exmap_plane", 1)):
        cs = [c for c in fx["exmaps"] if c["kind"] == kind]
        got = P.debug_exmap(code, np.array([c["x"] for c in cs]), np.array([c["d"] for c in cs]))
        for k, c in enumerate(cs):
            H.check_exmap(fx, c, got[k], worst, "device")
    print("\ndevice retractions against the 60-digit statement\n" + H.table(worst, fx))
