"""CPU: robust cost functions (pps_set_cost_function) before any kernel runs.

(1) csrc/pps_cost.h compiled with g++ (tests/cpp/cost_host.cpp) against the numpy rho / phi / phi' of tests/robust_helpers.py;
(2) the argument checks and refusals of the C ABI that need no device;
(3) the benefit, by the numpy restatement alone: ONE grossly wrong plane observation in small_20p_6l."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pop_up_slam_amd as P
import robust_helpers as RH
from helpers import load_fixture
from pop_up_slam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = [RH.HUBER, RH.PSEUDO_HUBER, RH.CAUCHY]


@pytest.fixture(scope="module")
def cost_lib(tmp_path_factory):
    so = tmp_path_factory.mktemp("cost") / "libcosthost.so"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "pop_up_slam_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "cost_host.cpp"), "-o", str(so)])
    lib = C.CDLL(str(so))
    for f in (lib.cost_host_rho, lib.cost_host_phi, lib.cost_host_dphi):
        f.argtypes = [C.c_int, C.c_double, C.c_double]; f.restype = C.c_double
    lib.cost_host_robustify3.argtypes = [C.c_int, C.c_double, C.POINTER(C.c_double)]
    return lib


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("b", [0.3, 1.0, 2.5])
def test_cost_header_against_numpy(cost_lib, kind, b):
    """rho, phi, phi' over |d| = 1e-12 .. 1e3 on both signs, both sides of Huber's kink and exactly at +-b, d = 0 and d = -0.0.
    Bound: 4 ulp-sized relative steps (both sides evaluate the same few correctly rounded operations; libm's log1p may differ in the last bit)."""
    mags = np.concatenate([np.logspace(-12, 3, 61), [b, np.nextafter(b, 0), np.nextafter(b, 10), 0.5 * b, 2 * b]])
    ds = np.concatenate([mags, -mags, [0.0, -0.0]])
    for d in ds:
        for name, ref in (("rho", RH.rho), ("phi", RH.phi), ("dphi", RH.dphi)):
            got = getattr(cost_lib, "cost_host_" + name)(kind, b, float(d))
            want = float(ref(kind, b, d))
            assert abs(got - want) <= 1e-15 * abs(want), (name, kind, b, d, got, want)
    # sign(0) = sign(-0.0) = +1: phi is +0.0 at both
    for z in (0.0, -0.0):
        v = cost_lib.cost_host_phi(kind, b, z)
        assert v == 0.0 and np.copysign(1.0, v) == 1.0
    # phi' at 0: the stated limits
    lim = 1.0 if kind != RH.CAUCHY else np.sqrt(np.log(np.pi / b)) / b
    assert abs(cost_lib.cost_host_dphi(kind, b, 0.0) - lim) <= 1e-15 * lim
    assert abs(cost_lib.cost_host_dphi(kind, b, 1e-200) - lim) <= 1e-15 * lim          # d^2 underflows: still the limit
    # phi' against a central difference of phi away from the kink
    for d in (0.37 * b, -0.37 * b, 3.1 * b, -3.1 * b):
        h = 1e-6 * b
        fd = (cost_lib.cost_host_phi(kind, b, d + h) - cost_lib.cost_host_phi(kind, b, d - h)) / (2 * h)
        assert abs(cost_lib.cost_host_dphi(kind, b, d) - fd) <= 1e-8 * max(1.0, abs(fd))
    r = (C.c_double * 3)(0.5 * b, -4.0 * b, -0.0)
    cost_lib.cost_host_robustify3(kind, b, r)
    np.testing.assert_allclose(list(r), RH.phi(kind, b, [0.5 * b, -4.0 * b, -0.0]), rtol=1e-15, atol=0)


def test_huber_is_continuous_at_the_kink(cost_lib):
    b = 0.7
    for s in (1.0, -1.0):
        lo, at, hi = (cost_lib.cost_host_phi(RH.HUBER, b, s * v) for v in (np.nextafter(b, 0), b, np.nextafter(b, 10)))
        assert abs(lo - at) <= 4e-16 and abs(hi - at) <= 4e-16 and abs(abs(at) - b) <= 4e-16


def test_symbols_argument_checks_and_get_after_set(built):
    lib = P.lib()
    with open(os.path.join(ROOT, "include", "pps.h")) as f:
        hdr = f.read()
    for name in ("pps_set_cost_function", "pps_get_cost_function"):
        assert name in hdr and name in P.SYMBOLS and getattr(lib, name) is not None
    assert "PPS_VERSION 30" in hdr and lib.pps_version() == P.PPS_VERSION               # not bumped
    assert lib.pps_set_cost_function(None, P.COST_HUBER, 1.0) == P.PPS_EINVAL
    k = C.c_int(); b = C.c_double()
    assert lib.pps_get_cost_function(None, C.byref(k), C.byref(b)) == P.PPS_EINVAL
    g = P.Graph()
    assert g.cost_function() == (P.COST_NONE, 1.0)
    bad = [(4, 1.0), (-1, 1.0), (P.COST_HUBER, 0.0), (P.COST_HUBER, -1.0), (P.COST_PSEUDO_HUBER, float("nan")), (P.COST_PSEUDO_HUBER, float("inf")),
           (P.COST_CAUCHY, np.pi), (P.COST_CAUCHY, 4.0), (P.COST_CAUCHY, 0.0)]
    for kind, bb in bad:
        with pytest.raises(P.PpsError) as e:
            g.set_cost_function(kind, bb)
        assert e.value.code == P.PPS_EINVAL, (kind, bb)
        assert g.cost_function() == (P.COST_NONE, 1.0)                                    # a refused call changes nothing
    for kind, bb in [(P.COST_HUBER, 0.5), (P.COST_PSEUDO_HUBER, 2.0), (P.COST_CAUCHY, 3.0), (P.COST_CAUCHY, np.nextafter(np.pi, 0))]:
        g.set_cost_function(kind, bb)
        assert g.cost_function() == (kind, bb)
    g.set_cost_function(P.COST_NONE, -5.0)                                                # b is ignored for NONE
    assert g.cost_function() == (P.COST_NONE, 1.0)
    g.close()


def test_refusals_while_a_cost_is_set_need_no_device(built):
    spec = synth.small_world(5, 3)
    g = P.Graph(); nid, _ = spec.replay(g)
    g.set_cost_function(P.COST_PSEUDO_HUBER, 1.0)
    with pytest.raises(P.PpsError) as e:
        P.Multi([g])
    assert e.value.code == P.PPS_ESTATE and "cost function" in str(e.value)
    pose = int([i for i, t in zip(nid, spec.node_type) if t == synth.NODE_POSE][0])
    with pytest.raises(P.PpsError) as e:
        g.assoc_gate(pose, np.array([[0.0, 0.0, -1.0, 1.0]]), np.array([synth._ut_diag([1.0] * 3)]))
    assert e.value.code == P.PPS_ESTATE and "cost function" in str(e.value)
    assert g.num_nodes() == len(nid)                                                      # the handle stays usable
    g.set_cost_function(P.COST_NONE)
    m = P.Multi([g]); m.close()                                                           # ... and NONE lifts the refusal
    g.close()


def test_one_gross_outlier_pulls_squared_lm_farther_than_pseudo_huber_lm():
    """small_20p_6l with ONE plane observation replaced by a plane tilted by 0.9 rad and moved by 2.5 (tests/robust_helpers.py:
    corrupt_one_observation), solved by the restatement's dense LM; errors against the uncorrupted graph's solution.
    Measured: squared LM ends 2.76e-2 (largest pose translation error) / 1.24e-2 (largest plane error) away, pseudo-Huber LM with
    b = 0.01 (inlier whitened residuals: median 4.6e-4, largest 2.9e-3; the outlier: 3.4e-2) 1.10e-2 / 4.1e-3.  Asserted with a factor 2."""
    fx, spec = load_fixture("small_20p_6l")
    clean = RH.RobustGraph(spec); clean.levenberg_marquardt()
    bad, k = RH.corrupt_one_observation(spec)
    sq = RH.RobustGraph(bad); sq.levenberg_marquardt()
    ph = RH.RobustGraph(bad, RH.PSEUDO_HUBER, 0.01); ph.levenberg_marquardt()
    (sp, sl), (pp, pl) = sq.state_error(clean.x), ph.state_error(clean.x)
    print(f"squared LM: pose {sp:.3e} plane {sl:.3e}; pseudo-Huber LM: pose {pp:.3e} plane {pl:.3e}")
    assert np.abs(ph.whitened(k, ph.x)).max() > 3 * 0.01                                  # the outlier sits in the linear part of rho
    assert sp > 2 * pp and sl > 2 * pl
