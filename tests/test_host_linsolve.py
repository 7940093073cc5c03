"""CPU: what tests/test_gpu_linear_solve.py stands on, checked without a device -- the front shapes every case of it exists for (an
ordering change is caught on every machine), the dense reference of tests/linsolve_helpers.py against an extended-precision Cholesky,
and the argument checks of pps_debug_solve (answered before the device is touched)."""
import ctypes as C

import numpy as np
import pytest

import pop_up_slam_amd as P
import linsolve_helpers as LH
from pop_up_slam_amd import synth


@pytest.mark.parametrize("case", LH.CASE_ORDER)
def test_case_graph_has_the_front_shapes_it_exists_for(built, case):
    spec = LH.CASES[case][0]()
    g = P.Graph(jacobian_mode=1); spec.replay(g); g.analyze()
    A = g.analysis_dump()
    LH.assert_case_shapes(case, A)
    lay = LH.spec_layout(spec, A)
    covered = sorted(o + k for o, dim in lay.values() for k in range(dim))
    assert covered == list(range(A["n_scalars"]))                     # node_voff tiles delta: the reference is indexed by it
    g.close()


def test_generator_makes_a_nontrivial_graph():
    spec = LH.loop_graph(48, 150, 10, 5)
    odo = spec.f_nodes[spec.f_type == synth.F_ODOMETRY]
    assert len(odo) == 47 + 150 and np.all(np.abs(odo[47:, 0] - odo[47:, 1]) >= 2)
    assert (spec.f_type == synth.F_PLANE_OBS).sum() == 50 and (spec.f_type == synth.F_POSE_PRIOR).sum() == 1
    q = spec.node_init[:48, 3:7]
    assert np.all(np.abs(q[1:, 3]) < 0.99999) and np.allclose(np.linalg.norm(q, axis=1), 1.0)     # no pose at the identity rotation
    assert (LH.loop_graph(48, 150, 10, 5, prior=False).f_type == synth.F_POSE_PRIOR).sum() == 0
    again = LH.loop_graph(48, 150, 10, 5)
    np.testing.assert_array_equal(spec.f_meas, again.f_meas); np.testing.assert_array_equal(spec.node_init, again.node_init)


def _longdouble_cholesky_solve(H, b):
    """(L L') x = b in np.longdouble, written out: the third, higher-precision opinion the yardstick is pinned with"""
    n = len(H)
    A = H.astype(np.longdouble)
    L = np.zeros((n, n), dtype=np.longdouble)
    for j in range(n):
        L[j, j] = np.sqrt(A[j, j] - L[j, :j] @ L[j, :j])
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    y = np.zeros(n, dtype=np.longdouble)
    for i in range(n):
        y[i] = (b[i] - L[i, :i] @ y[:i]) / L[i, i]
    x = np.zeros(n, dtype=np.longdouble)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


@pytest.mark.parametrize("lam", LH.LAMBDAS)
def test_reference_solves_against_extended_precision(lam):
    """random H with the sparsity of the 64-pose / 200-loop graph: x1 is within 16 d of an extended-precision Cholesky solve"""
    spec = LH.loop_graph(64, 200)
    rng = np.random.default_rng(11)
    N = 6 * 64
    H = np.zeros((N, N)); b = np.zeros(N)
    scale = np.tile([1.0, 1.0, 1.0, 30.0, 30.0, 30.0], 64)           # translation against rotation columns, as in the real H
    for (a, c), t in zip(spec.f_nodes, spec.f_type):
        cols = list(range(6 * a, 6 * a + 6)) + (list(range(6 * c, 6 * c + 6)) if c >= 0 else [])
        J = rng.normal(size=(6, len(cols))) * scale[cols]; r = rng.normal(size=6)
        H[np.ix_(cols, cols)] += J.T @ J; b[cols] -= J.T @ r
    Hl = LH.damped(H, lam)
    assert np.array_equal(np.diag(Hl), np.diag(H) * (1.0 + lam)) and np.array_equal(Hl - np.diag(np.diag(Hl)), H - np.diag(np.diag(H)))
    x1, x2, d = LH.reference_solves(Hl, b)
    x3 = _longdouble_cholesky_solve(Hl, b)
    e3 = float(np.linalg.norm(x1 - x3) / np.linalg.norm(x3))
    print(f"LINSOLVE reference lambda {lam:g}: cond {LH.cond_spd(Hl):.3e} d {d:.3e} |x1 - x_longdouble| / |x| {e3:.3e}")
    assert 0.0 < d < 1e-9
    assert e3 <= max(16.0 * d, 1e-12)
    lay = {k: (6 * k, 6) for k in range(64)}
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps        # (the third opinion is a wider format)
    # check_step accepts the second CPU solve and refuses a step with one wrong entry, or with the other sign
    LH.check_step(f"reference lambda {lam:g}", x2, Hl, b, lay, -1)
    wrong = x1.copy(); wrong[6 * 17 + 4] += 1e-6 * np.max(np.abs(x1))
    with pytest.raises(AssertionError):
        LH.check_step("one wrong block", wrong, Hl, b, lay, -1)
    with pytest.raises(AssertionError):
        LH.check_step("wrong sign", -x1, Hl, b, lay, -1)


def test_debug_solve_argument_errors_come_before_the_device(built):
    L = P.lib()
    spec = synth.small_world(5, 3, seed=1)
    g = P.Graph(); spec.replay(g)
    n = g.analysis_dump()["n_scalars"]
    delta, delta2 = np.zeros(n), np.zeros(n)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    form, bad = C.c_int(-7), C.c_double(-7.0)
    call = lambda h, lam, lam2, d1, d2: L.pps_debug_solve(h, lam, lam2, d1, d2, C.byref(form), C.byref(bad))
    assert call(None, 0.0, -1.0, dp(delta), None) == P.PPS_EINVAL                       # null handle
    assert call(g.h, -1e-3, -1.0, dp(delta), None) == P.PPS_EINVAL                      # lambda < 0
    assert call(g.h, 0.0, -1.0, None, None) == P.PPS_EINVAL                             # null delta
    assert call(g.h, float("nan"), -1.0, dp(delta), None) == P.PPS_EINVAL               # NaN lambda
    assert call(g.h, float("inf"), -1.0, dp(delta), None) == P.PPS_EINVAL
    assert call(g.h, 0.0, float("nan"), dp(delta), dp(delta2)) == P.PPS_EINVAL          # NaN lambda2
    assert call(g.h, 0.0, 1e-2, dp(delta), None) == P.PPS_EINVAL                        # second damping value without its output
    assert "delta2" in L.pps_last_error(g.h).decode()
    assert (form.value, bad.value) == (-7, -7.0) and not delta.any() and not delta2.any()   # nothing was written
    with pytest.raises(P.PpsError) as e:
        g.debug_solve(float("nan"))
    assert e.value.code == P.PPS_EINVAL
    g.close()
