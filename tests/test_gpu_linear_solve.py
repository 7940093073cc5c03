"""GPU: the solved LM step delta of every K3 form (pps_debug_solve) against a dense solve of the same normal equations.

Reference (tests/linsolve_helpers.py): J and r of every factor from pps_eval_factor at the same estimate and Jacobian mode, H = sum J'J and
b = -sum J'r assembled in numpy float64, H_lambda = H + lambda diag(H), solved twice on the CPU by code that shares no path (LU, Cholesky).
d = |x1 - x2| / |x1| is the yardstick; the device passes with e = |delta - x1| / |x1| <= max(16 d, 1e-12), for the whole step and for every
node block (block error in the maximum norm, relative to |x1|_inf of the whole step: a wrong single front cannot hide in the norm).

Every case first asserts -- from the analysis alone -- that its graph has the front shapes it exists for, then that the device ran the
K3 form the case is about (form of pps_debug_solve).  cond(H_lambda), d, e and form are printed per case (run with -s).
"""
import numpy as np
import pytest

import pop_up_slam_amd as P
import linsolve_helpers as LH
from pop_up_slam_amd import synth

pytestmark = pytest.mark.gpu

SINGLE = [(name, mode) for name in LH.CASE_ORDER for mode in LH.CASES[name][3]]
BAND = [(name, mode) for name, mode in SINGLE if 2 not in LH.CASES[name][2]]
_IDS = lambda cm: f"{cm[0]}-jac{cm[1]}"
_CTX = {}


class Ctx:
    """one handle per (case, Jacobian mode) that stays at its initial estimate, its analysis, and the reference of every damping value
    (computed once, shared by the tests, never modified)"""

    def __init__(self, name, mode):
        self.name, self.mode = name, mode
        self.spec = LH.CASES[name][0]()
        self.g = P.Graph(jacobian_mode=mode)
        self.spec.replay(self.g)
        self.g.analyze()
        self.A = self.g.analysis_dump()
        LH.assert_case_shapes(name, self.A)
        self.H, self.b, self.lay = LH.assemble_normal_equations(self.g, self.spec, self.A, mode)
        self.refs = {}

    def ref(self, lam):
        if lam not in self.refs:
            Hl = LH.damped(self.H, lam)
            x1, x2, d = LH.reference_solves(Hl, self.b)
            for v in (x1, x2):
                v.setflags(write=False)
            self.refs[lam] = (Hl, (x1, x2, d), LH.cond_spd(Hl))
        return self.refs[lam]

    def check(self, label, delta, lam, form):
        Hl, refs, cond = self.ref(lam)
        return LH.check_step(f"{self.name} jac {self.mode} {label}", delta, Hl, self.b, self.lay, form, refs, cond)


def _ctx(name, mode):
    if (name, mode) not in _CTX:
        _CTX[(name, mode)] = Ctx(name, mode)
    return _CTX[(name, mode)]


def _state(g):
    return g.chi2(), g.get_poses().copy(), g.get_planes().copy()


def _same_state(a, b):
    assert a[0] == b[0]
    np.testing.assert_array_equal(a[1], b[1]); np.testing.assert_array_equal(a[2], b[2])


@pytest.mark.parametrize("case_mode", SINGLE, ids=_IDS)
def test_single_lambda_step_against_the_dense_solve(built, case_mode):
    c = _ctx(*case_mode)
    g = c.g
    for lam in LH.LAMBDAS:
        before = _state(g)
        delta, delta2, form, bad = g.debug_solve(lam)
        assert delta2 is None and len(delta) == c.A["n_scalars"]
        assert form in LH.CASES[c.name][2], (c.name, "K3 form", form)
        assert bad == 0.0
        c.check(f"lambda {lam:g}", delta, lam, form)
        _same_state(before, _state(g))                                 # the hook leaves the estimate alone, bit for bit


@pytest.mark.parametrize("case_mode", BAND, ids=_IDS)
def test_two_lambdas_in_one_launch(built, case_mode):
    c = _ctx(*case_mode)
    g = c.g
    for lam, lam2 in ((1e-3, 1e-2), (10.0, 100.0)):
        single, _, form1, _ = g.debug_solve(lam)
        delta, delta2, form, bad = g.debug_solve(lam, lam2)
        assert form == form1 and form in (0, 1) and bad == 0.0
        c.check(f"dual ({lam:g}, {lam2:g}) first", delta, lam, form)
        c.check(f"dual ({lam:g}, {lam2:g}) second", delta2, lam2, form)
        # same arithmetic, different launch shape: what test_lm_loop_forms_are_bit_identical relies on
        np.testing.assert_array_equal(delta, single)


@pytest.mark.parametrize("case_mode", [cm for cm in SINGLE if 2 in LH.CASES[cm[0]][2]][:1], ids=_IDS)
def test_two_lambdas_are_refused_outside_the_band_forms(built, case_mode):
    c = _ctx(*case_mode)
    with pytest.raises(P.PpsError) as e:
        c.g.debug_solve(1e-3, 1e-2)
    assert e.value.code == P.PPS_ESTATE and "band" in str(e.value)
    delta, _, form, bad = c.g.debug_solve(1e-3)                        # ... and the handle goes on working
    assert form == 2 and bad == 0.0
    c.check("after the refused dual call, lambda 0.001", delta, 1e-3, form)


@pytest.mark.parametrize("case_mode", SINGLE, ids=_IDS)
def test_the_hook_measures_the_shipped_path(built, case_mode):
    name, mode = case_mode
    c = _ctx(name, mode)
    _, (x1, _, d), _ = c.ref(0.0)
    bound = max(16.0 * d, 1e-12)
    hooked = P.Graph(jacobian_mode=mode); c.spec.replay(hooked)
    plain = P.Graph(jacobian_mode=mode); c.spec.replay(plain)
    poses0, planes0 = hooked.get_poses().copy(), hooked.get_planes().copy()
    for lam in LH.LAMBDAS:
        hooked.debug_solve(lam)
    if 2 not in LH.CASES[name][2]:
        hooked.debug_solve(1e-3, 1e-2)
    delta, _, form, bad = hooked.debug_solve(0.0)
    assert bad == 0.0
    c.check("second handle, lambda 0", delta, 0.0, form)
    hooked.update(); plain.update()
    # |delta| of pps_update is the hook's (the device sums in blocks: bit equality is not promised)
    dn = hooked.stats()["last_delta_norm"]
    assert abs(dn - np.linalg.norm(delta)) <= 1e-13 * np.linalg.norm(delta), (dn, np.linalg.norm(delta))
    # the estimate after pps_update is the retraction of the reference step
    xinf = float(np.max(np.abs(x1)))
    n_pose = len(poses0)
    dp = np.array([x1[c.lay[i][0]:c.lay[i][0] + 6] for i in range(len(c.spec.node_type)) if c.spec.node_type[i] == synth.NODE_POSE])
    want = P.debug_exmap(0, poses0, dp)
    got = hooked.get_poses()
    assert np.all(np.abs(got - want) <= 64 * np.finfo(float).eps * np.maximum(1.0, np.abs(want)) + bound * xinf), np.max(np.abs(got - want))
    if len(planes0):
        dl = np.array([x1[c.lay[i][0]:c.lay[i][0] + 3] for i in range(len(c.spec.node_type)) if c.spec.node_type[i] == synth.NODE_PLANE])
        want = P.debug_exmap(1, planes0, dl)
        got = hooked.get_planes()
        assert np.all(np.abs(got - want) <= 64 * np.finfo(float).eps * np.maximum(1.0, np.abs(want)) + bound * xinf), np.max(np.abs(got - want))
    assert n_pose == len(dp)
    # a handle the hook never touched does the same thing, bit for bit
    assert hooked.chi2() == plain.chi2()
    np.testing.assert_array_equal(hooked.get_poses(), plain.get_poses()); np.testing.assert_array_equal(hooked.get_planes(), plain.get_planes())
    hooked.debug_solve(1e-3)
    assert hooked.batch_optimize() == plain.batch_optimize()
    assert hooked.trace() == plain.trace()
    np.testing.assert_array_equal(hooked.get_poses(), plain.get_poses())
    hooked.close(); plain.close()


def test_singular_normal_equations_in_the_dense_form(built):
    """The 48-pose dense graph without its prior: the gauge is free, H is singular at lambda = 0.  k_dense_panel flags a pivot that is
    not positive through the status word (no fault is involved); the hook hands that word out and clears it, and LM on the same graph
    ends with PPS_OK or PPS_ENOTPD, never PPS_EHIP."""
    spec = LH.loop_graph(48, 150, 10, 5, prior=False)
    g = P.Graph(jacobian_mode=1); spec.replay(g); g.analyze()
    A = g.analysis_dump()
    LH.assert_case_shapes("dense_48p_150l_10x5", A)
    H, b, lay = LH.assemble_normal_equations(g, spec, A, 1)
    before = _state(g)
    delta, _, form, bad = g.debug_solve(0.0)
    assert form == 2
    ev = np.linalg.eigvalsh(H)
    print(f"LINSOLVE singular dense_48p_150l_10x5: form {form} not_pd {bad} eig min {ev[0]:.3e} max {ev[-1]:.3e} finite {bool(np.all(np.isfinite(delta)))}")
    assert ev[6] > 1e6 * abs(ev[5]), "exactly the six gauge directions are (numerically) in the null space"
    assert bad == 1.0, "a pivot of the singular system was not flagged"
    _same_state(before, _state(g))
    # the flag does not outlive the call: a damped solve of the same handle is clean and correct
    Hl = LH.damped(H, 10.0)
    delta, _, form, bad = g.debug_solve(10.0)
    assert bad == 0.0
    LH.check_step("singular dense_48p_150l_10x5 lambda 10", delta, Hl, b, lay, form)
    try:
        g.batch_optimize()
        code = P.PPS_OK
    except P.PpsError as e:
        code = e.code
    assert code in (P.PPS_OK, P.PPS_ENOTPD), code
    assert np.isfinite(g.chi2())
    g.close()
