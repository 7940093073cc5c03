"""GPU: the factor sweeps at every per-type count where a block starts or ends (tests/sweep_count_helpers.py for the graphs, the reference
and the bounds; tests/test_host_sweep_counts.py pins those without a device).

K1, per (case, form): J and r of every factor of the varied type, and of the first and last 16 of every other type (every factor where a
    case varies no type), through pps_eval_factor -- which runs the shipped sweep and reads the factor's slot -- against the oracle:
    r 2e-11, analytic J 1e-11, numeric J 2e-8 (tests/test_gpu_solve.py's figures).  Forms: the lane form (numeric, the default), analytic
    mode, PPS_K1_THREAD_FORM=1 (numeric), a cost function set (k_linearize_robust and the robust re-popping kernel; pseudo-Huber, b = 1);
    the Factor2 cases run k_linearize_repop in all of them.
K4, per (case, form): pps_chi2 at the start; one LM trial (max_iterations = 1): the record's chi2 -- at the downloaded estimate where the
    trial was accepted, at the oracle's retraction of the start by the hook's delta where it was rejected --, the estimate against that
    retraction, |delta| of the record judged next, chi2_final == pps_chi2 bit for bit; and pps_update the same way.  Forms: default
    (k_trial_lin, light records), PPS_NO_EARLY_RECORD, PPS_NO_SPEC_LIN (k_trial_dual), PPS_NO_DUAL (k_retract<true> + k_chi2_trial), a
    cost function set (k_chi2_robust, k_chi2_trial_robust), and P.Multi batches of three different cases in one chunk (kb_chi2 for chi2
    at x -- stats chi2_initial --, kb_trial_dual + kb_chi2_finish for the trials; the batch has the dual-trial form only, and takes every
    graph's iteration cap from the graph's own max_iterations).  The kicked graph runs two trials, both rejected.
    Every single-handle form without a cost function and the batch report the same trace, bit for bit.

Bounds: a chi2 at a state both sides hold bit for bit |chi2 - chi2*| <= max(16 d, 1e-12) max(1, chi2*); a rejected trial's gains S eta
(SC.bound_retracted).  At every compared state the reference asserts min r*'r* >= 8 x the bound in force.  Every comparison prints case,
form, chi2*, d and the ratio to its bound (-s); the last test writes the worst ratio per axis and form to profiles/sweep_counts_device.txt.
"""
import os

import numpy as np
import pytest

import linsolve_helpers as LH
import pop_up_slam_amd as P
import sweep_count_helpers as SC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("PPS_NO_EARLY_RECORD", "PPS_LM_PLAIN_HOST", "PPS_NO_SPEC_LIN", "PPS_NO_DUAL", "PPS_K1_THREAD_FORM", "PPS_MULTI_THREAD_FORM",
            "PPS_MULTI_LEVELS", "PPS_MULTI_SPLIT")
NAMES = list(SC.CASES)
K1_FORMS = {"lanes": (None, P.JAC_NUMERIC, None), "analytic": (None, P.JAC_ANALYTIC, None), "thread": ("PPS_K1_THREAD_FORM", P.JAC_NUMERIC, None),
            "robust": (None, P.JAC_NUMERIC, SC.COST)}
K4_FORMS = {"default": (None, None), "no_early_record": ("PPS_NO_EARLY_RECORD", None), "no_spec_lin": ("PPS_NO_SPEC_LIN", None),
            "no_dual": ("PPS_NO_DUAL", None), "robust": (None, SC.COST)}
SAME_TRACE = ("default", "no_early_record", "no_spec_lin", "no_dual")
TOL_R, TOL_J_ANALYTIC, TOL_J_NUMERIC = 2e-11, 1e-11, 2e-8
_REF, _AT, _RUN, _WORST = {}, {}, {}, {}


def _graph(spec, switch=None, cost=None, **props):
    """a handle created with `switch` set (and none of the others), the variable gone again before anything runs"""
    saved = {k: os.environ.pop(k) for k in SWITCHES if k in os.environ}
    try:
        if switch:
            os.environ[switch] = "1"
        g = P.Graph(**props)
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(saved)
    spec.replay(g)
    if cost is not None:
        g.set_cost_function(*cost)
    st = g.stats()
    assert (st["n_poses"], st["n_planes"], st["n_factors"]) == (spec.n_poses, spec.n_planes, len(spec.f_type)), (spec.name, st)
    return g


def _ref(name, cost=None):
    if (name, cost) not in _REF:
        _REF[(name, cost)] = SC.Reference(SC.make(name), cost)
    return _REF[(name, cost)]


def _note(name, form, what, ratio):
    axis = SC.CASES[name]["axis"] if name in SC.CASES else name
    key = (axis, form, what)
    _WORST[key] = max(_WORST.get(key, 0.0), float(ratio))


def _at(name, cost, state, with_S=False):
    """the reference at a state (exactly these doubles), computed once per state: r*, chi2*, d, and S where a retracted bound needs it"""
    key = (name, cost, state[0].tobytes(), state[1].tobytes())
    if key not in _AT:
        ref = _ref(name, cost)
        ref.set_state(*state)
        res = ref.residuals()
        chi2, d, _ = ref.yardstick(res)
        assert d <= 1e-13, (name, d)
        _AT[key] = {"res": res, "chi2": chi2, "d": d}
    if with_S and "S" not in _AT[key]:
        ref = _ref(name, cost)
        ref.set_state(*state)
        _AT[key]["S"] = ref.sensitivity()
    return _AT[key]


def _check_chi2(name, form, what, got, cost, state, delta=None, base=None):
    """got against chi2* at `state`; with delta: `state` is the oracle's retraction of `base` by delta, which the device holds only to eta"""
    at = _at(name, cost, state, with_S=delta is not None)
    bound = SC.bound_exact(at["chi2"], at["d"]) if delta is None else SC.bound_retracted(at["chi2"], at["d"], at["S"], delta, base)
    vis = SC.assert_visible((name, form, what), at["res"], bound)
    ratio = abs(got - at["chi2"]) / bound
    print(f"SWEEPCOUNTS {name} {form} {what}: chi2 {got:.17g} chi2* {at['chi2']:.17g} d {at['d']:.2e} bound {bound:.3e} ratio {ratio:.3g} (min r'r / bound {vis:.3g})")
    _note(name, form, what, ratio)
    assert ratio <= 1.0, (name, form, what, got, at["chi2"], bound, ratio)


def _state(g):
    return g.get_poses().copy(), g.get_planes().copy() if g.stats()["n_planes"] else np.zeros((0, 4))


def _check_retraction(name, form, what, got, base, delta, lay, cost):
    """the downloaded estimate against the oracle's retraction of `base` by the hook's delta: test_the_hook_measures_the_shipped_path's bound"""
    want = _ref(name, cost).retracted(base, delta, lay)
    dinf = float(np.abs(delta).max())
    worst = 0.0
    for a, b in zip(got, want):
        if b.size:
            tol = 64.0 * SC.EPS * np.maximum(1.0, np.abs(b)) + 1e-13 * dinf
            worst = max(worst, float(np.max(np.abs(a - b) / tol)))
    print(f"SWEEPCOUNTS {name} {form} {what}: estimate against the retraction by the hook's delta, |delta|_inf {dinf:.3e}, ratio {worst:.3g}")
    _note(name, form, what, worst)
    assert worst <= 1.0, (name, form, what, worst)
    return want


def _check_delta_norm(name, form, what, dn, delta):
    n = float(np.linalg.norm(delta))
    ratio = abs(dn - n) / (1e-13 * n)
    print(f"SWEEPCOUNTS {name} {form} {what}: last_delta_norm {dn:.17g} |delta_hook| {n:.17g} ratio {ratio:.3g}")
    _note(name, form, what, ratio)
    assert ratio <= 1.0, (name, form, what, dn, n)


# ---- K1 ----------------------------------------------------------------------------------------------------------------------
def _compared_factors(spec, name):
    slots = SC.type_slots(spec)
    which = SC.varied_type(name)
    if which is None:
        return list(range(len(spec.f_type)))
    ks = []
    for t, lst in slots.items():
        ks += lst if t == which else lst[:16] + lst[-16:]
    return sorted(set(ks))


@pytest.mark.parametrize("form", list(K1_FORMS))
@pytest.mark.parametrize("name", NAMES)
def test_k1_every_factor_at_every_count(built, name, form):
    switch, mode, cost = K1_FORMS[form]
    spec = SC.make(name)
    g = _graph(spec, switch, cost, jacobian_mode=mode)
    ref = _ref(name, cost)
    ref.set_state(*_state(g))
    worst = {"r": 0.0, "J": 0.0}
    ks = _compared_factors(spec, name)
    which = SC.varied_type(name)
    if which is not None:
        assert set(SC.type_slots(spec)[which]) <= set(ks)
    for k in ks:
        J, r = g.eval_factor(k, mode)
        Jo, ro = ref.jacobian(k, analytic=mode)
        numeric = mode == P.JAC_NUMERIC or bool(spec.f_repop[k])          # (Factor2 edges are differentiated numerically in both modes)
        er, ej = float(np.abs(r - ro).max()) / TOL_R, float(np.abs(J - Jo).max()) / (TOL_J_NUMERIC if numeric else TOL_J_ANALYTIC)
        worst["r"], worst["J"] = max(worst["r"], er), max(worst["J"], ej)
        assert J.shape == Jo.shape and er <= 1.0 and ej <= 1.0, (name, form, "factor", k, int(spec.f_type[k]), er, ej)
    print(f"SWEEPCOUNTS {name} K1 {form}: {len(ks)} of {len(spec.f_type)} factors, worst r {worst['r']:.3g} x 2e-11, worst J {worst['J']:.3g} x its bound")
    _note(name, "K1 " + form, "r", worst["r"]); _note(name, "K1 " + form, "J", worst["J"])
    g.close()


# ---- K4 ----------------------------------------------------------------------------------------------------------------------
def _lay(g, spec):
    g.analyze()
    return LH.spec_layout(spec, g.analysis_dump())


def _hook(g, lam, name):
    delta, _, k3form, bad = g.debug_solve(lam)
    assert bad == 0.0, (name, "not_pd", bad)
    return delta, k3form


def _one_trial(name, form):
    """chi2 at the start, then one LM trial on a handle of `form`; everything checked here, the figures kept for the trace comparison"""
    if (name, form) in _RUN:
        return _RUN[(name, form)]
    switch, cost = K4_FORMS[form]
    spec = SC.make(name)
    g = _graph(spec, switch, cost, max_iterations=1)
    lay = _lay(g, spec)
    start = _state(g)
    c0 = g.chi2()
    _check_chi2(name, form, "chi2 at the start", c0, cost, start)
    delta0, k3form = _hook(g, SC.LAMBDA0, name)
    assert k3form in (0, 1), (name, "not a band graph: the dual loop and the batch do not run it", k3form)
    assert g.chi2() == c0
    it = g.batch_optimize()
    tr, st = g.trace(), g.stats()
    assert it == 1 and len(tr) == 1 and tr[0][0] == SC.LAMBDA0, (name, form, it, tr)
    assert st["chi2_initial"] == c0, (name, form, "chi2 at the linearisation point is pps_chi2's", st["chi2_initial"], c0)
    est = _state(g)
    lam, chi, accepted = tr[0]
    if accepted:
        _check_chi2(name, form, "accepted trial", chi, cost, est)
        _check_retraction(name, form, "accepted estimate", est, start, delta0, lay, cost)
    else:
        np.testing.assert_array_equal(est[0], start[0]); np.testing.assert_array_equal(est[1], start[1])
        _check_chi2(name, form, "rejected trial", chi, cost, _ref(name, cost).retracted(start, delta0, lay), delta=delta0, base=start)
    assert st["chi2_final"] == g.chi2() == (chi if accepted else c0), (name, form, st["chi2_final"], g.chi2(), chi, c0)
    # |delta| of the record the loop would judge next: the step for lambda_final at the estimate -- or, where the accepted trial also
    # ended the solve by epsilon_rel (lambda stays), the judged step itself
    converged = accepted and st["lambda_final"] == lam
    assert st["lambda_final"] == (lam if converged else (lam / SC.LAMBDA_FACTOR if accepted else lam * SC.LAMBDA_FACTOR))
    nxt = delta0 if converged else _hook(g, st["lambda_final"], name)[0]
    _check_delta_norm(name, form, "|delta| of the next record", st["last_delta_norm"], nxt)
    out = {"trace": tr, "chi2_0": c0, "chi2": g.chi2(), "est": est, "stats": st, "start": start}
    g.close()
    _RUN[(name, form)] = out
    return out


@pytest.mark.parametrize("form", list(K4_FORMS))
@pytest.mark.parametrize("name", NAMES)
def test_k4_records_of_one_trial(built, name, form):
    _one_trial(name, form)


@pytest.mark.parametrize("form", ["default", "robust"])
@pytest.mark.parametrize("name", NAMES)
def test_k4_update_at_every_count(built, name, form):
    """pps_update: the trial kernel with one trial at lambda = 0 (with a cost function: k_retract<false>, then the robust chi2 sweep)"""
    switch, cost = K4_FORMS[form]
    spec = SC.make(name)
    g = _graph(spec, switch, cost)
    lay = _lay(g, spec)
    start = _state(g)
    delta, _ = _hook(g, 0.0, name)
    g.update()
    st, est = g.stats(), _state(g)
    _check_chi2(name, form, "chi2_final of pps_update", st["chi2_final"], cost, est)
    _check_retraction(name, form, "estimate of pps_update", est, start, delta, lay, cost)
    _check_delta_norm(name, form, "|delta| of pps_update", st["last_delta_norm"], delta)
    assert st["chi2_final"] == g.chi2(), (name, form, st["chi2_final"], g.chi2())
    g.close()


@pytest.mark.parametrize("name", NAMES)
def test_k4_every_form_reports_the_same_trace(built, name):
    runs = {form: _one_trial(name, form) for form in SAME_TRACE}
    ref = runs["default"]
    for form, r in runs.items():
        assert r["trace"] == ref["trace"] and r["chi2_0"] == ref["chi2_0"] and r["chi2"] == ref["chi2"], (name, form, r["trace"], ref["trace"])
        np.testing.assert_array_equal(r["est"][0], ref["est"][0]); np.testing.assert_array_equal(r["est"][1], ref["est"][1])
        assert r["stats"]["last_delta_norm"] == ref["stats"]["last_delta_norm"] and r["stats"]["chi2_final"] == ref["stats"]["chi2_final"], (name, form)


# ---- the rejected start --------------------------------------------------------------------------------------------------------
def _rejected(form):
    if ("rejected", form) in _RUN:
        return _RUN[("rejected", form)]
    name = "rejected"
    switch, cost = K4_FORMS[form]
    spec = SC.make(name)
    g = _graph(spec, switch, cost, max_iterations=2)
    lay = _lay(g, spec)
    start = _state(g)
    c0 = g.chi2()
    _check_chi2(name, form, "chi2 at the start", c0, cost, start)
    it = g.batch_optimize()
    tr, st = g.trace(), g.stats()
    lams = [SC.LAMBDA0, SC.LAMBDA0 * SC.LAMBDA_FACTOR]
    assert it == 2 and [t[0] for t in tr] == lams and [t[2] for t in tr] == [False, False], (form, it, tr)
    est = _state(g)
    np.testing.assert_array_equal(est[0], start[0]); np.testing.assert_array_equal(est[1], start[1])       # the start, bit for bit
    assert st["chi2_final"] == g.chi2() == c0 == st["chi2_initial"]
    for k, lam in enumerate(lams):
        delta, k3form = _hook(g, lam, name)
        assert k3form in (0, 1)
        _check_chi2(name, form, f"rejected trial {k}", tr[k][1], cost, _ref(name, cost).retracted(start, delta, lay), delta=delta, base=start)
    assert st["lambda_final"] == lams[1] * SC.LAMBDA_FACTOR
    _check_delta_norm(name, form, "|delta| of the next record", st["last_delta_norm"], _hook(g, st["lambda_final"], name)[0])
    out = {"trace": tr, "chi2_0": c0, "chi2": g.chi2(), "est": est, "stats": st, "start": start}
    g.close()
    _RUN[(name, form)] = out
    return out


@pytest.mark.parametrize("form", list(K4_FORMS))
def test_k4_two_rejected_trials(built, form):
    r = _rejected(form)
    if form in SAME_TRACE:
        ref = _rejected("default")
        assert r["trace"] == ref["trace"] and r["chi2_0"] == ref["chi2_0"] and r["stats"]["last_delta_norm"] == ref["stats"]["last_delta_norm"], (form, r["trace"], ref["trace"])


# ---- the batch -----------------------------------------------------------------------------------------------------------------
# three different cases per chunk: the launch is as wide as the widest of them, so every graph also meets blocks beyond its own
# (cases three apart in the list share a batch: one of each axis where the axes are long enough)
def _triples():
    n = len(NAMES)
    step = -(-n // 3)
    out = [[NAMES[i], NAMES[(i + step) % n], NAMES[(i + 2 * step) % n]] for i in range(step)]
    assert set(x for t in out for x in t) == set(NAMES) and all(len(set(t)) == 3 for t in out)
    return out


def _check_batch(names, caps):
    gs = [_graph(SC.make(n), None, None, max_iterations=c) for n, c in zip(names, caps)]
    its, status = P.Multi(gs).optimize()
    assert np.all(status == 0), (names, status)
    for g, n, it in zip(gs, names, its):
        ref = _rejected("default") if n == "rejected" else _one_trial(n, "default")
        st = g.stats()
        # kb_chi2 + kb_chi2_finish: chi2 at x
        _check_chi2(n, "batch", "chi2 at the start", st["chi2_initial"], None, ref["start"])
        assert st["chi2_initial"] == ref["chi2_0"], (n, "batch", st["chi2_initial"], ref["chi2_0"])
        # kb_trial_dual + kb_chi2_finish: the single handle's records were checked against the reference; the batch must give their bits
        assert it == len(ref["trace"]) and g.trace() == ref["trace"], (n, "batch", g.trace(), ref["trace"])
        assert g.chi2() == ref["chi2"] and st["chi2_final"] == ref["stats"]["chi2_final"], (n, "batch")
        assert st["last_delta_norm"] == ref["stats"]["last_delta_norm"] and st["lambda_final"] == ref["stats"]["lambda_final"], (n, "batch")
        est = _state(g)
        np.testing.assert_array_equal(est[0], ref["est"][0]); np.testing.assert_array_equal(est[1], ref["est"][1])
        print(f"SWEEPCOUNTS {n} batch of {names}: trace {g.trace()} same bits as the single handle")
    for g in gs:
        g.close()


@pytest.mark.parametrize("names", _triples(), ids=lambda t: "+".join(t))
def test_k4_batch_of_three_cases(built, names):
    _check_batch(names, [1, 1, 1])


def test_k4_batch_with_the_rejected_start(built):
    _check_batch(["rejected", "pp-257", "nodes-513"], [2, 1, 1])


# ---- the report ----------------------------------------------------------------------------------------------------------------
def test_write_the_worst_ratios(built):
    """profiles/sweep_counts_device.txt: the worst ratio to its bound per axis, form and quantity.  Written when every axis ran in every
    form in this process (a run of a few selected tests leaves the file alone)."""
    assert _WORST, "run the whole file: this test reports what the others measured"
    assert max(_WORST.values()) <= 1.0
    axes = {c["axis"] for c in SC.CASES.values()} | {"rejected"}
    forms = {"K1 " + f for f in K1_FORMS} | set(K4_FORMS) | {"batch"}
    have = {(a, f) for a, f, _ in _WORST}
    if not {(a, f) for a in axes for f in forms if not (a == "rejected" and f.startswith("K1"))} <= have:
        return
    lines = ["device against the oracle at every per-type factor count: worst ratio to the bound in force (tests/test_gpu_sweep_counts.py)",
             f"{'axis':<12} {'form':<18} {'quantity':<34} worst ratio"]
    for (axis, form, what), v in sorted(_WORST.items()):
        lines.append(f"{axis:<12} {form:<18} {what:<34} {v:.3g}")
    with open(os.path.join(ROOT, "profiles", "sweep_counts_device.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
