"""GPU: robust cost functions (pps_set_cost_function; csrc/pps_robust.hip) against the numpy restatement of tests/robust_helpers.py, to the
bounds tests/test_gpu_golden.py applies to the same quantities without a cost function: r 2e-11, numeric J 2e-8, analytic J 2e-5 against
the central differences, chi2 at a fixed state 1e-12, a Gauss-Newton step 1e-8, LM trajectories lambda 1e-12 / chi2 1e-7 / final chi2 1e-9 /
final state 1e-6.  The restatement's references are computed once per module."""
import functools
import os
import subprocess

import numpy as np
import pytest

import pop_up_slam_amd as P
import robust_helpers as RH
from cov_helpers import cpu_inverses, dense_h_from_device, rel_err
from helpers import load_fixture
from pop_up_slam_amd import graphio, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = [RH.HUBER, RH.PSEUDO_HUBER, RH.CAUCHY]
EVAL_FIXTURES = ["small_5p_3l", "small_20p_6l", "hard_30p_8l", "pi_wrap_8p_3l"]


@functools.lru_cache(maxsize=None)
def _spec(name):
    """(spec, b): `corrupt:` prefix = ONE grossly wrong plane observation; b = the median whitened |r_i| at the initial state, so that
    components lie on both sides of Huber's kink"""
    if name.startswith("corrupt:"):
        spec = RH.corrupt_one_observation(load_fixture(name[8:])[1])[0]
    else:
        spec = load_fixture(name)[1]
    g = RH.RobustGraph(spec)
    w = np.concatenate([np.abs(g.whitened(k, g.x)) for k in range(len(spec.f_type))])
    b = float(np.median(w[w > 0]))
    assert np.sum(w < b) >= 3 and np.sum(w > b) >= 3 and b < 3.0
    return spec, b


# b of the whole solves: a few inlier standard deviations (inlier whitened residuals of small_20p_6l: median 4.6e-4, largest 2.9e-3; the
# outlier 3.4e-2), which also keeps the restatement's dense LM to a few seconds (at the median it takes > 100 trials)
LM_B = {"corrupt:small_20p_6l": 0.02, "hard_30p_8l": 0.05}
LM_CASES = sorted(LM_B)


@functools.lru_cache(maxsize=None)
def _lm_ref(name, kind):
    spec, b = _spec(name)[0], LM_B[name]
    ref = RH.RobustGraph(spec, kind, b)
    it, chi0, trace = ref.levenberg_marquardt()
    return it, chi0, trace, ref.chi2(ref.x), [np.array(v) for v in ref.x]


def _device(spec, kind, b, **props):
    g = P.Graph(**props)
    nid, fid = spec.replay(g)
    g.set_cost_function(kind, b)
    return g, nid, fid


def _check_state(g, spec, nid, want, atol=1e-6):
    for i, x in enumerate(want):
        if spec.node_type[i] == synth.NODE_POSE:
            got = np.array(g.get_pose(int(nid[i])))
            np.testing.assert_allclose(got[:3], x[:3], atol=atol)
            assert min(np.abs(got[3:] - x[3:]).max(), np.abs(got[3:] + x[3:]).max()) < atol
        else:
            got = np.array(g.get_plane(int(nid[i])))
            assert min(np.abs(got - x).max(), np.abs(got + x).max()) < atol


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", EVAL_FIXTURES)
def test_factor_residuals_jacobians_and_chi2(built, name, kind):
    spec, b = _spec(name)
    ref = RH.RobustGraph(spec, kind, b)
    ana = RH.RobustGraph(spec, kind, b, analytic=True)
    g, nid, fid = _device(spec, kind, b)
    want = ref.chi2(ref.x)
    assert abs(g.chi2() - want) <= 1e-12 * max(1.0, want)
    worst = [0.0, 0.0, 0.0]
    for k in range(len(spec.f_type)):
        H, r0 = ref.factor_jacobian(k, ref.x)
        J, r = g.eval_factor(int(fid[k]), P.JAC_NUMERIC)
        scale = max(1.0, np.abs(r0).max()); hs = max(1.0, np.abs(H).max())
        worst[0] = max(worst[0], np.abs(r - r0).max() / scale); worst[1] = max(worst[1], np.abs(J - H).max() / hs)
        np.testing.assert_allclose(r, r0, rtol=0, atol=2e-11 * scale)
        np.testing.assert_allclose(J, H, rtol=0, atol=2e-8 * hs)
        Ja, ra = g.eval_factor(int(fid[k]), P.JAC_ANALYTIC)
        np.testing.assert_allclose(ra, r0, rtol=0, atol=2e-11 * scale)
        # JAC_ANALYTIC is the chain rule: phi'(r_i) times the squared error's row, which test_gpu_golden.py holds to the central differences
        # at 2e-5 (their O(eps^2) truncation).  The central differences THROUGH phi are no yardstick for it at this b: their truncation
        # grows with (eps |J| / b)^2 (tests/robust_helpers.py).
        Hc, _ = ana.factor_jacobian(k, ana.x)
        hc = max(1.0, np.abs(Hc).max())
        worst[2] = max(worst[2], np.abs(Ja - Hc).max() / hc)
        np.testing.assert_allclose(Ja, Hc, rtol=2e-5, atol=2e-5 * hc)
    print(f"{name} kind {kind} b {b:.3e}: worst r {worst[0]:.2e} numeric J {worst[1]:.2e} analytic J {worst[2]:.2e}")
    g.close()


@pytest.mark.parametrize("kind", [RH.PSEUDO_HUBER, RH.CAUCHY])
@pytest.mark.parametrize("name", LM_CASES)
def test_lm_trajectory_of_the_smooth_costs(built, name, kind):
    spec, b = _spec(name)[0], LM_B[name]
    it, chi0, trace, chi_final, x_final = _lm_ref(name, kind)
    g, nid, fid = _device(spec, kind, b)
    assert g.batch_optimize() == it
    tr = g.trace()
    print(f"{name} kind {kind}: {it} iterations, chi2 {chi0:.6g} -> {chi_final:.9g}; device {g.chi2():.9g}")
    assert [bool(a) for _, _, a in tr] == [bool(a) for _, _, a in trace]
    np.testing.assert_allclose([l for l, _, _ in tr], [l for l, _, _ in trace], rtol=1e-12)
    np.testing.assert_allclose([c for _, c, _ in tr], [c for _, c, _ in trace], rtol=1e-7)
    assert abs(g.stats()["chi2_initial"] - chi0) <= 1e-12 * max(1.0, chi0)
    assert abs(g.chi2() - chi_final) <= 1e-9 * chi_final
    _check_state(g, spec, nid, x_final)
    g.close()


@pytest.mark.parametrize("name", LM_CASES)
def test_huber_final_chi2_and_estimate(built, name):
    """a component on the kink may flip a verdict on rounding: only the end of the solve is compared"""
    spec, b = _spec(name)[0], LM_B[name]
    it, chi0, trace, chi_final, x_final = _lm_ref(name, RH.HUBER)
    g, nid, fid = _device(spec, RH.HUBER, b)
    g.batch_optimize()
    assert abs(g.chi2() - chi_final) <= 1e-9 * chi_final
    _check_state(g, spec, nid, x_final)
    g.close()


@pytest.mark.parametrize("mode", [P.JAC_NUMERIC, P.JAC_ANALYTIC])
@pytest.mark.parametrize("kind", KINDS)
def test_update_is_one_gauss_newton_step_of_the_robustified_system(built, kind, mode):
    """chi2 after pps_update against the restatement's Gauss-Newton step, to test_gpu_golden.py's 1e-8 in both modes.  JAC_NUMERIC: the
    restatement's own central differences.  JAC_ANALYTIC: the restatement has no closed-form Jacobian, so its dense step is taken over the
    robustified records pps_eval_factor returns in that mode (held to the chain rule at 2e-5 by the test above) -- what is checked is
    that the update IS the Gauss-Newton step of that system; retraction and chi2 are the restatement's."""
    spec, b = _spec("small_20p_6l")
    ref = RH.RobustGraph(spec, kind, b)
    g, nid, fid = _device(spec, kind, b, jacobian_mode=mode)
    if mode == P.JAC_NUMERIC:
        ref.gauss_newton_step()
    else:
        rows, rhs = [], []
        for k in range(len(spec.f_type)):
            J, r = g.eval_factor(int(fid[k]), P.JAC_ANALYTIC)
            R = np.zeros((J.shape[0], ref.n())); c = 0
            for n in spec.f_nodes[k]:
                if n >= 0:
                    R[:, ref.start[n]:ref.start[n] + ref.dim[n]] = J[:, c:c + ref.dim[n]]; c += ref.dim[n]
            rows.append(R); rhs.append(-r)
        ref.x = ref.retract(ref.x, ref.solve(np.vstack(rows), np.concatenate(rhs), 0.0))
    want = ref.chi2(ref.x)
    g.update()
    print(f"kind {kind} mode {mode}: chi2 after the step {g.chi2():.12g}, restatement {want:.12g}")
    assert abs(g.chi2() - want) <= 1e-8 * max(want, 1e-12)
    g.close()


@pytest.mark.parametrize("no_dual", [False, True])
def test_cost_none_returns_the_handle_to_todays_launches(built, monkeypatch, no_dual):
    if no_dual:
        monkeypatch.setenv("PPS_NO_DUAL", "1")
    else:
        monkeypatch.delenv("PPS_NO_DUAL", raising=False)
    spec = load_fixture("hard_30p_8l")[1]
    a = P.Graph(); nid_a, _ = spec.replay(a)
    b = P.Graph(); nid_b, _ = spec.replay(b)
    b.set_cost_function(P.COST_PSEUDO_HUBER, 0.01); c_rob = b.chi2()
    b.set_cost_function(P.COST_NONE)
    assert c_rob != a.chi2() and b.chi2() == a.chi2()
    assert a.batch_optimize() == b.batch_optimize()
    assert a.stats()["n_launches"] == b.stats()["n_launches"]
    assert np.array_equal(np.array(a.trace()), np.array(b.trace()))
    assert np.array_equal(a.get_poses(), b.get_poses()) and np.array_equal(a.get_planes(), b.get_planes())
    a.close(); b.close()


def test_cost_set_takes_the_one_step_loop_whatever_the_switch_says(built, monkeypatch):
    spec, bb = _spec("corrupt:small_20p_6l")
    out = []
    for no_dual in (False, True):
        if no_dual:
            monkeypatch.setenv("PPS_NO_DUAL", "1")
        else:
            monkeypatch.delenv("PPS_NO_DUAL", raising=False)
        g, nid, fid = _device(spec, P.COST_PSEUDO_HUBER, bb)
        g.batch_optimize()
        out.append((np.array(g.trace()), g.get_poses().copy(), g.stats()["n_launches"]))
        g.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]


def test_covariances_of_the_robustified_system(built):
    """pps_cov_recover + pps_cov_marginals with pseudo-Huber against the dense inverse of J'J from pps_eval_factor's robustified records:
    the measure and bound of tests/test_gpu_cov.py (two CPU inverses that share no code path: e <= max(16 d, 1e-12))"""
    spec, b = _spec("small_20p_6l")
    g, nid, fid = _device(spec, P.COST_PSEUDO_HUBER, b)
    g.batch_optimize()
    dims = [6 if t == synth.NODE_POSE else 3 for t in spec.node_type]
    f_nodes = [(int(a), int(c)) for a, c in spec.f_nodes]
    H, starts = dense_h_from_device(g, len(dims), dims, fid, f_nodes, P.JAC_NUMERIC)
    g2 = P.Graph(); spec.replay(g2)                                       # the squared system's H differs: the recovery must be the robust one
    for i, n in enumerate(nid):
        (g2.set_pose if dims[i] == 6 else g2.set_plane)(int(n), (g.get_pose if dims[i] == 6 else g.get_plane)(int(n)))
    H2, _ = dense_h_from_device(g2, len(dims), dims, fid, f_nodes, P.JAC_NUMERIC)
    assert rel_err(H2, H) > 1e-3
    S1, S2 = cpu_inverses(H)
    g.cov_recover()
    blocks = g.cov_marginals([int(n) for n in nid])
    e = d = 0.0
    for i, M in enumerate(blocks):
        sl = slice(starts[i], starts[i] + dims[i])
        e = max(e, rel_err(M, S1[sl, sl])); d = max(d, rel_err(S2[sl, sl], S1[sl, sl]))
    print(f"robust COV: e {e:.3e} d {d:.3e} bound {max(16 * d, 1e-12):.3e}")
    assert e <= max(16 * d, 1e-12)
    # pps_set_cost_function counts as a pps_set_*: the recovery ends, reads answer PPS_ESTATE
    g.set_cost_function(P.COST_PSEUDO_HUBER, b)
    with pytest.raises(P.PpsError) as err:
        g.cov_marginals()
    assert err.value.code == P.PPS_ESTATE
    g.close(); g2.close()


def test_dense_front_graph_solves_to_the_restatements_final_chi2(built):
    """sphere2500's first 700 edges: 376 poses, a front of 138 scalars -- beyond the band kernels, so the dense-front K3 runs behind the
    robust K1.  chi2 at the initial state against the live restatement; the pseudo-Huber solve against the restatement's RECORDED solve
    (tests/golden/robust_sphere700_pseudo_huber.json, written once by tests/robust_helpers.py: 24 dense LM iterations take over a minute)."""
    import json
    with open(os.path.join(ROOT, "tests", "golden", "robust_sphere700_pseudo_huber.json")) as f:
        rec = json.load(f)
    spec = graphio.load_edge3_log(os.path.join(ROOT, "tests", "golden", "isam_data", "sphere2500.txt"), max_lines=rec["max_lines"])
    g = P.Graph(); spec.replay(g); g.analyze()
    assert g.stats()["max_front"] > 127
    g.set_cost_function(rec["kind"], rec["b"])
    ref = RH.RobustGraph(spec, rec["kind"], rec["b"])
    want = ref.chi2(ref.x)
    assert abs(want - rec["chi2_initial"]) <= 1e-12 * want                 # the record belongs to this graph
    assert abs(g.chi2() - want) <= 1e-12 * max(1.0, want)
    it = g.batch_optimize()
    tr = g.trace()
    print(f"dense front: {it} iterations (recorded {rec['lm_iterations']}), chi2 {g.chi2():.12g} (recorded {rec['chi2_final']:.12g})")
    assert it == rec["lm_iterations"]
    assert [bool(a) for _, _, a in tr] == [bool(a) for _, _, a in rec["lm_trace"]]
    np.testing.assert_allclose([c for _, c, _ in tr], [c for _, c, _ in rec["lm_trace"]], rtol=1e-7)
    assert abs(g.chi2() - rec["chi2_final"]) <= 1e-9 * rec["chi2_final"]
    g.close()


@functools.lru_cache(maxsize=None)
def _factor2_ops():
    from tests.test_gpu_factor2 import _mixed_graph
    ops = _mixed_graph(6)
    sp = RH.OpsSpec(ops)
    assert len(sp.rays) >= 10
    sq = RH.RobustGraph(sp)
    w = np.concatenate([np.abs(sq.whitened(k, sq.x)) for k in range(len(sp.f_type))])
    return ops, sp, float(np.median(w[w > 0]))


@pytest.mark.parametrize("kind", KINDS)
def test_factor2_graph_residuals_jacobians_and_chi2(built, kind):
    """a graph whose wall edges alternate between the stored-measurement factor and Pose3d_Plane3d_Factor2 (pps_add_plane_obs2: central
    differences in both Jacobian modes, the measurement moves with the pose): k_linearize_repop_robust and the re-pop branch of the chi2 body"""
    from tests.test_gpu_factor2 import _replay
    ops, sp, b = _factor2_ops()
    ref = RH.RobustGraph(sp, kind, b)
    g = P.Graph(); fids = _replay(ops, g); g.set_cost_function(kind, b)
    want = ref.chi2(ref.x)
    assert abs(g.chi2() - want) <= 1e-12 * max(1.0, want)
    n2 = 0; worst = [0.0, 0.0]
    for k, (what, fid) in enumerate(fids):
        if what != "obs2":
            continue
        n2 += 1
        H, r0 = ref.factor_jacobian(k, ref.x)
        w0 = np.abs(ref.whitened(k, ref.x))
        scale = max(1.0, np.abs(r0).max()); hs = max(1.0, np.abs(H).max())
        for mode in (P.JAC_NUMERIC, P.JAC_ANALYTIC):                       # (both are central differences for this factor)
            J, r = g.eval_factor(fid, mode)
            worst[0] = max(worst[0], np.abs(r - r0).max() / scale); worst[1] = max(worst[1], np.abs(J - H).max() / hs)
            np.testing.assert_allclose(r, r0, rtol=0, atol=2e-11 * scale)
            np.testing.assert_allclose(J, H, rtol=0, atol=2e-8 * hs)
    print(f"Factor2 kind {kind} b {b:.3e}: {n2} edges, worst r {worst[0]:.2e} J {worst[1]:.2e}")
    assert n2 == len(sp.rays)
    g.close()


def test_factor2_graph_solves_to_the_restatements_final_chi2(built):
    from tests.test_gpu_factor2 import _replay
    ops, sp, _ = _factor2_ops()
    b = 0.005                                                              # (whitened residuals at the start: median 7e-4, largest 3.5e-2)
    ref = RH.RobustGraph(sp, RH.PSEUDO_HUBER, b)
    it, chi0, trace = ref.levenberg_marquardt()
    want = ref.chi2(ref.x)
    g = P.Graph(); _replay(ops, g); g.set_cost_function(P.COST_PSEUDO_HUBER, b)
    assert g.batch_optimize() == it
    tr = g.trace()
    print(f"Factor2 solve: {it} iterations, chi2 {chi0:.6g} -> {want:.12g}; device {g.chi2():.12g}")
    assert [bool(a) for _, _, a in tr] == [bool(a) for _, _, a in trace]
    np.testing.assert_allclose([c for _, c, _ in tr], [c for _, c, _ in trace], rtol=1e-7)
    assert abs(g.chi2() - want) <= 1e-9 * want
    g.close()


def test_facade_replay_gives_the_cabi_result(built, tmp_path):
    exe = tmp_path / "robust_facade"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "robust_facade.cpp"), "-o", str(exe),
                           "-L", os.path.join(ROOT, "pop_up_slam_amd"), "-lpps", "-Wl,-rpath," + os.path.join(ROOT, "pop_up_slam_amd")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    F = [l[2:] for l in lines if l.startswith("F ")]; Cc = [l[2:] for l in lines if l.startswith("C ")]
    assert len(F) == len(Cc) == 4 and F == Cc
    assert [int(l.split()[0]) for l in F] == [P.COST_PSEUDO_HUBER, P.COST_HUBER, P.COST_CAUCHY, P.COST_NONE]
    chis = [float.fromhex(l.split()[2]) for l in F]
    assert all(c == c and c > 0 for c in chis) and len(set(chis)) == 4               # four different error functions
