"""GPU: marginal covariances from the multifrontal factor (pps_cov_recover / _marginals / _access / _joint) against a dense inverse.

Reference of every comparison: H = J'J assembled in numpy from pps_eval_factor (same jacobian_mode, at the estimate) of every factor,
inverted on the CPU.  Per block e = |S_dev - S_ref|_F / |S_ref|_F; the yardstick is the disagreement d between two CPU inverses of
the same H that share no code path (np.linalg.inv and scipy cho_solve), per graph, maximum over the same blocks: e <= max(16 d, 1e-12).

The figures e and d are printed per graph (run with -s; PPS_COV_TABLE=<file> collects them as JSON lines).  The measured tables of the
covariance calls on an MI355X are in DESIGN.md, section 5b (COVSEL, COVSHAPE: tests/test_gpu_cov_shapes.py pins the level pass at every
front shape and pattern entry) -- the CPU suite checks the same recursion, and the kernel source compiled for the host, against the dense
inverse (tests/test_host_cov.py, tests/test_host_cov_shapes.py).
"""
import json
import os

import numpy as np
import pytest

import pop_up_slam_amd as P
from cov_helpers import cpu_inverses, dense_h_from_device, factor_pairs, rel_err
from helpers import ALL_FIXTURES, load_fixture
from pop_up_slam_amd import graphio, pipeline, synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


class Recorder:
    """notes the nodes and factors a graph receives, whoever adds them (GraphSpec.replay, the frame pipeline)"""

    def __init__(self, g):
        self.g, self.dims, self.factors = g, {}, {}
        for name, dim in (("add_pose", 6), ("add_plane", 3)):
            self._wrap_node(name, dim)
        for name, binary in (("add_pose_prior", False), ("add_odometry", True), ("add_plane_obs", True), ("add_plane_obs2", True),
                             ("add_plane_prior", False)):
            self._wrap_factor(name, binary)

    def _wrap_node(self, name, dim):
        inner = getattr(self.g, name)
        def f(*a, **k):
            i = inner(*a, **k); self.dims[i] = dim; return i
        setattr(self.g, name, f)

    def _wrap_factor(self, name, binary):
        inner = getattr(self.g, name)
        def f(*a, **k):
            i = inner(*a, **k); self.factors[i] = (int(a[0]), int(a[1]) if binary else -1); return i
        setattr(self.g, name, f)

    def remove_factor(self, fid):
        self.g.remove_factor(fid); del self.factors[fid]

    def node_ids(self):
        return sorted(self.dims)


def _reference(g, rec, mode):
    """dense H over the recorder's nodes (in id order) and its two CPU inverses"""
    ids = rec.node_ids()
    col = {n: k for k, n in enumerate(ids)}
    dims = [rec.dims[n] for n in ids]
    fids = sorted(rec.factors)
    f_nodes = [(col[rec.factors[f][0]], col[rec.factors[f][1]] if rec.factors[f][1] >= 0 else -1) for f in fids]
    H, starts = dense_h_from_device(g, len(ids), dims, fids, f_nodes, mode)
    S1, S2 = cpu_inverses(H)
    def blk(S, r, c):
        return S[starts[col[r]]:starts[col[r]] + rec.dims[r], starts[col[c]]:starts[col[c]] + rec.dims[c]]
    return S1, S2, blk


def _check_against_dense(g, rec, mode, label):
    """all marginals, all factor-joined pairs (both orders), a joint of one pose with its planes; returns (e, d)"""
    ids = rec.node_ids()
    marg = g.cov_marginals()                       # (read BEFORE pps_eval_factor runs: that call moves the linearisation point)
    assert len(marg) == len(ids)
    marg_sel = g.cov_marginals(ids[::3])
    pairs = factor_pairs(list(rec.factors.values()))
    pairs = pairs + [(b, a) for a, b in pairs]
    cross = g.cov_access(pairs)
    pose = next(n for n in reversed(ids) if rec.dims[n] == 6 and any(a == n and b >= 0 and rec.dims[b] == 3 for a, b in rec.factors.values()))
    group = [pose] + sorted({b for a, b in rec.factors.values() if a == pose and b >= 0 and rec.dims[b] == 3})
    joint = g.cov_joint(group)
    S1, S2, blk = _reference(g, rec, mode)
    e = d = 0.0
    for n, M in zip(ids, marg):
        assert M.shape == (rec.dims[n], rec.dims[n])
        assert np.array_equal(M, M.T), (label, n, "diagonal block not symmetric bit for bit")
        assert np.all(np.diag(M) > 0), (label, n)
        e = max(e, rel_err(M, blk(S1, n, n))); d = max(d, rel_err(blk(S2, n, n), blk(S1, n, n)))
    for n, M in zip(ids[::3], marg_sel):
        assert np.array_equal(M, marg[ids.index(n)])
    for (r, c), M in zip(pairs, cross):
        assert M is not None, (label, r, c, "a factor-joined pair must be in the pattern")
        assert M.shape == (rec.dims[r], rec.dims[c])
        e = max(e, rel_err(M, blk(S1, r, c))); d = max(d, rel_err(blk(S2, r, c), blk(S1, r, c)))
    assert np.array_equal(joint, joint.T)
    o = 0
    for i, r in enumerate(group):
        oc = 0
        for c in group:
            J = joint[o:o + rec.dims[r], oc:oc + rec.dims[c]]
            e = max(e, rel_err(J, blk(S1, r, c))); d = max(d, rel_err(blk(S2, r, c), blk(S1, r, c)))
            oc += rec.dims[c]
        assert np.array_equal(joint[o:o + rec.dims[r], o:o + rec.dims[r]], marg[ids.index(r)])
        o += rec.dims[r]
    print(f"COV {label}: nodes {len(ids)} blocks {len(ids) + len(pairs)} e {e:.3e} d {d:.3e} bound {max(16 * d, 1e-12):.3e}")
    if os.environ.get("PPS_COV_TABLE"):                                   # (a file that collects the measured e / d figures of a run)
        with open(os.environ["PPS_COV_TABLE"], "a") as f:
            f.write(json.dumps({"graph": label, "nodes": len(ids), "e": e, "d": d}) + "\n")
    assert e <= max(16 * d, 1e-12), (label, e, d)
    return e, d


def _build(spec, **props):
    g = P.Graph(**props); rec = Recorder(g); spec.replay(g)
    return g, rec


ACCURACY_CASES = {**{name: (lambda name=name: load_fixture(name)[1], 0) for name in ALL_FIXTURES},
                  "small_world_5_3": (lambda: synth.small_world(5, 3), 0),
                  "corridor_60_14": (lambda: synth.corridor(60, 14, seed=7), 0),
                  "c2_corridor_1000": (lambda: synth.corridor(), 0),
                  "corridor_150_analytic": (lambda: synth.corridor(150, 32, seed=8), 1)}


@pytest.mark.parametrize("case", sorted(ACCURACY_CASES))
def test_covariances_against_the_dense_inverse(built, case):
    make, mode = ACCURACY_CASES[case]
    g, rec = _build(make(), jacobian_mode=mode)
    g.batch_optimize()
    g.cov_recover()
    _check_against_dense(g, rec, mode, case)
    g.close()


def test_a_pair_outside_the_pattern_is_reported_not_invented(built):
    g, rec = _build(synth.corridor(60, 14, seed=7))
    g.batch_optimize(); g.cov_recover()
    ids = rec.node_ids()
    poses = [n for n in ids if rec.dims[n] == 6]
    res = g.cov_access([(poses[0], poses[-1]), (poses[0], poses[1])])
    assert res[0] is None and res[1] is not None
    with pytest.raises(P.PpsError) as e:
        g.cov_joint([poses[0], poses[-1]])
    assert e.value.code == P.PPS_ESTATE and "outside the pattern" in str(e.value)
    g.close()


def test_validity_ends_with_every_change_and_a_new_recovery_sees_the_new_state(built):
    spec = synth.small_world(20, 6, seed=2, obs_per_pose=5)
    g, rec = _build(spec)
    g.batch_optimize()
    ids = rec.node_ids()
    pose0 = next(n for n in ids if rec.dims[n] == 6); plane0 = next(n for n in ids if rec.dims[n] == 3)
    obs = next(f for f, (a, b) in rec.factors.items() if b >= 0 and rec.dims[b] == 3)

    def add_node_and_factor():
        p = g.add_pose(g.get_pose(pose0)); g.add_pose_prior(p, np.zeros(6), synth._ut_diag([1.0] * 6))
    changes = {
        "add": add_node_and_factor,
        "remove_factor": lambda: rec.remove_factor(max(f for f, (a, b) in rec.factors.items() if b >= 0 and rec.dims[b] == 3)),
        "set_pose": lambda: g.set_pose(pose0, synth.pose_exmap(g.get_pose(pose0), np.array([0.01, 0, 0, 0, 0.01, 0]))),
        "set_plane": lambda: g.set_plane(plane0, synth.plane_exmap(g.get_plane(plane0), np.array([0.01, -0.01, 0.02]))),
        "set_measurement": lambda: g.set_measurement(obs, synth.plane_exmap(g.get_measurement(obs), np.array([0.02, -0.01, 0.03]))),
        "update": g.update,
        "batch_optimize": g.batch_optimize,
        "restore_state": g.restore_state,
        "refresh_measurements": g.refresh_measurements,
    }
    g.save_state()
    for name, change in changes.items():
        g.cov_recover()
        assert len(g.cov_marginals()) == len(rec.node_ids())            # recover -> read: fine
        change()
        for read in (lambda: g.cov_marginals(), lambda: g.cov_access([(pose0, plane0)]), lambda: g.cov_joint([pose0])):
            with pytest.raises(P.PpsError) as e:
                read()
            assert e.value.code == P.PPS_ESTATE, name
        g.cov_recover()
        _check_against_dense(g, rec, 0, "after " + name)
        if name in ("add", "remove_factor"):
            g.save_state()                                              # (a snapshot belongs to one topology)
    g.close()


def test_multi_optimize_membership_ends_a_recovery(built):
    import ctypes as C
    gs = []
    for seed in (1, 2):
        g, _ = _build(synth.small_world(12, 4, seed=seed, obs_per_pose=4)); g.batch_optimize(); g.cov_recover(); gs.append(g)
    L = P.lib()
    arr = (C.c_void_p * 2)(*[g.h for g in gs]); m = C.c_void_p()
    assert L.pps_multi_create(2, arr, C.byref(m)) == P.PPS_OK
    assert len(gs[0].cov_marginals()) > 0
    assert L.pps_multi_optimize(m, None, None) == P.PPS_OK
    for g in gs:
        with pytest.raises(P.PpsError) as e:
            g.cov_marginals()
        assert e.value.code == P.PPS_ESTATE
    assert L.pps_multi_destroy(m) == P.PPS_OK
    for g in gs:
        g.close()


def test_frame_loop_recovery_after_incremental_analyses(built):
    frames = pipeline.popup_sequence(24, seed=3)
    pl, g, pp, stats = pipeline.gpu_pipeline(step=2)
    rec = Recorder(g)
    for k, fr in enumerate(frames):
        pl.process(fr)
        if k in (7, 16, 23):
            if k == 16:
                g.update()
            g.cov_recover()
            _check_against_dense(g, rec, 0, f"frame loop, frame {k}")
    assert g.analysis_reuse()[0] > 0
    pipeline.gpu_pipeline_finish(pp, stats)
    g.close()


def test_recovery_does_not_disturb_the_solves(built):
    spec = synth.corridor(150, 32, seed=8)
    def run(with_cov):
        g = P.Graph(); spec.replay(g)
        if with_cov:
            g.cov_recover()
        it1 = g.batch_optimize(); tr1 = g.trace(); st1 = g.stats()
        x1 = (g.get_poses().copy(), g.get_planes().copy())
        if with_cov:
            g.cov_recover()
            after = g.stats()
            for k in ("lm_iterations", "lm_trials_accepted", "lm_trials_rejected", "chi2_initial", "chi2_final", "lambda_final", "last_delta_norm",
                      "n_linearize", "n_factorize", "n_launches", "t_total"):
                assert after[k] == st1[k], k                            # the stats of the last solve stay what they were
            assert g.trace() == tr1
            np.testing.assert_array_equal(g.get_poses(), x1[0]); np.testing.assert_array_equal(g.get_planes(), x1[1])
        it2 = g.batch_optimize(); tr2 = g.trace()
        x2 = (g.get_poses().copy(), g.get_planes().copy())
        g.close()
        return it1, tr1, x1, it2, tr2, x2
    a, b = run(False), run(True)
    assert a[0] == b[0] and a[1] == b[1] and a[3] == b[3] and a[4] == b[4]
    for i in (2, 5):
        np.testing.assert_array_equal(a[i][0], b[i][0]); np.testing.assert_array_equal(a[i][1], b[i][1])


def test_dense_front_graph_is_refused_and_stays_usable(built):
    spec = graphio.load_edge3_log(os.path.join(HERE, "golden", "isam_data", "sphere2500.txt"), max_lines=1400)
    g = P.Graph(jacobian_mode=1); spec.replay(g); g.analyze()
    assert g.stats()["max_front"] > 127                                  # (so that the refusal cannot come from somewhere else)
    with pytest.raises(P.PpsError) as e:
        g.cov_recover()
    assert e.value.code == P.PPS_ESTATE and "dense-front" in str(e.value)
    c0 = g.chi2(); g.batch_optimize()
    assert g.chi2() < c0
    with pytest.raises(P.PpsError) as e:
        g.cov_marginals()
    assert e.value.code == P.PPS_ESTATE
    g.close()


def test_graph_without_any_prior_is_not_positive_definite(built):
    spec = synth.small_world(12, 4, seed=3, obs_per_pose=4)
    g = P.Graph(); rec = Recorder(g); spec.replay(g)
    for f in [f for f, (a, b) in rec.factors.items() if b < 0]:          # every prior goes: the gauge is free, H is singular at lambda = 0
        rec.remove_factor(f)
    before = (g.get_poses().copy(), g.get_planes().copy())
    with pytest.raises(P.PpsError) as e:
        g.cov_recover()
    assert e.value.code == P.PPS_ENOTPD and "positive definite" in str(e.value)
    with pytest.raises(P.PpsError) as e:
        g.cov_marginals()
    assert e.value.code == P.PPS_ESTATE
    np.testing.assert_array_equal(g.get_poses(), before[0]); np.testing.assert_array_equal(g.get_planes(), before[1])
    assert np.isfinite(g.chi2())                                         # the handle goes on working
    g.close()
