"""GPU: pps_cov_factor -- the factor-only recovery, band or dense-front -- and the path walk for wide fronts (k_cov_path_wide) behind
pps_cov_block and pps_assoc_gate, against a dense inverse.

Reference everywhere: H = sum J'J assembled in numpy from pps_eval_factor of every factor, inverted twice (cov_helpers.cpu_inverses).
e and d as in tests/test_gpu_cov_block.py (per node pair, |M - M0|_F / sqrt(|S0(r, r)|_F |S0(c, c)|_F); d the same between the two CPU
inverses, maximum over the same blocks); bound e <= max(16 d, 1e-12).  One `COVFACTOR <graph>: e ... d ...` line per graph (-s).

Graphs: the four dense cases of tests/linsolve_helpers.py in analytic mode, a fifth of the same maker whose fronts pass 1 024 rows
(tests/cov_factor_helpers.py says why), and the first 1 400 lines of sphere2500.  The node sets and their shape contract are asserted on
the CPU (tests/test_host_cov_factor.py) and again here from the same dump.

State: a pps_cov_recover that is refused (dense-front graph) starts, like every pps_cov_recover, by ending what the handle holds -- the factor
of an earlier pps_cov_factor included.  The order that holds is therefore recover (refused) -> factor -> queries; it is tested below.
"""
import os

import numpy as np
import pytest

import pop_up_slam_amd as P
from cov_factor_helpers import DENSE, GRAPHS, WIDE, assert_contract, choose_nodes
from linsolve_helpers import assert_case_shapes, loop_graph, spec_layout
from pop_up_slam_amd import graphio, synth
from test_gpu_cov import Recorder, _build, _reference
from test_gpu_cov_block import _errors
from test_gpu_gate import _measurements, _reference_d2
from test_host_cov_factor import SINGULAR

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NO_RECOVERY = "no valid covariance recovery"


def _dense(name, **props):
    spec = GRAPHS[name]()
    g, rec = _build(spec, jacobian_mode=1, **props)
    g.analyze()
    A = g.analysis_dump()
    if name in DENSE:
        assert_case_shapes(name, A)
    assert A["max_front"] > 127
    lay = spec_layout(spec, A)
    sel = choose_nodes(A, lay)
    assert_contract(name, A, lay, sel)
    return g, rec, sel


def _check(label, g, rec, queries, got):
    S1, S2, blk = _reference(g, rec, 1)
    e = d = 0.0
    for (r, c), M in zip(queries, got):
        assert np.all(np.isfinite(M)), label
        if c is None:
            assert np.array_equal(M, M.T), (label, "joint not symmetric bit for bit")
            assert np.all(np.diag(M) > 0), label
        eq, dq = _errors(M, r, r if c is None else c, rec, S1, S2, blk)
        e, d = max(e, eq), max(d, dq)
    print(f"COVFACTOR {label}: nodes {len(rec.node_ids())} e {e:.3e} d {d:.3e} bound {max(16 * d, 1e-12):.3e}")
    assert e <= max(16 * d, 1e-12), (label, e, d)


# ---- 1. dense cases ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GRAPHS))
def test_dense_front_blocks_against_the_dense_inverse(built, name):
    g, rec, sel = _dense(name)
    g.cov_factor()
    queries = [(sel, None), (sel[:4], sel[2:7])]                        # the joint marginal; rows x cols with nodes in both lists
    if name == "dense_48p_150l_10x5":
        queries.append((rec.node_ids(), None))                          # every node: all 58 diagonal blocks (and every cross block)
        assert len(rec.node_ids()) == 58
    got = []
    for r, c in queries:
        got.append(g.cov_block(r, c))
        assert g.cov_block_last()[1] == 2                               # one walk launch, one Gram launch
    assert g.cov_last_times()[0] > 0 and g.cov_last_times()[1] == 0
    _check(name, g, rec, queries, got)
    g.close()


# ---- 2. sphere2500 ------------------------------------------------------------------------------------------------------------
def test_sphere2500_after_batch_optimize(built):
    spec = graphio.load_edge3_log(os.path.join(HERE, "golden", "isam_data", "sphere2500.txt"), max_lines=1400)
    g, rec = _build(spec, jacobian_mode=1)
    g.analyze()
    assert g.stats()["max_front"] > 127
    g.batch_optimize()
    poses = rec.node_ids()
    sel = [poses[k] for k in sorted(set(np.linspace(0, len(poses) - 1, 6).astype(int).tolist()))]      # first, last, four between
    g.cov_factor()
    M = g.cov_block(sel)
    assert g.cov_block_last()[1] == 2
    with pytest.raises(P.PpsError) as e:                                 # the full recovery still refuses the graph ...
        g.cov_recover()
    assert e.value.code == P.PPS_ESTATE and "dense-front" in str(e.value)
    with pytest.raises(P.PpsError) as e:                                 # ... and, like every pps_cov_recover, has ended what the handle held
        g.cov_block(sel)
    assert e.value.code == P.PPS_ESTATE and NO_RECOVERY in str(e.value)
    g.cov_factor()                                                       # the order that holds: recover (refused) -> factor -> queries
    assert np.array_equal(g.cov_block(sel), M)
    _check("sphere2500_1400", g, rec, [(sel, None)], [M])
    g.close()


# ---- 3. the gate ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dense_48p_150l_10x5", "dense_100p_100l_30x8"])
def test_gate_on_a_dense_front_graph_against_numpy(built, name):
    g, rec, sel = _dense(name)
    ids = rec.node_ids()
    poses = [n for n in ids if rec.dims[n] == 6]; planes = [n for n in ids if rec.dims[n] == 3]
    pose = poses[-1]
    g.cov_factor()
    meas, W, src = _measurements(g, pose, planes, seed=11, steps=(2.5, 10.0, 40.0))
    assert len(meas) == 3
    d2, best = g.assoc_gate(pose, meas, W, planes)
    assert g.assoc_gate_last()[1] == 2
    S1, S2, blk = _reference(g, rec, 1)
    # r and Jw of the candidates: each added to THIS handle as a real factor, afterwards (the estimate passes through the re-analysis as a copy)
    state = (g.get_poses().copy(), g.get_planes().copy())
    r = np.zeros((3, len(planes), 3)); J = np.zeros((3, len(planes), 3, 9))
    fids = [[P.Graph.add_plane_obs(g, pose, l, meas[i], W[i]) for l in planes] for i in range(3)]
    for i in range(3):
        for k in range(len(planes)):
            J[i, k], r[i, k] = g.eval_factor(fids[i][k], 1)
    assert np.array_equal(g.get_poses(), state[0]) and np.array_equal(g.get_planes(), state[1])
    ref, ref2 = _reference_d2(r, J, pose, planes, S1, blk), _reference_d2(r, J, pose, planes, S2, blk)
    assert d2.shape == ref.shape and np.all(np.isfinite(d2)) and np.all(d2 >= 0)
    e = float(np.max(np.abs(d2 - ref) / ref)); d = float(np.max(np.abs(ref2 - ref) / ref))
    bound = max(16 * d, 1e-12)
    print(f"COVFACTOR gate {name}: M 3 L {len(planes)} e {e:.3e} d {d:.3e} bound {bound:.3e}")
    assert e <= bound, (name, e, d)
    for i in range(3):
        order = np.argsort(ref[i], kind="stable")
        if (ref[i, order[1]] - ref[i, order[0]]) > bound * ref[i, order[0]]:
            assert best[i] == order[0], (name, i, best[i], order[0])
    g.close()


# ---- 4. band graphs: the same bits either way ----------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [lambda: synth.corridor(60, 14, seed=7), lambda: synth.small_world(12, 4, seed=3)], ids=["corridor_60_14", "small_world_12_4"])
def test_band_graph_same_bits_from_either_entry_point_and_either_kernel(built, make):
    def queries(g, rec):
        ids = rec.node_ids()
        poses = [n for n in ids if rec.dims[n] == 6]; planes = [n for n in ids if rec.dims[n] == 3]
        meas, W, _ = _measurements(g, poses[-1], planes, seed=5, steps=(2.5, 40.0))
        out = [g.cov_block(ids[::3]), g.cov_block([poses[0]], [poses[-1]] + planes)]
        assert g.cov_block_last()[1] == 2
        out += list(g.assoc_gate(poses[-1], meas, W, planes))
        assert g.assoc_gate_last()[1] == 2
        return out
    a, ra = _build(make()); b, rb = _build(make())
    a.cov_recover(); b.cov_factor()
    qa, qb = queries(a, ra), queries(b, rb)
    b.debug_cov_path_form(1)
    qw = queries(b, rb)
    a.debug_cov_path_form(1)
    qaw = queries(a, ra)
    for x, y, z, w in zip(qa, qb, qw, qaw):
        assert np.all(np.isfinite(x))
        assert x.tobytes() == y.tobytes() == z.tobytes() == w.tobytes()
    assert np.all(np.isfinite(np.concatenate([m.ravel() for m in a.cov_marginals()])))        # (the full recovery still has its selected inverse)
    a.close(); b.close()


# ---- 5. state -----------------------------------------------------------------------------------------------------------------
def test_factor_alone_refuses_the_selected_inverse_and_ends_with_every_change(built):
    g, rec = _build(synth.small_world(20, 6, seed=2, obs_per_pose=5))
    g.batch_optimize()
    ids = rec.node_ids()
    pose0 = next(n for n in ids if rec.dims[n] == 6); plane0 = next(n for n in ids if rec.dims[n] == 3)
    g.cov_factor()
    first = g.cov_block(ids[::4])
    for read in (lambda: g.cov_marginals(), lambda: g.cov_access([(pose0, plane0)]), lambda: g.cov_joint([pose0, plane0])):
        with pytest.raises(P.PpsError) as e:
            read()
        assert e.value.code == P.PPS_ESTATE and "pps_cov_factor" in str(e.value) and "pps_cov_recover" in str(e.value)
    assert np.array_equal(g.cov_block(ids[::4]), first)                 # (a refused read changes nothing)

    def add():
        p = g.add_pose(g.get_pose(pose0)); g.add_pose_prior(p, np.zeros(6), synth._ut_diag([1.0] * 6))
    changes = {
        "add": add,
        "remove": lambda: rec.remove_factor(max(f for f, (a, b) in rec.factors.items() if b >= 0 and rec.dims[b] == 3)),
        "set": lambda: g.set_pose(pose0, synth.pose_exmap(g.get_pose(pose0), np.array([0.01, 0, 0, 0, 0.01, 0]))),
        "update": g.update,
        "batch_optimize": g.batch_optimize,
        "restore_state": g.restore_state,
        "set_cost_function": lambda: g.set_cost_function(P.COST_NONE),
    }
    g.save_state()
    for name, change in changes.items():
        g.cov_factor()
        assert np.all(np.isfinite(g.cov_block([pose0], [plane0]))), name
        change()
        for read in (lambda: g.cov_block([pose0], [plane0]), lambda: g.cov_marginals([pose0])):
            with pytest.raises(P.PpsError) as e:
                read()
            assert e.value.code == P.PPS_ESTATE and NO_RECOVERY in str(e.value), name
        if name in ("add", "remove"):
            g.save_state()                                              # (a snapshot belongs to one topology)
    g.close()


@pytest.mark.parametrize("make,mode", [(lambda: synth.corridor(60, 14, seed=7), 0), (GRAPHS["dense_48p_150l_10x5"], 1)], ids=["band", "dense"])
def test_batch_optimize_after_the_factor_is_bit_identical(built, make, mode):
    def run(with_factor):
        g = P.Graph(jacobian_mode=mode); ids, _ = make().replay(g)
        if with_factor:
            g.cov_factor(); g.cov_block([int(ids[0])], [int(ids[-1])])
        it = g.batch_optimize(); tr = g.trace(); st = g.stats()
        x = (g.get_poses().copy(), g.get_planes().copy())
        if with_factor:
            g.cov_factor(); g.cov_block([int(i) for i in ids[:5]])
            after = g.stats()
            for k in ("lm_iterations", "chi2_initial", "chi2_final", "lambda_final", "n_linearize", "n_factorize", "n_launches", "t_total"):
                assert after[k] == st[k], k                             # the stats of the last solve stay what they were
            assert g.trace() == tr
            np.testing.assert_array_equal(g.get_poses(), x[0]); np.testing.assert_array_equal(g.get_planes(), x[1])
        g.close()
        return it, tr, x
    a, b = run(False), run(True)
    assert a[0] == b[0] and a[1] == b[1]
    np.testing.assert_array_equal(a[2][0], b[2][0]); np.testing.assert_array_equal(a[2][1], b[2][1])


# ---- 6. not positive definite --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SINGULAR))
def test_graph_without_any_prior_is_not_positive_definite(built, name):
    """(tests/test_host_cov_factor.py asserts on the CPU that H of both graphs, factored in the analysis's order, has a collapsed pivot)"""
    spec = SINGULAR[name]()
    g = P.Graph(jacobian_mode=1); ids, _ = spec.replay(g)
    with pytest.raises(P.PpsError) as e:
        g.cov_factor()
    assert e.value.code == P.PPS_ENOTPD and "positive definite" in str(e.value)
    with pytest.raises(P.PpsError) as e:
        g.cov_block([int(ids[0])])
    assert e.value.code == P.PPS_ESTATE and NO_RECOVERY in str(e.value)
    assert np.isfinite(g.chi2())                                        # the handle goes on working
    g.batch_optimize()
    assert np.isfinite(g.chi2())
    g.close()


# ---- 7. robust cost ------------------------------------------------------------------------------------------------------------
def test_robust_cost_on_a_dense_front_graph(built):
    g, rec, sel = _dense("dense_48p_150l_10x5")
    g.set_cost_function(P.COST_PSEUDO_HUBER, 1.0)
    g.cov_factor()
    queries = [(sel, None), (sel[:3], sel[1:6])]
    got = [g.cov_block(r, c) for r, c in queries]
    _check("dense_48p_150l_10x5 pseudo-Huber b = 1", g, rec, queries, got)      # (pps_eval_factor gives the robustified J)
    g.close()
