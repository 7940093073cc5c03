"""GPU: pps_cov_select -- the selected inverse on dense-front trees (csrc/pps_cov_dense.hip) -- against a dense inverse, against the column
solves of pps_cov_block, and on band graphs against pps_cov_recover.

Reference: H = sum J'J assembled in numpy from pps_eval_factor of every factor, inverted twice (cov_helpers.cpu_inverses).  e and d as in
tests/test_gpu_cov_block.py (per node pair, |M - M0|_F / sqrt(|S0(r, r)|_F |S0(c, c)|_F); d the same between the two CPU inverses, maximum
over the same blocks); bound e <= max(16 d, 1e-12).  One `COVSEL <graph>: e ... d ...` line per graph (-s).

After cov_select: every diagonal block (symmetric bit for bit, positive diagonal), every factor-joined pair through cov_access in both
orders, one cov_joint of three nodes that share the widest front.  The whole sphere2500 has no dense inverse to compare with: there the
diagonal blocks of about twelve nodes spread over the tree are compared with cov_block of the same handle -- an independent route over
the same factor -- under the same rule, with d taken from the truncated graph's run.
"""
import os

import numpy as np
import pytest

import pop_up_slam_amd as P
from cov_block_helpers import block_err
from cov_factor_helpers import DENSE, GRAPHS, choose_nodes
from cov_helpers import factor_pairs
from linsolve_helpers import assert_case_shapes, spec_layout
from pop_up_slam_amd import graphio, synth
from test_gpu_cov import _build, _reference
from test_gpu_cov_block import _errors
from test_host_cov_factor import SINGULAR

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SPHERE = os.path.join(HERE, "golden", "isam_data", "sphere2500.txt")
NO_RECOVERY = "no valid covariance recovery"
D_TRUNCATED = {}                                            # d of the sphere2500_1400 run, for the whole graph's comparison


def _front_nodes(A, lay, s):
    """the nodes whose scalars are rows of front s, pivots first"""
    po, p = int(A["f_poff"][s]), int(A["f_p"][s])
    rows = [int(v) for v in A["pidx"][po:po + p]] + [int(v) for v in A["bidx"][A["f_bidx_off"][s]:A["f_bidx_off"][s + 1]]]
    at = {lay[n][0]: n for n in lay}
    return [at[v] for v in rows if v in at]


def _check(label, g, rec, spec, A, mode=1):
    """all marginals, all factor-joined pairs in both orders, a joint of three nodes of the widest front; returns (e, d)"""
    ids = rec.node_ids()
    marg = g.cov_marginals()                               # (read BEFORE pps_eval_factor runs: that call moves the linearisation point)
    pairs = factor_pairs(list(rec.factors.values()))
    pairs = pairs + [(b, a) for a, b in pairs]
    cross = g.cov_access(pairs)
    lay = spec_layout(spec, A)
    widest = max(range(A["n_fronts"]), key=lambda s: int(A["f_p"][s]) + int(A["f_b"][s]))
    members = _front_nodes(A, lay, widest)
    group = [members[0], members[len(members) // 2], members[-1]]
    assert len(set(group)) == 3
    joint = g.cov_joint(group)
    S1, S2, blk = _reference(g, rec, mode)
    e = d = 0.0
    for n, M in zip(ids, marg):
        assert M.shape == (rec.dims[n],) * 2 and np.all(np.isfinite(M)), (label, n)
        assert np.array_equal(M, M.T), (label, n, "diagonal block not symmetric bit for bit")
        assert np.all(np.diag(M) > 0), (label, n)
        eq, dq = _errors(M, [n], [n], rec, S1, S2, blk); e, d = max(e, eq), max(d, dq)
    for (r, c), M in zip(pairs, cross):
        assert M is not None, (label, r, c, "a factor-joined pair must be in the pattern")
        eq, dq = _errors(M, [r], [c], rec, S1, S2, blk); e, d = max(e, eq), max(d, dq)
    assert np.array_equal(joint, joint.T)
    eq, dq = _errors(joint, group, group, rec, S1, S2, blk); e, d = max(e, eq), max(d, dq)
    assert np.array_equal(joint[:rec.dims[group[0]], :rec.dims[group[0]]], marg[ids.index(group[0])])
    print(f"COVSEL {label}: nodes {len(ids)} blocks {len(ids) + len(pairs)} max front {A['max_front']} e {e:.3e} d {d:.3e} bound {max(16 * d, 1e-12):.3e}")
    assert e <= max(16 * d, 1e-12), (label, e, d)
    return e, d


def _dense(name, **props):
    spec = GRAPHS[name]()
    g, rec = _build(spec, jacobian_mode=1, **props)
    g.analyze()
    A = g.analysis_dump()
    if name in DENSE:
        assert_case_shapes(name, A)
    assert A["max_front"] > 127
    return g, rec, spec, A


# ---- 1. dense graphs against the dense inverse ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GRAPHS))
def test_dense_front_selected_inverse_against_the_dense_inverse(built, name):
    g, rec, spec, A = _dense(name)
    g.cov_select()
    t = g.cov_last_times()
    assert t[0] > t[1] > 0
    _check(name, g, rec, spec, A)
    g.close()


# ---- 2. sphere2500 ------------------------------------------------------------------------------------------------------------
def test_sphere2500_truncated_against_the_dense_inverse(built):
    spec = graphio.load_edge3_log(SPHERE, max_lines=1400)
    g, rec = _build(spec, jacobian_mode=1)
    g.analyze()
    A = g.analysis_dump()
    assert A["max_front"] > 127
    g.batch_optimize()
    g.cov_select()
    D_TRUNCATED["d"] = _check("sphere2500_1400", g, rec, spec, A)[1]
    g.close()


def test_sphere2500_whole_against_the_column_solves(built):
    if "d" not in D_TRUNCATED:
        test_sphere2500_truncated_against_the_dense_inverse(built)
    spec = graphio.load_edge3_log(SPHERE)
    g, rec = _build(spec, jacobian_mode=1)
    g.batch_optimize()
    A = g.analysis_dump()
    assert A["max_front"] > 127 and len(rec.node_ids()) == 2500
    sel = choose_nodes(A, spec_layout(spec, A))
    g.cov_select()
    marg = g.cov_marginals(sel)
    e = 0.0
    for n, M in zip(sel, marg):
        ref = g.cov_block([n])
        assert np.array_equal(M, M.T) and np.all(np.diag(M) > 0)
        e = max(e, block_err(M, ref, ref, ref))
    d = D_TRUNCATED["d"]
    print(f"COVSEL sphere2500: nodes {len(sel)} of 2500, max front {A['max_front']} levels {A['n_levels']} e {e:.3e} (against cov_block) d {d:.3e} (sphere2500_1400) "
          f"bound {max(16 * d, 1e-12):.3e}; cov_select {g.cov_last_times()[0] * 1e3:.2f} ms, pass {g.cov_last_times()[1] * 1e3:.2f} ms")
    assert e <= max(16 * d, 1e-12), (e, d)
    g.close()


# ---- 3. the forced form on band graphs -----------------------------------------------------------------------------------------
BAND = {"corridor_60_14": lambda: synth.corridor(60, 14, seed=7), "small_world_12_4": lambda: synth.small_world(12, 4, seed=3)}


@pytest.mark.parametrize("name", sorted(BAND))
def test_dense_pass_forced_onto_a_band_graph_against_the_recovery(built, name):
    g, rec = _build(BAND[name]())
    g.analyze()
    assert g.stats()["max_front"] <= 127
    ids = rec.node_ids()
    pairs = factor_pairs(list(rec.factors.values()))
    pairs = pairs + [(b, a) for a, b in pairs]
    g.cov_recover()
    m0, c0 = g.cov_marginals(), g.cov_access(pairs)
    g.cov_select()                                          # without the switch: pps_cov_recover, bit for bit
    m1, c1 = g.cov_marginals(), g.cov_access(pairs)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(m0 + c0, m1 + c1))
    g.debug_cov_select_form(1)
    g.cov_select()
    m2, c2 = g.cov_marginals(), g.cov_access(pairs)
    # the recovery differs from the dense inverse by about what two CPU inverses differ by (tests/test_gpu_cov.py); the MFMA sums differ
    # in order from its FMA loops, so the yardstick is d of this graph's H and no bit equality is asked
    S1, S2, blk = _reference(g, rec, 0)
    e = d = 0.0
    for n, A0, A2 in zip(ids, m0, m2):
        assert np.array_equal(A2, A2.T)
        e = max(e, block_err(A2, A0, blk(S1, n, n), blk(S1, n, n))); d = max(d, block_err(blk(S2, n, n), blk(S1, n, n), blk(S1, n, n), blk(S1, n, n)))
    for (r, c), A0, A2 in zip(pairs, c0, c2):
        assert A0 is not None and A2 is not None
        e = max(e, block_err(A2, A0, blk(S1, r, r), blk(S1, c, c))); d = max(d, block_err(blk(S2, r, c), blk(S1, r, c), blk(S1, r, r), blk(S1, c, c)))
    print(f"COVSEL forced {name}: blocks {len(ids) + len(pairs)} e {e:.3e} (against cov_recover) d {d:.3e} bound {max(16 * d, 1e-12):.3e}")
    assert e <= max(16 * d, 1e-12), (name, e, d)
    g.debug_cov_select_form(0)
    g.cov_select()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(m0, g.cov_marginals()))
    g.close()


# ---- 4. state -----------------------------------------------------------------------------------------------------------------
def test_state_of_a_selection_on_a_dense_front_graph(built):
    g, rec, spec, A = _dense("dense_48p_150l_10x5")
    ids = rec.node_ids()
    pose0 = next(n for n in ids if rec.dims[n] == 6); plane0 = next(n for n in ids if rec.dims[n] == 3)
    obs = next(f for f, (a, b) in rec.factors.items() if b >= 0 and rec.dims[b] == 3)
    g.cov_select()
    first = np.concatenate([m.ravel() for m in g.cov_marginals()])
    blk = g.cov_block([pose0], [plane0])                    # the factor is held as after pps_cov_factor
    g.cov_select()
    assert np.concatenate([m.ravel() for m in g.cov_marginals()]).tobytes() == first.tobytes()      # the same state, the same bits
    assert g.cov_block([pose0], [plane0]).tobytes() == blk.tobytes()
    reads = (lambda: g.cov_marginals(), lambda: g.cov_access([(pose0, pose0)]), lambda: g.cov_joint([pose0]))
    g.cov_factor()                                          # the factor alone: the selection is gone, the text names both calls
    for read in reads:
        with pytest.raises(P.PpsError) as e:
            read()
        assert e.value.code == P.PPS_ESTATE and "pps_cov_factor" in str(e.value) and "pps_cov_recover" in str(e.value)
    assert g.cov_block([pose0], [plane0]).tobytes() == blk.tobytes()
    g.cov_select()
    with pytest.raises(P.PpsError) as e:                    # the full recovery still refuses the graph, and ends the selection
        g.cov_recover()
    assert e.value.code == P.PPS_ESTATE and "dense-front" in str(e.value)
    for read in reads + (lambda: g.cov_block([pose0]),):
        with pytest.raises(P.PpsError) as e:
            read()
        assert e.value.code == P.PPS_ESTATE and NO_RECOVERY in str(e.value)

    def add():
        p = g.add_pose(g.get_pose(pose0)); g.add_pose_prior(p, np.zeros(6), synth._ut_diag([1.0] * 6))
    changes = {
        "set_pose": lambda: g.set_pose(pose0, synth.pose_exmap(g.get_pose(pose0), np.array([0.01, 0, 0, 0, 0.01, 0]))),
        "set_plane": lambda: g.set_plane(plane0, synth.plane_exmap(g.get_plane(plane0), np.array([0.01, -0.01, 0.02]))),
        "set_measurement": lambda: g.set_measurement(obs, synth.plane_exmap(g.get_measurement(obs), np.array([0.02, -0.01, 0.03]))),
        "update": g.update,
        "batch_optimize": g.batch_optimize,
        "restore_state": g.restore_state,
        "refresh_measurements": g.refresh_measurements,
        "set_cost_function": lambda: g.set_cost_function(P.COST_NONE),
        "remove_factor": lambda: rec.remove_factor(max(f for f, (a, b) in rec.factors.items() if b >= 0 and rec.dims[b] == 3)),
        "add": add,
    }
    g.save_state()
    for name, change in changes.items():
        g.cov_select()
        assert len(g.cov_marginals()) == len(rec.node_ids()), name
        change()
        for read in reads + (lambda: g.cov_block([pose0]),):
            with pytest.raises(P.PpsError) as e:
                read()
            assert e.value.code == P.PPS_ESTATE and NO_RECOVERY in str(e.value), name
        if name in ("add", "remove_factor"):
            g.save_state()                                  # (a snapshot belongs to one topology)
    g.cov_select()                                          # ... and a new selection sees the new state
    assert all(np.all(np.isfinite(m)) and np.all(np.diag(m) > 0) for m in g.cov_marginals())
    g.close()


def test_batch_optimize_after_the_selection_is_bit_identical(built):
    make = GRAPHS["dense_48p_150l_10x5"]

    def run(with_select):
        g = P.Graph(jacobian_mode=1); ids, _ = make().replay(g)
        if with_select:
            g.cov_select(); g.cov_marginals([int(ids[0])])
        it = g.batch_optimize(); tr = g.trace(); st = g.stats()
        x = (g.get_poses().copy(), g.get_planes().copy())
        if with_select:
            g.cov_select(); g.cov_marginals()
            after = g.stats()
            for k in ("lm_iterations", "chi2_initial", "chi2_final", "lambda_final", "n_linearize", "n_factorize", "n_launches", "t_total"):
                assert after[k] == st[k], k                 # the stats of the last solve stay what they were
            assert g.trace() == tr
            np.testing.assert_array_equal(g.get_poses(), x[0]); np.testing.assert_array_equal(g.get_planes(), x[1])
        g.close()
        return it, tr, x
    a, b = run(False), run(True)
    assert a[0] == b[0] and a[1] == b[1]
    np.testing.assert_array_equal(a[2][0], b[2][0]); np.testing.assert_array_equal(a[2][1], b[2][1])


# ---- 5. not positive definite, robust cost -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SINGULAR))
def test_graph_without_any_prior_is_not_positive_definite(built, name):
    """(tests/test_host_cov_factor.py asserts on the CPU that H of both graphs, factored in the analysis's order, has a collapsed pivot)"""
    spec = SINGULAR[name]()
    g = P.Graph(jacobian_mode=1); ids, _ = spec.replay(g)
    before = (g.get_poses().copy(), g.get_planes().copy())
    g.debug_cov_select_form(1)                              # (the band graph of the two takes the dense-front pass as well)
    with pytest.raises(P.PpsError) as e:
        g.cov_select()
    assert e.value.code == P.PPS_ENOTPD and "positive definite" in str(e.value)
    for read in (lambda: g.cov_marginals(), lambda: g.cov_block([int(ids[0])])):
        with pytest.raises(P.PpsError) as e:
            read()
        assert e.value.code == P.PPS_ESTATE and NO_RECOVERY in str(e.value)
    np.testing.assert_array_equal(g.get_poses(), before[0]); np.testing.assert_array_equal(g.get_planes(), before[1])
    assert np.isfinite(g.chi2())                            # the handle goes on working
    g.batch_optimize()
    assert np.isfinite(g.chi2())
    g.close()


def test_robust_cost_on_a_dense_front_graph(built):
    g, rec, spec, A = _dense("dense_48p_150l_10x5")
    g.set_cost_function(P.COST_PSEUDO_HUBER, 1.0)
    g.cov_select()
    _check("dense_48p_150l_10x5 pseudo-Huber b = 1", g, rec, spec, A)      # (pps_eval_factor gives the robustified J)
    g.close()
