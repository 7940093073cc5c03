"""CPU: what tests/test_gpu_k2_shapes.py stands on, checked without a device -- the block shapes every case of it exists for (a change of
the ordering or of seg_len is caught on every machine), the contribution lists of the small cases through the numpy emulation of
tests/mf_emulator.py (diagonal H blocks summed from the product records, as K2 does), and the sparse reference against the dense one."""
import numpy as np
import pytest

import pop_up_slam_amd as P
import k2_shape_helpers as KS
import linsolve_helpers as LH
from mf_emulator import solve_with_analysis, solve_with_band_schedule
from oracle import oracle_py as O
from pop_up_slam_amd import synth


def _analysis(name):
    spec = KS.make(name)
    g = P.Graph(jacobian_mode=1); spec.replay(g); g.analyze()
    A = g.analysis_dump()
    g.close()
    return spec, A


@pytest.mark.parametrize("case", KS.CASE_ORDER + list(KS.BATCH_ONLY))
def test_case_graph_has_the_block_shapes_it_exists_for(built, case):
    spec, A = _analysis(case)
    KS.assert_case_shapes(case, A, spec)
    lay = LH.spec_layout(spec, A)
    covered = np.sort(np.concatenate([np.arange(o, o + dim) for o, dim in lay.values()]))
    assert np.array_equal(covered, np.arange(A["n_scalars"]))         # node_voff tiles delta: the reference is indexed by it


def test_contracts_refuse_the_neighbouring_shapes(built):
    """a contract that any graph passes pins nothing: each one refuses the graph of the case next to it"""
    for case, other in (("ground_16seg", "ground_17seg"), ("ground_17seg", "ground_16seg"), ("pose_18", "pose_34"), ("pose_34", "pose_18"),
                        ("pose_64", "pose_65"), ("pose_65", "pose_64"), ("mixed_repop_129", "repop_128")):
        spec, A = _analysis(other)
        with pytest.raises(AssertionError):
            KS.assert_case_shapes(case, A, spec)
    spec, A = _analysis("pose_18")                                      # no Factor2 edge at all: no mix
    plain = KS.RepopSpec(**{**spec.__dict__, "f_repop": np.zeros(len(spec.f_type), dtype=bool), "f_ray": np.zeros((len(spec.f_type), 6))})
    with pytest.raises(AssertionError):
        KS.CASES["mixed_repop_129"][1](A, plain)


def test_repop_corridor_edges(built):
    """the Factor2 graphs: exact edge counts (one wave, two waves, two waves and one lane of k_linearize_repop), rays that re-pop the
    wall they were drawn on, the device's and the oracle's ray arithmetic agree, and the generator is deterministic"""
    for name, n in (("repop_64", 64), ("repop_128", 128), ("mixed_repop_129", 129)):
        spec = KS.make(name)
        assert int(spec.f_repop.sum()) == n and np.all(spec.f_type[spec.f_repop] == synth.F_PLANE_OBS)
        assert (spec.f_type == synth.F_PLANE_PRIOR).sum() == 4             # the ground's and three walls'
        for k in np.where(spec.f_repop)[0]:
            a, b = spec.f_nodes[k]
            m = O.repop_wall_plane(spec.truth[a], spec.f_ray[k])
            want = synth.plane_transform_to(spec.truth[b, :4], spec.truth[a])
            assert min(np.abs(m - want).max(), np.abs(m + want).max()) < 2e-2, (name, k, m, want)   # (half a pixel of noise at 2 .. 4 m)
    again = KS.repop_corridor(129, edge_ray=lambda k, s: O.edge_ray(k, s))
    np.testing.assert_array_equal(again.f_ray, KS.make("mixed_repop_129").f_ray)
    np.testing.assert_array_equal(again.f_repop, KS.make("mixed_repop_129").f_repop)


@pytest.mark.parametrize("case", KS.SMALL)
@pytest.mark.parametrize("lam", [0.0, 1e-3])
def test_contribution_lists_of_the_small_cases_solve_the_normal_equations(built, case, lam):
    """tests/test_host_analysis.py's emulation at the block shapes of this file: the band schedule with the diagonal H blocks summed
    from the product records, as K2 does, against a dense solve of the same damped normal equations"""
    spec, A = _analysis(case)
    o = O.OracleGraph(analytic=1); spec.replay(o)
    Jbuf, Pbuf, J, rhs, starts, dims = KS.jbuf_and_pbuf(spec, A, o)
    H = J.T @ J; H[np.diag_indices(len(H))] *= (1 + lam)
    dref = np.linalg.solve(H, J.T @ rhs)
    # (the band kernels' arrays exist up to 127 rows per front: pose_34 and the cases beyond it have dense fronts and take the emulation of
    # the level-per-launch arrays -- K2's lists are the same in both)
    solver = solve_with_band_schedule if A["max_front"] <= 127 else solve_with_analysis
    for label, pbuf in (("Jacobian slices", None), ("product records", Pbuf)):
        d = solver(A, Jbuf, lam, pbuf)
        dm = np.zeros_like(dref)
        for i in range(len(dims)):
            c = A["node_compact"][i]
            dm[starts[i]:starts[i] + dims[i]] = d[A["node_voff"][c]:A["node_voff"][c] + dims[i]]
        assert np.abs(dm - dref).max() <= 1e-9 * np.abs(dref).max(), (case, label)


def test_sparse_reference_against_the_dense_one():
    """the sparse assembly's damping and the SuperLU solves against LH.damped / LH.reference_solves on a matrix small enough for both"""
    from scipy import sparse
    rng = np.random.default_rng(5)
    n = 40
    N = 6 * n
    H = np.zeros((N, N)); b = rng.normal(size=N)
    for a in range(n):
        for c in {a, min(a + 1, n - 1), int(rng.integers(0, n))}:
            cols = list(range(6 * a, 6 * a + 6)) + (list(range(6 * c, 6 * c + 6)) if c != a else [])
            J = rng.normal(size=(6, len(cols)))
            H[np.ix_(cols, cols)] += J.T @ J
    Hs = sparse.csc_matrix(H)
    lay = {k: (6 * k, 6) for k in range(n)}
    for lam in LH.LAMBDAS:
        Hl = LH.damped(H, lam)
        assert np.array_equal(KS.damped_sparse(Hs, lam).toarray(), Hl)
        x1, x2, d = LH.reference_solves(Hl, b)
        refs = KS.sparse_reference_solves(KS.damped_sparse(Hs, lam), b)
        s0, s1, s2, ds = refs
        assert 0.0 <= ds < 1e-9 and d < 1e-9
        for v in (s0, s1, s2):
            assert np.linalg.norm(v - x1) / np.linalg.norm(x1) <= max(16.0 * d, 1e-12)
        KS.check_step_sparse(f"sparse reference lambda {lam:g}", x2, refs, lay, -1)
        wrong = s0.copy(); wrong[6 * 17 + 4] += 1e-6 * np.max(np.abs(s0))
        with pytest.raises(AssertionError):
            KS.check_step_sparse("one wrong block", wrong, refs, lay, -1)
        with pytest.raises(AssertionError):
            KS.check_step_sparse("wrong sign", -s0, refs, lay, -1)


@pytest.mark.parametrize("lam", [0.0, 1e-3])
def test_sparse_reference_against_extended_precision(built, lam):
    """ground_17seg (H from the oracle's Jacobians: no device): the solve a device step is compared with is within the bound of an
    extended-precision refinement, whole vector and per node block -- and one contribution lost from the 1 025 of the ground block moves the
    step far beyond that bound, so the bound can see what the ground_* cases are about"""
    spec, A = _analysis("ground_17seg")
    o = O.OracleGraph(analytic=1); spec.replay(o)

    class OracleEval:
        def eval_factor(self, fid, mode):
            return o.factor_jacobian(fid, 1)

    H, b, lay = KS.assemble_sparse(OracleEval(), spec, A, 1)
    Hl = KS.damped_sparse(H, lam)
    refs = KS.sparse_reference_solves(Hl, b)
    x0, x1, x2, d = refs
    xt, sizes = KS.refine_extended(Hl, b, x0)
    xt = np.asarray(xt, dtype=np.float64)
    bound = max(16.0 * d, 1e-12)
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps        # (the third opinion is a wider format)
    assert sizes[-1] <= 1e-3 * bound, sizes                              # ... and has settled far below what it is used to judge
    e0, eb0, _ = LH.step_errors(x0, xt, lay)
    for label, v in (("COLAMD", x1), ("MMD_AT_PLUS_A", x2)):
        e, eb, _ = LH.step_errors(v, xt, lay)
        print(f"LINSOLVE sparse reference lambda {lam:g} {label}: against the refinement {e:.3e} / node block {eb:.3e}")
    print(f"LINSOLVE sparse reference lambda {lam:g} symmetric mode: against the refinement {e0:.3e} / node block {eb0:.3e}; d {d:.3e} bound {bound:.3e}")
    assert 0.0 < d < (1e-7 if lam == 0.0 else 1e-10)
    assert e0 <= bound / 16.0 and eb0 <= bound / 16.0
    KS.check_step_sparse(f"the refinement, lambda {lam:g}", xt, refs, lay, -1)
    # the last plain observation of the ground left out of H and b
    ground = int(np.where(spec.node_type == synth.NODE_PLANE)[0][0])
    k = int(np.where((spec.f_type == synth.F_PLANE_OBS) & (spec.f_nodes[:, 1] == ground))[0][-1])
    J, r = o.factor_jacobian(k, 1)
    cols = np.arange(lay[ground][0], lay[ground][0] + 3)
    from scipy import sparse
    Jg = J[:, 6:]
    Hm = (H - sparse.coo_matrix(((Jg.T @ Jg).ravel(), (np.repeat(cols, 3), np.tile(cols, 3))), shape=H.shape)).tocsc()
    bm = b.copy(); bm[cols] += Jg.T @ r
    lost = KS.sparse_reference_solves(KS.damped_sparse(Hm, lam), bm)[0]
    e, eb, _ = LH.step_errors(lost, x0, lay)
    print(f"LINSOLVE sparse reference lambda {lam:g}: one ground contribution of 1 025 lost moves the step by {e:.3e} / node block {eb:.3e}")
    assert e > (100.0 if lam > 0.0 else 1.0) * bound                      # (at lambda = 0 the chain is badly conditioned and the bound loose: the damped solves carry the weight)
