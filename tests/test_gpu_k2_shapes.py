"""GPU: K2's normal equations (csrc/pps_k2.hip) at every block shape where its control flow changes, and in every form.

B. The solved step delta (pps_debug_solve) against a CPU solve of the same normal equations, with the yardstick of
   tests/linsolve_helpers.py: J and r of every factor from pps_eval_factor, H = sum J'J and b = -sum J'r in float64, H + lambda diag(H),
   two CPU solves that share no code path, d = |x1 - x2| / |x1|, and the device passes with e <= max(16 d, 1e-12) for the whole step and
   for every node block.  The cases (tests/k2_shape_helpers.py) are a landmark of 16, 17, 24 and 33 segments (one chunk of sixteen; a
   second chunk and k_hfinish; a last chunk of eight; three chunks), a pose block with a second and a third batch of product records, a
   pose block of exactly 64 and of 65 contributions (one segment, two), and Factor2 edges -- Jacobian slices -- in segments that also
   hold product records.  The small cases take the dense reference unchanged; the ground_* cases (6 700 .. 13 500 unknowns) a sparse
   H, d from SuperLU with partial pivoting under two column orderings (COLAMD, MMD on A' + A), and the step compared with a third solve,
   SuperLU's symmetric mode, because the errors of the two pivoting solves sit in a few node blocks and reach 16 d there themselves
   (KS.sparse_reference_solves; pinned by an extended-precision refinement in tests/test_host_k2_shapes.py).  Three cases are repeated
   with the thread-per-factor K1, behind which K2 multiplies Jacobian slices for every contribution.
C. Every other form of K2 gives the bits of the form pinned in B: one batch of long, short and Factor2 graphs in the default batch
   kernels (kb_hblocks2, kb_hfinish, kb_linearize_repop) and in the throughput forms (kb_hblocks_tc / kb_hblocks_tg / kb_hreduce)
   against single handles -- iteration count, LM trace, chi2 and state equal bit for bit.  (Before kb_hreduce added a block of more
   than 16 segments chunk by chunk, the throughput run differed in the last bits for the 17- and the 33-segment graph.)
D. The wave boundaries of k_linearize_repop: 64, 128 and 129 Factor2 edges against the one-factor evaluations.

Every case first asserts -- from the analysis alone -- that its graph has the block shapes it exists for.  cond(H_lambda), d, e and form
are printed per case and lambda (run with -s).
"""
import numpy as np
import pytest

import pop_up_slam_amd as P
import k2_shape_helpers as KS
import linsolve_helpers as LH
from oracle import oracle_py as O
from pop_up_slam_amd import synth

pytestmark = pytest.mark.gpu

SINGLE = [(name, mode) for name in KS.CASE_ORDER for mode in KS.CASES[name][3]]
_IDS = lambda cm: f"{cm[0]}-jac{cm[1]}"
_CTX, _REF = {}, {}


class Ref:
    """the normal equations of one (graph, Jacobian mode) at the initial estimate and their CPU solves per damping value: computed
    once from the one-factor evaluations of a handle, shared by the tests, never modified"""

    def __init__(self, g, spec, A, mode, dense):
        self.dense = dense
        self.H, self.b, self.lay = (LH.assemble_normal_equations if dense else KS.assemble_sparse)(g, spec, A, mode)
        self.b.setflags(write=False)
        self.chi2 = float(sum(float(r @ r) for r in (g.eval_factor(int(fid), mode)[1] for fid in range(len(spec.f_type)))))
        self.solves = {}

    def solve(self, lam):
        if lam not in self.solves:
            if self.dense:
                Hl = LH.damped(self.H, lam)
                refs, cond = LH.reference_solves(Hl, self.b), LH.cond_spd(Hl)
            else:
                Hl = KS.damped_sparse(self.H, lam)
                refs, cond = KS.sparse_reference_solves(Hl, self.b), None
            for v in refs[:-1]:
                v.setflags(write=False)
            self.solves[lam] = (Hl, refs, cond)
        return self.solves[lam]

    def check(self, label, delta, lam, form):
        Hl, refs, cond = self.solve(lam)
        if self.dense:
            return LH.check_step(label, delta, Hl, self.b, self.lay, form, refs, cond)
        return KS.check_step_sparse(label, delta, refs, self.lay, form)


class Ctx:
    """one handle per (case, Jacobian mode, K1 form) that stays at its initial estimate, with its analysis; the reference is shared
    between the K1 forms (pps_eval_factor is the same one-factor evaluation behind both)"""

    def __init__(self, name, mode, thread_form):
        self.name, self.mode, self.thread_form = name, mode, thread_form
        self.spec = KS.make(name)
        self.g = P.Graph(jacobian_mode=mode)
        self.spec.replay(self.g)
        self.g.analyze()
        self.A = self.g.analysis_dump()
        KS.assert_case_shapes(name, self.A, self.spec)
        if (name, mode) not in _REF:
            dense = KS.CASES[name][4] if name in KS.CASES else True
            _REF[(name, mode)] = Ref(self.g, self.spec, self.A, mode, dense)
        self.ref = _REF[(name, mode)]
        self.label = f"{name} jac {mode}" + (" K1 thread form" if thread_form else "")


def _ctx(name, mode, thread_form=False):
    """(a thread-form context is made by a test that has set PPS_K1_THREAD_FORM: the library reads its switches once per handle)"""
    if (name, mode, thread_form) not in _CTX:
        _CTX[(name, mode, thread_form)] = Ctx(name, mode, thread_form)
    return _CTX[(name, mode, thread_form)]


def _state(g):
    return g.chi2(), g.get_poses().copy(), g.get_planes().copy()


def _same_state(a, b):
    assert a[0] == b[0]
    np.testing.assert_array_equal(a[1], b[1]); np.testing.assert_array_equal(a[2], b[2])


def _check_steps(c, lambdas):
    g = c.g
    for lam in lambdas:
        before = _state(g)
        delta, delta2, form, bad = g.debug_solve(lam)
        assert delta2 is None and len(delta) == c.A["n_scalars"]
        assert form in (0, 1, 2), (c.label, "K3 form", form)
        assert bad == 0.0, (c.label, "not_pd", bad)
        c.ref.check(f"{c.label} lambda {lam:g}", delta, lam, form)
        _same_state(before, _state(g))                                 # the hook leaves the estimate alone, bit for bit


# ---- B ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_mode", SINGLE, ids=_IDS)
def test_step_against_the_reference_at_every_block_shape(built, case_mode):
    name, mode = case_mode
    _check_steps(_ctx(name, mode), KS.CASES[name][2])


@pytest.mark.parametrize("name", KS.THREAD_FORM)
def test_step_with_jacobian_slices_for_every_contribution(built, monkeypatch, name):
    """PPS_K1_THREAD_FORM=1: K1 writes no product records, K2 multiplies the Jacobian slices of every contribution (d.P == nullptr) and
    meets the same counts"""
    _ctx(name, 1)                                                      # (the reference, from a handle of the default form)
    monkeypatch.setenv("PPS_K1_THREAD_FORM", "1")
    _check_steps(_ctx(name, 1, True), KS.CASES[name][2])


# ---- C ---------------------------------------------------------------------------------------------------------------------
# (pose_65 itself cannot join a batch: 63 planes seen from one pose make a front of 195 rows, beyond the wave-per-front kernels, and
# pps_multi refuses such a graph -- test_multi_refuses_the_dense_front_case.  pose_65_repeat has the same two-segment pose block, from one
# pose that sees its five walls many times, in fronts of at most 57 rows.)
BATCH = ("ground_17seg", "ground_33seg", "pose_65_repeat", "mixed_repop_129", "repop_64", "repop_128")
ORACLE = ("mixed_repop_129", "pose_65_repeat")
_ORACLE = {}


def _oracle(name, mode):
    if (name, mode) not in _ORACLE:
        o = O.OracleGraph(analytic=mode); KS.make(name).replay(o)
        _ORACLE[(name, mode)] = (o.batch_optimize(), o.chi2())
    return _ORACLE[(name, mode)]


def _build(specs, mode):
    gs = []
    for sp in specs:
        g = P.Graph(jacobian_mode=mode); sp.replay(g); gs.append(g)
    return gs


@pytest.mark.parametrize("forms", ["batch", "throughput"])
@pytest.mark.parametrize("mode", [P.JAC_NUMERIC, P.JAC_ANALYTIC])
def test_batch_forms_give_the_bits_of_the_single_handles(built, monkeypatch, mode, forms):
    """Long blocks (17 and 33 segments: kb_hfinish / the chunks of kb_hreduce), a two-segment pose block, 64 / 128 / 129 Factor2 edges
    (kb_linearize_repop) and a graph with neither (the launch is wider than it needs) in one batch: per graph the iteration count, the LM
    trace, chi2 and the state of its own pps_batch_optimize, bit for bit.  "throughput": the singles run the thread-per-factor K1 with
    the ordinary K2 over Jacobian slices, the batch K1's thread form, K2's LDS-staged class kernels with kb_hreduce, and K3's level form."""
    specs = [KS.make(n) for n in BATCH] + [synth.small_world(20, 6, seed=2)]
    names = list(BATCH) + ["small_world_20_6"]
    if forms == "throughput":
        monkeypatch.setenv("PPS_K1_THREAD_FORM", "1")
    singles = _build(specs, mode)
    for g, n in zip(singles, names):
        if n in KS.CASES or n in KS.BATCH_ONLY:
            g.analyze(); KS.assert_case_shapes(n, g.analysis_dump(), KS.make(n))
    ref = []
    for g in singles:
        it = g.batch_optimize()
        ref.append((it, g.trace(), g.chi2(), g.get_poses().copy(), g.get_planes().copy()))
    if forms == "throughput":
        monkeypatch.setenv("PPS_MULTI_THREAD_FORM", "1")
        monkeypatch.setenv("PPS_MULTI_LEVELS", "1")
    batch = _build(specs, mode)
    its, st = P.Multi(batch).optimize()
    assert np.all(st == 0)
    bad = []
    for k, g in enumerate(batch):
        it, tr, c, poses, planes = ref[k]
        same = (its[k] == it and g.trace() == tr and g.chi2() == c and np.array_equal(g.get_poses(), poses)
                and np.array_equal(g.get_planes(), planes))
        print(f"K2FORMS {forms} jac {mode} {names[k]}: {it} iterations, chi2 {c:.17g} single / {g.chi2():.17g} batch, {'same bits' if same else 'DIFFERENT'}")
        if not same:
            bad.append(names[k])
    assert not bad, (forms, mode, bad)
    for n in ORACLE:
        k = names.index(n)
        ito, co = _oracle(n, mode)
        assert ito == ref[k][0] and abs(co - ref[k][2]) <= 1e-7 * ref[k][2], (n, ito, ref[k][0], co, ref[k][2])
    for g in singles + batch:
        g.close()


def test_multi_refuses_the_dense_front_case(built):
    """pose_65 has fronts beyond 127 rows: the batched solve says so (PPS_ESTATE) and leaves the handle as it was"""
    g = _build([KS.make("pose_65")], P.JAC_ANALYTIC)[0]
    g.analyze()
    assert g.analysis_dump()["max_front"] > 127
    c0 = g.chi2()
    with pytest.raises(P.PpsError) as e:
        P.Multi([g]).optimize()
    assert e.value.code == P.PPS_ESTATE
    assert g.chi2() == c0
    # ... and its own handle solves it: the oracle's trial count and chi2
    it, c = g.batch_optimize(), g.chi2()
    ito, co = _oracle("pose_65", P.JAC_ANALYTIC)
    assert ito == it and abs(co - c) <= 1e-7 * c, (ito, it, co, c)
    g.close()


def test_step_of_the_band_form_two_segment_pose_block(built):
    """pose_65_repeat (the stand-in for pose_65 in the batch) against the dense reference on its own"""
    _check_steps(_ctx("pose_65_repeat", 1), LH.LAMBDAS)


# ---- D ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["repop_64", "repop_128", "mixed_repop_129"])
def test_factor2_wave_boundaries(built, name):
    """64, 128 and 129 Factor2 edges: the full-graph launch of k_linearize_repop (blocks 0, 1 and 2; a last wave with one live lane,
    its clamped lanes and its staged flush) against the one-factor evaluations -- the step at lambda = 1e-3 against the dense reference
    assembled from them, and chi2, whose kernel re-pops across the boundary between fixed and Factor2 slots inside one block, against
    the sum of |r|^2"""
    c = _ctx(name, 1)
    assert int(c.spec.f_repop.sum()) == int(name.rsplit("_", 1)[1])
    _check_steps(c, (1e-3,))
    chi2 = c.g.chi2()
    print(f"K2SHAPES {name}: chi2 {chi2:.17g} sum |r|^2 {c.ref.chi2:.17g}")
    assert abs(chi2 - c.ref.chi2) <= 1e-12 * c.ref.chi2
