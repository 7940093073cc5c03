"""GPU: pps_loop_gate -- d2 = r' (I + Jw Sigma Jw')^-1 r of candidate odometry factors between existing poses, S, and the candidates below a
threshold.

1. Records.  A SCRATCH handle with the same graph after the same (deterministic) LM run -- node values asserted equal bit for bit, as
   tests/test_gpu_merge_gate.py does -- gets every candidate as a real pps_add_odometry factor.  On a JAC_NUMERIC handle
   pps_debug_loop_gate_records must EQUAL pps_eval_factor(fid, JAC_NUMERIC).  On the JAC_ANALYTIC handles the largest |difference| over the
   largest |J| entry of the factor is printed (`LOOP <graph>: analytic records ...`) and asserted against 4 x ANALYTIC_REL of
   tests/test_gpu_factor_gate.py: the same closed form in a sibling file built with the same flags.  The call made 2 launches, whatever n.
2. d2 and S against numpy: Sigma from the two CPU inverses of tests/test_gpu_cov.py (_reference), Jw and r from step 1,
   loop_gate_helpers.reference.  e = the largest relative error, of d2 over the candidates and of the entries of S relative to max |S|;
   d = the same distance between the two CPU references; bound e <= max(16 d, 1e-12).  Each reference S has a condition number below 1e8.
   One `LOOP <graph>: e ... d ... cond ...` line per graph (-s).
3. Decisions at 12.592: `accepted` is the reference's list; the REFERENCE alone accepts and rejects at least one candidate per graph and has
   no d2 within 1 % of the threshold.  (The offsets of loop_gate_helpers.make_candidates -- one sigma of the candidate's noise for the even
   entries, a gross one for the odd ones -- were checked with loop_gate_helpers.cpu_reference, the oracle's LM run and a dense inverse, on
   every graph of the table before any device ran: 3 to 7 of the 5 to 11 candidates accepted, the d2 closest to the threshold 11.80 on
   hard_30p_8l, 6 % away.)
4 .. 7: independence of the rest of the list, the candidate that is not positive definite, validity and side effects, log data (below).

Graphs: small_world_5_3, two poses with a prior and one odometry edge (both poses in the root front), corridor_60_14, the fixture
hard_30p_8l, corridor_60_14 with the wide walk kernel forced, corridor_60_14 on an analytic handle, band_60p_40l of
tests/linsolve_helpers.py after pps_cov_factor only, and dense_64p_200l after pps_cov_factor only.
"""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

import pop_up_slam_amd as P
from cov_factor_helpers import GRAPHS
from cov_helpers import node_layout
from helpers import load_fixture
from linsolve_helpers import CASES as LINSOLVE_CASES, loop_graph
from loop_gate_helpers import CHI2_6_095, WAVES, choose_pairs, errors, make_candidates, pose_paths, reference, tree_case
from pop_up_slam_amd import graphio, synth
from test_gpu_cov import _build, _reference
from test_gpu_factor_gate import ANALYTIC_REL

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NO_RECOVERY = "no valid covariance recovery"
_corridor = lambda: synth.corridor(60, 14, seed=7)
GROSS, LOOSE = (1.0, 0.5), (20.0, 1.0)
# name -> (spec, jacobian_mode of the handle, recovery, force the wide walk kernel, all three tree cases must be among the candidates, the gross
# offset in m / rad).  The generator's graphs carry unit sqrt information (1 m, 1 rad per factor), a relative pose there is uncertain by
# metres and 1 m is no gross error: their gross offset is 20 m / 1 rad.
CASES = {"small_world_5_3": (lambda: synth.small_world(5, 3), 0, "recover", False, True, LOOSE),
         "two_poses": (lambda: loop_graph(2, 0), 0, "recover", False, False, GROSS),
         "corridor_60_14": (_corridor, 0, "recover", False, True, LOOSE),
         "hard_30p_8l": (lambda: load_fixture("hard_30p_8l")[1], 0, "recover", False, True, LOOSE),
         "corridor_60_14_wide": (_corridor, 0, "recover", True, True, LOOSE),
         "corridor_60_14_analytic": (_corridor, 1, "recover", False, True, LOOSE),
         "band_60p_40l": (LINSOLVE_CASES["band_60p_40l"][0], 1, "factor", False, True, GROSS),
         "dense_64p_200l": (GRAPHS["dense_64p_200l"], 1, "factor", False, True, GROSS)}
SEED = 17
_DONE = {}


def _poses(rec):
    return [n for n in rec.node_ids() if rec.dims[n] == 6]


def _values(g, rec):
    return [g.get_pose(n) if rec.dims[n] == 6 else g.get_plane(n) for n in rec.node_ids()]


def _same_values(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _handle(case):
    make, mode, recovery, wide, _, _ = CASES[case]
    g, rec = _build(make(), jacobian_mode=mode)
    g.batch_optimize()
    if wide:
        g.debug_cov_path_form(1)
    g.cov_recover() if recovery == "recover" else g.cov_factor()
    return g, rec


def _candidates(g, rec, gross):
    """(pairs, meas, sqrtinf, tree cases among the pairs) from the handle's own analysis and estimate"""
    A = g.analysis_dump()
    lay = node_layout(A, [rec.dims[n] for n in rec.node_ids()])
    poses = _poses(rec)
    path = pose_paths(A, lay, poses)
    pairs, _ = choose_pairs(poses, path)
    meas, sq = make_candidates({n: g.get_pose(n) for n in poses}, pairs, SEED, gross=gross)
    return pairs, meas, sq, {tree_case(path[a], path[b]) for a, b in pairs}


def _gate(g, pairs, meas, sq, sel=None, **kw):
    sel = range(len(pairs)) if sel is None else sel
    return g.loop_gate([pairs[k][0] for k in sel], [pairs[k][1] for k in sel], meas[list(sel)], sq[list(sel)], **kw)


def _scratch_records(case, values, pairs, meas, sq):
    """(Jw, r) per candidate from pps_eval_factor on a second handle: the same graph after the same LM run, every candidate added AFTERWARDS
    as a real odometry factor (the estimate passes through the re-analysis as a plain copy)"""
    make, mode, _, _, _, _ = CASES[case]
    s, srec = _build(make(), jacobian_mode=mode)
    s.batch_optimize()
    assert _same_values(_values(s, srec), values), case
    fids = [s.add_odometry(a, b, meas[k], sq[k]) for k, (a, b) in enumerate(pairs)]
    ev = [s.eval_factor(f, mode) for f in fids]
    assert _same_values(_values(s, srec), values), case
    s.close()
    return np.array([J for J, _ in ev]), np.array([r for _, r in ev])


def _sigma(S, blk, pairs):
    return np.array([np.block([[blk(S, a, a), blk(S, a, b)], [blk(S, b, a), blk(S, b, b)]]) for a, b in pairs])


def _case(case):
    """everything the tests of one graph share, computed once: the device's answer, its records, eval_factor's, the two references"""
    if case in _DONE:
        return _DONE[case]
    g, rec = _handle(case)
    pairs, meas, sq, cases = _candidates(g, rec, CASES[case][5])
    d2, S, acc = _gate(g, pairs, meas, sq, want_S=True)
    out = {"pairs": pairs, "meas": meas, "sq": sq, "cases": cases, "dev": (d2, S, acc, g.loop_gate_last()), "records": g.loop_gate_records()}
    values = _values(g, rec)
    out["scratch"] = _scratch_records(case, values, pairs, meas, sq)
    S1, S2, blk = _reference(g, rec, CASES[case][1])
    out["ref"] = tuple(reference(*out["scratch"], _sigma(Sx, blk, pairs)) for Sx in (S1, S2))
    g.close()
    _DONE[case] = out
    return out


# ---- 1. Jw and r are pps_eval_factor's ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_records_against_eval_factor(built, case):
    c = _case(case)
    pairs, n = c["pairs"], len(c["pairs"])
    # what the list is made of: a pose in at least three candidates, a pair listed twice, a count that leaves a workgroup partly empty
    assert max(sum(p in q for q in pairs) for p in {a for a, _ in pairs}) >= 3 and len(set(pairs)) < n and n % WAVES != 0
    if CASES[case][4]:
        assert c["cases"] == {"same", "nested", "apart"}, (case, c["cases"])
    Jw, r = c["records"]
    sJ, sr = c["scratch"]
    assert Jw.shape == (n, 6, 12) and r.shape == (n, 6)
    worst = max(float(max(np.max(np.abs(Jw[k] - sJ[k])), np.max(np.abs(r[k] - sr[k]))) / np.max(np.abs(sJ[k]))) for k in range(n))
    if CASES[case][1] == 0:
        print(f"LOOP {case}: numeric records, largest difference over the candidate's largest |J| {worst:.3e}")
        assert np.array_equal(Jw, sJ) and np.array_equal(r, sr), case
    else:
        print(f"LOOP {case}: analytic records, largest difference over the candidate's largest |J| {worst:.3e}")
        assert worst <= 4 * ANALYTIC_REL, (case, worst)
    assert c["dev"][3][1] == 2                                              # the walk launch + ONE candidate launch, whatever n


# ---- 2. d2 and S against numpy, 3. decisions ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_d2_s_and_decisions_against_numpy(built, case):
    c = _case(case)
    n = len(c["pairs"])
    d2, S, acc, last = c["dev"]
    (ref, refS, cond), (ref2, ref2S, _) = c["ref"]
    assert np.all(np.isfinite(ref)) and np.all(ref > 0) and cond < 1e8, (case, cond)          # asserted on the reference alone
    want = [k for k in range(n) if ref[k] < CHI2_6_095]
    assert 0 < len(want) < n, (case, ref)
    assert np.all(np.abs(ref - CHI2_6_095) > 0.01 * CHI2_6_095), (case, ref)
    assert d2.shape == (n,) and S.shape == (n, 6, 6) and np.all(np.isfinite(d2)) and np.all(np.isfinite(S)) and last[2] == 0
    assert np.array_equal(S, np.transpose(S, (0, 2, 1)))                    # exactly symmetric
    e, d = errors(d2, S, ref, refS), errors(ref2, ref2S, ref, refS)
    bound = max(16 * d, 1e-12)
    print(f"LOOP {case}: candidates {n} e {e:.3e} d {d:.3e} bound {bound:.3e} cond {cond:.2e} d2 {ref.min():.3g} .. {ref.max():.3g} accepted {len(want)} "
          f"kernel_sec {last[0]:.3e} launches {last[1]}")
    assert e <= bound, (case, e, d)
    assert list(acc) == want, case


def test_cap_accepted_and_the_outputs_that_may_be_null(built):
    c = _case("corridor_60_14")
    pairs, meas, sq = c["pairs"], c["meas"], c["sq"]
    d2, S, acc, _ = c["dev"]
    n = len(pairs)
    g, _ = _handle("corridor_60_14")
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    ia = np.array([a for a, _ in pairs], dtype=np.int32); ib = np.array([b for _, b in pairs], dtype=np.int32)
    m = np.ascontiguousarray(meas); w = np.ascontiguousarray(sq)
    call = lambda thr, d2p, Sp, cap, accp, cntp: g.L.pps_loop_gate(g.h, n, ia.ctypes.data_as(ip), ib.ctypes.data_as(ip), m.ctypes.data_as(dp),
                                                                  w.ctypes.data_as(dp), thr, d2p, Sp, cap, accp, cntp)
    thr = float(np.sort(d2)[n - 2]) * 1.0000001                              # all but the largest pass
    want = [k for k in range(n) if d2[k] < thr]
    assert len(want) == n - 1
    few = np.full(5, -7, dtype=np.int32); cnt = C.c_int(-1)
    assert call(thr, None, None, 4, few.ctypes.data_as(ip), C.byref(cnt)) == P.PPS_OK
    assert cnt.value == len(want) and list(few[:4]) == want[:4] and few[4] == -7          # cap below the count: that many written, the full count reported
    assert call(thr, None, None, 0, None, C.byref(cnt)) == P.PPS_OK and cnt.value == len(want)                # the count alone
    only = np.full(n, -7.0)
    assert call(np.nan, only.ctypes.data_as(dp), None, 0, None, None) == P.PPS_OK and np.array_equal(only, d2)   # d2 alone; nobody reads the threshold
    onlyS = np.full((n, 6, 6), -7.0)
    assert call(CHI2_6_095, None, onlyS.ctypes.data_as(dp), 0, None, None) == P.PPS_OK and np.array_equal(onlyS, S)
    d2n, none, accn = _gate(g, pairs, meas, sq)
    assert none is None and np.array_equal(d2n, d2) and np.array_equal(accn, acc)
    g.close()


# ---- 4. an entry's answer does not depend on the rest of the list ------------------------------------------------------------------
@pytest.mark.parametrize("case", ["corridor_60_14", "band_60p_40l"])
def test_answers_are_independent_of_the_rest_of_the_list(built, case):
    c = _case(case)
    pairs, meas, sq = c["pairs"], c["meas"], c["sq"]
    d2, S, acc, _ = c["dev"]
    n = len(pairs)
    g, _ = _handle(case)
    for k in range(n):                                                       # every candidate alone
        d2k, Sk, _ = _gate(g, pairs, meas, sq, [k], want_S=True)
        assert d2k[0] == d2[k] and np.array_equal(Sk[0], S[k]), (case, k)
    for sel in (list(range(n))[::-1], list(range(n))[1::3]):                 # the list reversed, a sub-list
        d2s, Ss, accs = _gate(g, pairs, meas, sq, sel, want_S=True)
        assert np.array_equal(d2s, d2[sel]) and np.array_equal(Ss, S[sel]), (case, sel)
        assert [sel[i] for i in accs] == [k for k in sel if k in acc]
    # the pair listed twice: with the same measurement and weights, equal bits
    dup = [k for k in range(n) if pairs[k] == pairs[0]]
    assert len(dup) == 2
    m2, w2 = meas.copy(), sq.copy()
    m2[dup[1]] = m2[dup[0]]; w2[dup[1]] = w2[dup[0]]
    d2d, Sd, _ = _gate(g, pairs, m2, w2, want_S=True)
    assert d2d[dup[0]] == d2d[dup[1]] == d2[dup[0]] and np.array_equal(Sd[dup[0]], Sd[dup[1]])
    g.close()


# ---- 5. a candidate whose S is not positive definite -----------------------------------------------------------------------------------
def test_not_positive_definite_candidate(built):
    """sqrt information 1e200 on a graph with nonzero marginals: Jw Sigma Jw' overflows, the first pivot of S is not finite.  The candidate is
    NaN, not accepted and counted; every other entry keeps its bits; the call answers PPS_OK."""
    c = _case("corridor_60_14")
    pairs, meas = c["pairs"], c["meas"]
    d2, S, acc, _ = c["dev"]
    n = len(pairs); bad = 2
    sq = c["sq"].copy(); sq[bad] = synth._ut_diag([1e200] * 6)
    g, _ = _handle("corridor_60_14")
    d2b, Sb, accb = _gate(g, pairs, meas, sq, want_S=True)
    last = g.loop_gate_last()
    _, rb = g.loop_gate_records()
    assert np.all(np.isfinite(rb[bad]))                                      # (the residual itself is finite: it is S that overflows)
    assert np.isnan(d2b[bad]) and bad not in accb and last[2] == 1 and last[1] == 2
    keep = [k for k in range(n) if k != bad]
    assert np.array_equal(d2b[keep], d2[keep]) and np.array_equal(Sb[keep], S[keep]) and list(accb) == [k for k in acc if k != bad]
    d2a, _, _ = _gate(g, pairs, meas, c["sq"])                               # the next call counts none
    assert np.array_equal(d2a, d2) and g.loop_gate_last()[2] == 0
    g.close()


# ---- 6. validity and side effects ---------------------------------------------------------------------------------------------------
def test_validity_follows_the_recovery_and_solves_are_left_alone(built):
    spec = _corridor()

    def run(with_gate):
        g, rec = _build(spec)
        poses = _poses(rec)
        ia, ib = [poses[0], poses[5]], [poses[-1], poses[2]]
        meas = np.zeros((2, 6)); sq = np.array([synth._ut_diag([4.0] * 3 + [20.0] * 3)] * 2)
        if with_gate:
            need = C.c_int64(-1)
            assert g.L.pps_debug_loop_gate_records(g.h, 0, None, C.byref(need)) == P.PPS_ESTATE      # records are refused before the first call
            with pytest.raises(P.PpsError) as e:                             # no recovery yet ...
                g.loop_gate(ia, ib, meas, sq)
            assert e.value.code == P.PPS_ESTATE and NO_RECOVERY in str(e.value)
            assert len(g.loop_gate([], [], np.zeros((0, 6)), np.zeros((0, 21)))[0]) == 0              # ... but n == 0 is answered before it is looked at
            g.cov_recover()
            g.loop_gate(ia, ib, meas, sq)
        it = g.batch_optimize(); tr = g.trace(); x = (g.get_poses().copy(), g.get_planes().copy())
        if with_gate:
            st = g.stats()
            g.cov_factor()                                                   # the factor alone is enough ...
            first = g.loop_gate(ia, ib, meas, sq, want_S=True)
            g.cov_recover()                                                  # ... and so is the full recovery: the same bits
            again = g.loop_gate(ia, ib, meas, sq, want_S=True)
            assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1])
            assert g.trace() == tr and g.stats()["lm_iterations"] == st["lm_iterations"] and g.stats()["n_launches"] == st["n_launches"]
            np.testing.assert_array_equal(g.get_poses(), x[0]); np.testing.assert_array_equal(g.get_planes(), x[1])
            assert np.isfinite(g.chi2())                                     # a read keeps the recovery
            assert np.array_equal(g.loop_gate(ia, ib, meas, sq)[0], first[0])
            Jw, r = g.loop_gate_records()
            assert Jw.shape == (2, 6, 12) and r.shape == (2, 6)
            changes = [lambda: g.set_pose(poses[3], g.get_pose(poses[3])), lambda: g.add_odometry(ia[0], ib[0], meas[0], sq[0]),
                       lambda: g.set_cost_function(P.COST_HUBER, 1.0)]
            for change in changes:                                           # every call that ends a recovery ends the gate's answers
                g.cov_recover(); g.loop_gate(ia, ib, meas, sq)
                change()
                with pytest.raises(P.PpsError) as e:
                    g.loop_gate(ia, ib, meas, sq)
                assert e.value.code == P.PPS_ESTATE
            assert "cost function" in str(e.value)                           # (the last refusal names the cost function, recovery or not)
        g.close()
        return it, tr, x
    a, b = run(False), run(True)
    assert a[0] == b[0] and a[1] == b[1]                                     # the LM trace after the call is the one without it, bit for bit
    np.testing.assert_array_equal(a[2][0], b[2][0]); np.testing.assert_array_equal(a[2][1], b[2][1])


def test_refusals_with_a_valid_recovery(built):
    g, rec = _handle("small_world_5_3")
    poses = _poses(rec); planes = [n for n in rec.node_ids() if rec.dims[n] == 3]
    meas = np.zeros((1, 6)); sq = np.array([synth._ut_diag([4.0] * 3 + [20.0] * 3)])
    bad = max(rec.node_ids()) + 7
    for a, b, m, w in (([poses[0]], [bad], meas, sq), ([-1], [poses[1]], meas, sq), ([poses[0]], [planes[0]], meas, sq), ([poses[1]], [poses[1]], meas, sq),
                       ([poses[0]], [poses[1]], meas + np.nan, sq), ([poses[0]], [poses[1]], meas, sq * np.inf)):
        with pytest.raises(P.PpsError) as e:
            g.loop_gate(a, b, m, w)
        assert e.value.code == P.PPS_EINVAL
    with pytest.raises(P.PpsError) as e:
        g.loop_gate([poses[0]], [poses[1]], meas, sq, threshold=np.nan)
    assert e.value.code == P.PPS_EINVAL
    d2, _, _ = g.loop_gate([poses[0]], [poses[1]], meas, sq)                 # the refusals left the recovery and the buffers alone
    assert np.all(np.isfinite(d2))
    g.close()


# ---- 7. log data -------------------------------------------------------------------------------------------------------------------
def test_held_out_loop_closures_of_sphere2500(built):
    """The first 1 400 lines of sphere2500 with every tenth loop-closing edge (|i - j| > 1) held out; batch_optimize, cov_factor, and the held-out
    edges -- their own measurements and information -- as the candidates.  d2 against numpy (Sigma from the two CPU inverses of the dense H, Jw
    and r the gate's own records, which test 1 ties to pps_eval_factor) under the bound of test 2, equal decisions at 12.592; the share
    accepted is printed (DESIGN.md 5h quotes it), not asserted."""
    spec = graphio.load_edge3_log(os.path.join(HERE, "golden", "isam_data", "sphere2500.txt"), max_lines=1400)
    loops = [k for k in range(len(spec.f_type)) if spec.f_type[k] == synth.F_ODOMETRY and abs(int(spec.f_nodes[k][0]) - int(spec.f_nodes[k][1])) > 1]
    held = loops[::10]
    keep = np.ones(len(spec.f_type), dtype=bool); keep[held] = False
    meta = dict(spec.meta)
    if meta.get("factor_after_node") is not None:                            # (the replay order of the log: one entry per factor)
        meta["factor_after_node"] = np.asarray(meta["factor_after_node"])[keep]
    kept = dataclasses.replace(spec, f_type=spec.f_type[keep], f_nodes=spec.f_nodes[keep], f_meas=spec.f_meas[keep], f_sqrtinf=spec.f_sqrtinf[keep],
                               meta=meta)
    assert len(held) == 68 and len(loops) == 675
    g, rec = _build(kept, jacobian_mode=1)
    g.batch_optimize()
    g.cov_factor()
    pairs = [(int(spec.f_nodes[k][0]), int(spec.f_nodes[k][1])) for k in held]
    meas, sq = spec.f_meas[held, :6], spec.f_sqrtinf[held, :21]
    d2, S, acc = _gate(g, pairs, meas, sq, want_S=True)
    last = g.loop_gate_last()
    Jw, r = g.loop_gate_records()
    S1, S2, blk = _reference(g, rec, 1)
    (ref, refS, cond), (ref2, ref2S, _) = (reference(Jw, r, _sigma(Sx, blk, pairs)) for Sx in (S1, S2))
    e, d = errors(d2, S, ref, refS), errors(ref2, ref2S, ref, refS)
    print(f"LOOP sphere2500_1400: held out {len(held)} of {len(loops)} loop closures, accepted at 12.592: {len(acc)} ({len(acc) / len(held):.2f}); "
          f"e {e:.3e} d {d:.3e} bound {max(16 * d, 1e-12):.3e} cond {cond:.2e} d2 {ref.min():.3g} .. {ref.max():.3g} kernel_sec {last[0]:.3e}")
    assert cond < 1e8 and last[1] == 2 and last[2] == 0
    assert e <= max(16 * d, 1e-12), (e, d)
    assert list(acc) == [k for k in range(len(held)) if ref[k] < CHI2_6_095]
    g.close()
