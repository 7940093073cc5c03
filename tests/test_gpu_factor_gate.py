"""GPU: pps_factor_gate -- d2 = r' (I - P)^-1 r and lev = trace(P), P = J Sigma_ff J', of every factor of the graph, and the factors whose
d2 exceeds the chi-square threshold of their dimension.

1. Records.  On a JAC_NUMERIC handle J and r of every entry EQUAL pps_eval_factor(fid, JAC_NUMERIC) bit for bit (taken after the gate call:
   the estimate is asserted unchanged), the Factor2 edges of the mixed graph included (pps_eval_factor evaluates those in a kernel built
   with contraction; csrc/pps_fgate.hip carries that contraction for their residual).  On the JAC_ANALYTIC handles they are compared with pps_eval_factor(fid, JAC_ANALYTIC), whose kernel is
   built with contraction while the gate's is not: the largest |difference| over the largest |J| entry of the factor on the device is
   printed (`FGATE <graph>: analytic records ...`) and asserted against 4 x ANALYTIC_REL -- measured on an MI355X: 8.9e-16 on
   corridor_60_14_analytic, 1.4e-15 on dense_48p_150l_10x5 (a value above 1e-12 would be a defect, not a tolerance).
2. d2 and leverage against numpy: Sigma from the two CPU inverses of tests/test_gpu_cov.py (_reference), J and r from pps_eval_factor,
   factor_gate_helpers.reference_gate.  e = the largest relative error over all testable entries (d2 and leverage), d = the same distance
   between the two CPU references; bound e <= max(16 d, 1e-12), the rule of tests/test_gpu_cov.py and the other gates.  One
   `FGATE <graph>: e ... d ...` line per graph (-s).  The NaN entries are exactly the reference's factors whose I - P has an eigenvalue
   below 1e-7; on the band graphs that is the pose prior alone.
3. The leverages sum to dim_nodes within 1e-8: a missing, doubled or transposed block moves the sum by at least the smallest single
   leverage (order 1e-2 on these graphs); rounding measured on the CPU is 6e-13 (tests/test_host_factor_gate.py).
4 .. 7: calibration and an outlier end to end, lists, validity and non-interference, pps_factor_gate_last.

Graphs: small_world(5, 3), corridor(60, 14), the fixture hard_30p_8l, the physically weighted corridor, the corridor on an analytic handle,
the corridor through the dense-front pass (pps_debug_cov_select_form(1) + pps_cov_select), the mixed Factor2 graph of
tests/test_gpu_factor2.py, and dense_48p_150l_10x5 after pps_cov_select (on the CPU, oracle/numpy_ref.py, no factor of that graph has the
smallest eigenvalue of its I - P between 1e-10 and 1e-4: the pose prior has 1.3e-15, the next factor 2.0e-2).
"""
import ctypes as C

import numpy as np
import pytest

import pop_up_slam_amd as P
from cov_factor_helpers import GRAPHS
from factor_gate_helpers import CHI2_3_095, CHI2_6_095, PIVOT_MIN, reference_gate, threshold_of
from helpers import load_fixture
from pop_up_slam_amd import synth
from robust_helpers import corrupt_one_observation
from test_gpu_cov import Recorder, _build, _reference
from test_gpu_factor2 import _mixed_graph, _replay

pytestmark = pytest.mark.gpu

DENSE = "dense_48p_150l_10x5"
# the largest |J_gate - J_eval_factor| / max |J| of a factor on an analytic handle, as measured on an MI355X (test 1): 8.9e-16 on
# corridor_60_14_analytic, 1.4e-15 on dense_48p_150l_10x5; 4 x the larger is asserted
ANALYTIC_REL = 1.43e-15
_corridor = lambda: synth.corridor(60, 14, seed=7)
_physical = lambda: synth.corridor(60, 14, seed=7, physical_weights=True)


def _mixed():
    class Ops:
        def replay(self, g):
            _replay(_mixed_graph(), g)
    return Ops()


# name -> (spec, jacobian_mode of the handle, recovery, band graph)
CASES = {"small_world_5_3": (lambda: synth.small_world(5, 3), 0, "recover", True),
         "corridor_60_14": (_corridor, 0, "recover", True),
         "hard_30p_8l": (lambda: load_fixture("hard_30p_8l")[1], 0, "recover", True),
         "corridor_60_physical": (_physical, 0, "recover", True),
         "corridor_60_14_analytic": (_corridor, 1, "recover", True),
         "corridor_60_14_select_form": (_corridor, 0, "select_form", True),
         "factor2_mixed": (_mixed, 0, "recover", False),
         DENSE: (GRAPHS[DENSE], 1, "select", False)}
_DONE = {}


def _values(g, rec):
    return [g.get_pose(n) if rec.dims[n] == 6 else g.get_plane(n) for n in rec.node_ids()]


def _same_values(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _recover(g, recovery):
    if recovery == "select_form":
        g.debug_cov_select_form(1)
    g.cov_recover() if recovery == "recover" else g.cov_select()


def _handle(case):
    make, mode, recovery, _ = CASES[case]
    g, rec = _build(make(), jacobian_mode=mode)
    g.batch_optimize()
    _recover(g, recovery)
    return g, rec


def _unpack(slot, m, c):
    return slot[:m * c].reshape(m, c).copy(), slot[m * c:m * c + m].copy()


def _columns(rec, fid, starts):
    a, b = rec.factors[fid]
    cols = list(range(starts[a], starts[a] + rec.dims[a]))
    return cols + (list(range(starts[b], starts[b] + rec.dims[b])) if b >= 0 else [])


def _case(case):
    """everything the tests of one graph share, computed once: the device's answers, its records, eval_factor's, the two references"""
    if case in _DONE:
        return _DONE[case]
    mode = CASES[case][1]
    g, rec = _handle(case)
    fids = sorted(rec.factors)
    d2, lev, flagged = g.factor_gate()
    last = g.factor_gate_last()
    slots = g.factor_gate_records()
    dim_nodes = g.stats()["dim_nodes"]
    values = _values(g, rec)
    ev = [g.eval_factor(f, mode) for f in fids]                               # (after the gate call; the estimate must not have moved)
    assert _same_values(_values(g, rec), values), case
    records = [_unpack(slots[i], *ev[i][0].shape) for i in range(len(fids))]
    S1, S2, _ = _reference(g, rec, mode)
    ids = rec.node_ids()
    st = np.concatenate([[0], np.cumsum([rec.dims[n] for n in ids])]).astype(int)
    starts = {n: int(st[k]) for k, n in enumerate(ids)}
    cols = [_columns(rec, f, starts) for f in fids]
    Js, rs = [J for J, _ in ev], [r for _, r in ev]
    out = {"fids": fids, "d2": d2, "lev": lev, "flagged": flagged, "last": last, "records": records, "ev": ev, "dim_nodes": dim_nodes,
           "ref": (reference_gate(Js, rs, S1, cols), reference_gate(Js, rs, S2, cols)), "m": np.array([len(r) for r in rs])}
    g.close()
    _DONE[case] = out
    return out


# ---- 1. the records are pps_eval_factor's ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_records_against_eval_factor(built, case):
    c = _case(case)
    mode = CASES[case][1]
    assert len(c["records"]) == len(c["fids"]) == len(c["d2"])
    worst = 0.0
    for (J, r), (Je, re_) in zip(c["records"], c["ev"]):
        worst = max(worst, float(max(np.max(np.abs(J - Je)), np.max(np.abs(r - re_))) / np.max(np.abs(Je))))
    if mode == 0:
        print(f"FGATE {case}: numeric records, largest difference over the factor's largest |J| {worst:.3e}")
        for k, ((J, r), (Je, re_)) in enumerate(zip(c["records"], c["ev"])):
            assert np.array_equal(J, Je) and np.array_equal(r, re_), (case, c["fids"][k])
    else:
        print(f"FGATE {case}: analytic records, largest difference over the factor's largest |J| {worst:.3e}")
        assert worst <= 4 * ANALYTIC_REL, (case, worst)


# ---- 2. d2 and leverage against numpy --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_d2_and_leverage_against_numpy(built, case):
    c = _case(case)
    (r2, rlev, emin), (s2, slev, _) = c["ref"]
    d2, lev = c["d2"], c["lev"]
    untestable = emin < PIVOT_MIN
    if case == DENSE:                                                        # (on the reference alone: no factor of this graph sits near the threshold)
        assert not np.any((emin > 1e-10) & (emin < 1e-4)), emin[(emin > 1e-10) & (emin < 1e-4)]
    assert np.array_equal(np.isnan(d2), untestable), (case, np.flatnonzero(np.isnan(d2)), np.flatnonzero(untestable))
    if CASES[case][3]:
        assert list(np.flatnonzero(untestable)) == [0] and c["last"][2] == 1                            # the pose prior alone
    ok = ~untestable
    assert np.all(np.isfinite(lev)) and np.all(r2[ok] > 0) and np.all(d2[ok] >= 0)
    e = max(float(np.max(np.abs(d2 - r2)[ok] / r2[ok])), float(np.max(np.abs(lev - rlev) / rlev)))
    d = max(float(np.max(np.abs(s2 - r2)[ok] / r2[ok])), float(np.max(np.abs(slev - rlev) / rlev)))
    bound = max(16 * d, 1e-12)
    print(f"FGATE {case}: factors {len(d2)} untestable {int(untestable.sum())} e {e:.3e} d {d:.3e} bound {bound:.3e} d2 {r2[ok].min():.3g} .. {r2[ok].max():.3g} "
          f"smallest eigenvalue of a testable I - P {emin[ok].min():.3e} kernel_sec {c['last'][0]:.3e} launches {c['last'][1]}")
    assert e <= bound, (case, e, d)


# ---- 3. the trace of the hat matrix -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_leverages_sum_to_the_state_dimension(built, case):
    c = _case(case)
    total = float(np.sum(c["lev"]))
    print(f"FGATE {case}: sum of leverages - dim_nodes {total - c['dim_nodes']:.3e} (dim_nodes {c['dim_nodes']}, smallest leverage {c['lev'].min():.3e})")
    assert abs(total - c["dim_nodes"]) <= 1e-8, (case, total, c["dim_nodes"])


# ---- 4. calibration and an outlier, end to end ------------------------------------------------------------------------------------
def _share(d2, flagged):
    return len(flagged) / float(np.sum(np.isfinite(d2)))


def test_calibration_and_an_outlier_end_to_end(built):
    """the physically weighted corridor: about 5 % of the correct factors exceed the 0.95 thresholds (CPU reference: 17 of 360, 4.7 %); one
    corrupted observation is flagged, is the arg-max of d2 / threshold and has d2 > 100 (CPU reference: 598); with it removed the flagged
    share is back in the band"""
    spec = _physical()
    g, rec = _build(spec)
    fids = sorted(rec.factors)
    g.batch_optimize(); g.cov_recover()
    d2, lev, flagged = g.factor_gate()
    thr = np.array([threshold_of(m) for m in _case("corridor_60_physical")["m"]])
    assert list(flagged) == [i for i in range(len(d2)) if np.isfinite(d2[i]) and d2[i] > thr[i]]
    print(f"FGATE calibration: clean {len(flagged)} of {int(np.sum(np.isfinite(d2)))} flagged")
    assert 0.01 <= _share(d2, flagged) <= 0.10
    bad, k = corrupt_one_observation(spec, 7, 0.2, 0.3)
    g.set_measurement(fids[k], bad.f_meas[k, :4])
    g.batch_optimize(); g.cov_recover()
    b2, _, bflag = g.factor_gate()
    ratio = np.where(np.isfinite(b2), b2 / thr, -1.0)
    print(f"FGATE calibration: corrupted factor {fids[k]} d2 {b2[k]:.1f}, {len(bflag)} flagged")
    assert k in list(bflag) and int(np.argmax(ratio)) == k and b2[k] > 100
    rec.remove_factor(fids[k])
    g.batch_optimize(); g.cov_recover()
    a2, _, aflag = g.factor_gate()
    print(f"FGATE calibration: after the removal {len(aflag)} of {int(np.sum(np.isfinite(a2)))} flagged")
    assert len(a2) == len(d2) - 1 and 0.01 <= _share(a2, aflag) <= 0.10
    g.close()


# ---- 5. lists ---------------------------------------------------------------------------------------------------------------------
def test_lists(built):
    c = _case("corridor_60_14")
    fids, d2, lev, m = c["fids"], c["d2"], c["lev"], c["m"]
    g, rec = _handle("corridor_60_14")
    assert sorted(rec.factors) == fids
    pos = list(range(0, len(fids), 7))[::-1]                                 # a reversed subset (it ends at the pose prior, entry 0) ...
    pos.insert(3, pos[1])                                                    # ... with one factor repeated
    assert 0 in pos and len(pos) > 30
    sub = [fids[p] for p in pos]
    thr = float(np.median(d2[np.isfinite(d2)]))                              # about half of the entries exceed it
    s2, slev, sflag = g.factor_gate(sub, thr3=thr, thr6=thr)
    assert np.array_equal(s2, d2[pos], equal_nan=True) and np.array_equal(slev, lev[pos])         # entry by entry the bits of the all-factors call
    want = [i for i in range(len(sub)) if np.isfinite(s2[i]) and s2[i] > thr]
    assert list(sflag) == want and 8 < len(want) < len(sub) - 8                                  # indices INTO the list given
    assert g.factor_gate_last()[2] == 1 and np.isnan(s2[pos.index(0)])
    # the thresholds go by the factor's rows
    _, _, only6 = g.factor_gate(sub, thr3=1e300, thr6=thr)
    assert list(only6) == [i for i in want if m[pos[i]] == 6] and len(only6) > 0
    # cap_flagged below the count truncates the list, not the count; the count alone; d2 alone
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    ids = np.array(sub, dtype=np.int32); few = np.full(5, -7, dtype=np.int32); cnt = C.c_int(-1); only = np.full(len(sub), -7.0)
    assert g.L.pps_factor_gate(g.h, len(sub), ids.ctypes.data_as(ip), thr, thr, None, None, 3, few.ctypes.data_as(ip), C.byref(cnt)) == P.PPS_OK
    assert cnt.value == len(want) and list(few[:3]) == want[:3] and list(few[3:]) == [-7, -7]
    assert g.L.pps_factor_gate(g.h, len(sub), ids.ctypes.data_as(ip), thr, thr, None, None, 0, None, C.byref(cnt)) == P.PPS_OK and cnt.value == len(want)
    assert g.L.pps_factor_gate(g.h, len(sub), ids.ctypes.data_as(ip), np.nan, np.nan, only.ctypes.data_as(dp), None, 0, None, None) == P.PPS_OK
    assert np.array_equal(only, s2, equal_nan=True)
    one2, onel, _ = g.factor_gate([fids[17]])
    assert one2[0] == d2[17] and onel[0] == lev[17]
    assert np.array_equal(g.factor_gate()[0], d2, equal_nan=True)
    g.close()


# ---- 6. validity and non-interference ---------------------------------------------------------------------------------------------
def test_validity_follows_the_selected_inverse_and_solves_are_left_alone(built):
    spec = _corridor()

    def run(with_gate):
        g, rec = _build(spec)
        fids = sorted(rec.factors)
        if with_gate:
            with pytest.raises(P.PpsError) as e:                             # no recovery yet ...
                g.factor_gate()
            assert e.value.code == P.PPS_ESTATE and "no valid covariance recovery" in str(e.value)
            assert len(g.factor_gate([])[0]) == 0                            # ... but an empty list is answered before it is looked at
            g.cov_recover()
            g.factor_gate()
        it = g.batch_optimize(); tr = g.trace(); x = (g.get_poses().copy(), g.get_planes().copy())
        if with_gate:
            st = g.stats()
            g.cov_factor()                                                   # the factor alone is not the selected inverse
            with pytest.raises(P.PpsError) as e:
                g.factor_gate()
            assert e.value.code == P.PPS_ESTATE and "pps_cov_factor" in str(e.value) and "pps_cov_recover" in str(e.value)
            g.cov_recover()
            first = g.factor_gate()
            marg = g.cov_marginals()                                         # the recovery is still there after a gate call
            assert len(marg) == len(rec.node_ids()) and all(np.all(np.isfinite(M)) for M in marg)
            g.cov_select()                                                   # either recovery call provides the selected inverse
            again = g.factor_gate()
            assert np.array_equal(again[0], first[0], equal_nan=True) and np.array_equal(again[1], first[1])
            assert g.trace() == tr and g.stats()["lm_iterations"] == st["lm_iterations"] and g.stats()["n_launches"] == st["n_launches"]
            np.testing.assert_array_equal(g.get_poses(), x[0]); np.testing.assert_array_equal(g.get_planes(), x[1])
            planes = [n for n in rec.node_ids() if rec.dims[n] == 3]
            obs = next(f for f, (a, b) in rec.factors.items() if b >= 0 and rec.dims[b] == 3)

            def add():
                p = g.add_pose(g.get_pose(rec.node_ids()[0])); g.add_pose_prior(p, np.zeros(6), synth._ut_diag([1.0] * 6))
            changes = [add, lambda: g.set_plane(planes[0], g.get_plane(planes[0])), lambda: g.set_measurement(obs, g.get_measurement(obs)),
                       g.update, g.batch_optimize]
            for change in changes:                                           # every kind of change that ends a recovery ends the gate's answers
                g.cov_recover(); g.factor_gate(fids[:5])
                change()
                with pytest.raises(P.PpsError) as e:
                    g.factor_gate(fids[:5])
                assert e.value.code == P.PPS_ESTATE and "no valid covariance recovery" in str(e.value)
        g.close()
        return it, tr, x
    a, b = run(False), run(True)
    assert a[0] == b[0] and a[1] == b[1]                                     # the LM trace after the call is the one without it, bit for bit
    np.testing.assert_array_equal(a[2][0], b[2][0]); np.testing.assert_array_equal(a[2][1], b[2][1])


# ---- 7. pps_factor_gate_last -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_factor_gate_last(built, case):
    c = _case(case)
    sec, launches, untestable = c["last"]
    assert launches == 1 and sec > 0 and untestable == int(np.sum(np.isnan(c["d2"])))
    assert len(c["flagged"]) == int(np.sum(np.nan_to_num(c["d2"], nan=0.0) > np.where(c["m"] == 3, CHI2_3_095, CHI2_6_095)))
