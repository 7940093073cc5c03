"""CPU: pps_factor_gate before any kernel runs on a device -- the C-ABI surface without a device, what the statistic means, and the
invariants the GPU tests (tests/test_gpu_factor_gate.py) take their inputs from.

d2 = r' (I - P)^-1 r, lev = trace(P), P = J Sigma_ff J' (factor_gate_helpers.reference_gate; oracle/numpy_ref.py for the graph, its central
differences and LM, a dense inverse for Sigma)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pop_up_slam_amd as P
from factor_gate_helpers import CHI2_3_095, CHI2_6_095, PIVOT_MIN, cpu_graph_gate, leave_one_out_d2, threshold_of
from helpers import load_fixture
from oracle import numpy_ref as NR
from pop_up_slam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LM = dict(eps2=1e-9, eps_rel=1e-14)      # converged far below the default stopping rule: the statistic is defined at the solution


def test_symbols_are_declared_exported_and_bound(built):
    hdr = open(os.path.join(ROOT, "include", "pps.h")).read()
    lib = C.CDLL(P.LIB_PATH)
    for name in ("pps_factor_gate", "pps_factor_gate_last", "pps_debug_factor_gate_records"):
        assert re.search(r"\b" + name + r"\s*\(", hdr) and name in P.SYMBOLS and getattr(lib, name) is not None
    assert P.lib().pps_version() == 305                    # detected by symbol lookup, not by a version bump
    assert (CHI2_3_095, CHI2_6_095) == (7.815, 12.592)


def test_arguments_and_state_without_a_device(built):
    spec = synth.small_world(5, 3, seed=1)
    g = P.Graph(); _, fid = spec.replay(g)
    fids = [int(f) for f in fid]
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    d2 = np.full(4, -7.0); lev = np.full(4, -7.0); flagged = np.full(4, -7, dtype=np.int32); cnt = C.c_int(-7)
    ids = np.array(fids[:3], dtype=np.int32)
    args = lambda **k: [k.get("h", g.h), k.get("n", 3), k.get("ids", ids.ctypes.data_as(ip)), C.c_double(k.get("thr3", 7.815)), C.c_double(k.get("thr6", 12.592)),
                        k.get("d2", d2.ctypes.data_as(dp)), k.get("lev", lev.ctypes.data_as(dp)), k.get("cap", 4), k.get("flagged", flagged.ctypes.data_as(ip)),
                        k.get("cnt", C.byref(cnt))]
    untouched = lambda: np.all(d2 == -7.0) and np.all(lev == -7.0) and np.all(flagged == -7) and cnt.value == -7
    bad = np.array([fids[0], len(fids) + 7], dtype=np.int32); neg = np.array([-1], dtype=np.int32)
    for k in ({"h": None}, {"n": -1}, {"cap": -1}, {"d2": None, "lev": None, "flagged": None, "cnt": None}, {"cnt": None}, {"flagged": None},
              {"thr3": np.nan}, {"thr6": np.inf}, {"thr3": -np.inf}, {"n": 2, "ids": bad.ctypes.data_as(ip)}, {"n": 1, "ids": neg.ctypes.data_as(ip)}):
        assert g.L.pps_factor_gate(*args(**k)) == P.PPS_EINVAL, k
    assert untouched()
    # what is no PPS_EINVAL: NULL fids (n ignored), the count alone, one output of the three, thresholds that nobody reads -- each goes on
    # to ask for the recovery, which this handle does not have
    for k in ({"n": -5, "ids": None}, {"flagged": None, "cap": 0}, {"d2": None, "lev": None}, {"lev": None, "flagged": None, "cnt": None, "cap": 0},
              {"flagged": None, "cnt": None, "cap": 0, "thr3": np.nan, "thr6": np.nan}):
        assert g.L.pps_factor_gate(*args(**k)) == P.PPS_ESTATE, k
        assert "no valid covariance recovery" in g.L.pps_last_error(g.h).decode()
    # n == 0: PPS_OK before the recovery is looked at, outputs untouched
    assert g.L.pps_factor_gate(*args(n=0)) == P.PPS_OK and untouched()
    empty = P.Graph(); empty.add_pose([0, 0, 0, 0, 0, 0, 1])                        # no live factor, all asked for: nothing to do
    e2, el, ef = empty.factor_gate()
    assert len(e2) == 0 and len(el) == 0 and len(ef) == 0
    empty.close()
    # a cost function: refused after the argument checks, without a device, naming the cost function; PPS_COST_NONE lifts the refusal
    g.set_cost_function(P.COST_HUBER, 1.0)
    assert g.L.pps_factor_gate(*args(n=-1)) == P.PPS_EINVAL                         # (the argument checks come first)
    assert g.L.pps_factor_gate(*args()) == P.PPS_ESTATE and "cost function" in g.L.pps_last_error(g.h).decode() and untouched()
    with pytest.raises(P.PpsError) as e:
        g.factor_gate()
    assert e.value.code == P.PPS_ESTATE and "pps_set_cost_function" in str(e.value)
    g.set_cost_function(P.COST_NONE)
    with pytest.raises(P.PpsError) as e:
        g.factor_gate()
    assert e.value.code in (P.PPS_ESTATE, P.PPS_EHIP) and "cost function" not in str(e.value)      # for want of a recovery (or a device)
    # the _last call and the records before any successful call
    sec = C.c_double(-1.0); n = C.c_int(-1); unt = C.c_int(-1)
    assert g.L.pps_factor_gate_last(g.h, C.byref(sec), C.byref(n), C.byref(unt)) == P.PPS_OK and (sec.value, n.value, unt.value) == (0.0, 0, 0)
    assert g.L.pps_factor_gate_last(g.h, None, None, None) == P.PPS_OK and g.L.pps_factor_gate_last(None, None, None, None) == P.PPS_EINVAL
    need = C.c_int64(-1)
    assert g.L.pps_debug_factor_gate_records(g.h, 0, None, C.byref(need)) == P.PPS_ESTATE
    assert g.L.pps_debug_factor_gate_records(g.h, 0, None, None) == P.PPS_EINVAL
    # a removed factor is an unknown one; the handle stays usable
    g.remove_factor(fids[-1])
    with pytest.raises(P.PpsError) as e:
        g.factor_gate([fids[0], fids[-1]])
    assert e.value.code == P.PPS_EINVAL
    assert g.num_factors() == len(fids) - 1
    p = g.add_pose([0, 0, 0, 0, 0, 0, 1]); g.add_pose_prior(p, np.zeros(6), synth._ut_diag([1.0] * 6))
    assert g.num_factors() == len(fids)
    g.close()


def test_d2_is_the_distance_at_the_solution_without_the_factor():
    """small_20p_6l converged with eps2 = 1e-9, eps_rel = 1e-14.  For every 15th testable factor (indices 1, 16, ..., 106): the formula's d2
    against a REAL leave-one-out solve -- the factor removed, LM run again from the estimate with the same stopping rule, the removed factor's
    r and J taken at the new estimate, d2 = r' (I + J Sigma_- J')^-1 r with Sigma_- the dense inverse of the reduced graph's J'J.
    Measured: the largest relative difference over the eight factors is 1.7e-2 (factor 61; the smallest 8.7e-5, factor 106) -- what is left
    is the nonlinearity between the two estimates.  Asserted with a factor 2."""
    _, spec = load_fixture("small_20p_6l")
    G = NR.Graph(spec)
    G.levenberg_marquardt(**LM)
    d2, lev, emin, _ = cpu_graph_gate(G)
    testable = [k for k in range(len(d2)) if emin[k] >= PIVOT_MIN]
    sample = testable[::15]
    assert sample == [1, 16, 31, 46, 61, 76, 91, 106]
    worst = 0.0
    for k in sample:
        loo = leave_one_out_d2(NR, spec, G, k, **LM)
        worst = max(worst, abs(loo - d2[k]) / loo)
        print(f"FGATE leave-one-out small_20p_6l factor {k}: formula {d2[k]:.6e} re-solved {loo:.6e}")
    print(f"FGATE leave-one-out small_20p_6l: largest relative difference {worst:.3e}")
    assert worst <= 2 * 1.7e-2, worst


def test_invariants_of_the_physically_weighted_corridor():
    """corridor(60, 14, seed=7, physical_weights=True) at its converged estimate: the leverages sum to the state dimension (the trace of the
    hat matrix; measured 402 + 1e-13), the pose prior (factor 0, the gauge) is the one untestable factor (smallest eigenvalue of I - P
    -1.5e-14), every other factor has its smallest eigenvalue above 1e-3 (measured: 1.3e-2), and the 0.95 thresholds flag 17 of the 360
    testable factors.  With ONE corrupted observation (robust_helpers.corrupt_one_observation(spec, 7, 0.2, 0.3)) that factor, index 10, has
    d2 = 598 and is the arg-max of d2 / threshold."""
    from robust_helpers import corrupt_one_observation
    spec = synth.corridor(60, 14, seed=7, physical_weights=True)
    G = NR.Graph(spec)
    G.levenberg_marquardt(**LM)
    d2, lev, emin, Jr = cpu_graph_gate(G)
    assert G.n() == 402 and abs(float(lev.sum()) - G.n()) <= 1e-9
    assert spec.f_type[0] == NR.F_POSE_PRIOR and [k for k in range(len(d2)) if emin[k] < PIVOT_MIN] == [0]
    assert np.all(emin[1:] > 1e-3), float(emin[1:].min())
    assert np.all(lev > 0) and np.all(lev[1:] < np.array([len(r) for _, r in Jr])[1:])
    thr = np.array([threshold_of(len(r)) for _, r in Jr])
    flagged = int(np.sum(d2[1:] > thr[1:]))
    print(f"FGATE corridor_60_physical (CPU): chi2 {G.chi2(G.x):.1f} flagged {flagged} of {len(d2) - 1} smallest eigenvalue {emin[1:].min():.3e}")
    assert flagged == 17 and len(d2) - 1 == 360
    bad, k = corrupt_one_observation(spec, 7, 0.2, 0.3)
    B = NR.Graph(bad)
    B.levenberg_marquardt(**LM)
    b2, _, bmin, _ = cpu_graph_gate(B)
    ratio = np.where(bmin >= PIVOT_MIN, b2 / thr, -1.0)
    print(f"FGATE corridor_60_physical corrupted (CPU): factor {k} d2 {b2[k]:.1f}")
    assert k == 10 and int(np.argmax(ratio)) == k and 500 < b2[k] < 700
