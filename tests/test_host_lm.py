"""The Levenberg-Marquardt rule of the three host loops lives in one header (csrc/pps_lm.h: loop condition, accept / reject / stop,
lambda schedule, trace, trial counters, the not-PD report).  tests/cpp/lm_host.cpp drives it without a device: the seven recorded
trajectories of tests/golden (chi2_initial and, per trial, lambda / chi2 / accepted of the reference's loop) are replayed from their
chi2 values alone, and the controller must reproduce every lambda and verdict and stop where the reference stopped."""
import ctypes as C
import glob
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
# pps_default_props (include/pps.h): epsilon2, epsilon_abs, epsilon_rel, max_iterations, lm_lambda0, lm_lambda_factor
DEFAULTS = dict(epsilon2=1e-3, epsilon_abs=1e-4, epsilon_rel=1e-6, max_iterations=500, lm_lambda0=1e-6, lm_lambda_factor=10.0)
REJECTED, ACCEPTED, CONVERGED = 0, 1, 2
PPS_OK, PPS_ENOTPD = 0, 2
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "*p_*l.json")))


@pytest.fixture(scope="module")
def replay():
    src = os.path.join(ROOT, "tests", "cpp", "lm_host.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "liblm_host.so")
    deps = [src, os.path.join(ROOT, "pop_up_slam_amd", "csrc", "pps_lm.h"), os.path.join(ROOT, "include", "pps.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-ffp-contract=off",
                               "-I" + os.path.join(ROOT, "pop_up_slam_amd", "csrc"), src, "-o", out])
    lib = C.CDLL(out)
    lib.lm_host_replay.restype = C.c_int
    lib.lm_host_replay.argtypes = [_dp, C.c_double, C.c_int, _dp, _dp, _dp, _dp, _dp, _ip, _ip, _dp]

    def run(chi2_initial, chi2, dn2=None, notpd=None, **props):
        p = dict(DEFAULTS, **props)
        n = len(chi2)
        props6 = np.array([p[k] for k in DEFAULTS], dtype=np.float64)
        chi2 = np.ascontiguousarray(chi2, dtype=np.float64)
        dn2 = np.full(n, 1.0) if dn2 is None else np.ascontiguousarray(dn2, dtype=np.float64)      # |delta| = 1 > epsilon2
        notpd = np.zeros(n) if notpd is None else np.ascontiguousarray(notpd, dtype=np.float64)
        lam, c2, acc, ver, summ = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(9)
        k = lib.lm_host_replay(props6.ctypes.data_as(_dp), chi2_initial, n, chi2.ctypes.data_as(_dp), dn2.ctypes.data_as(_dp),
                               notpd.ctypes.data_as(_dp), lam.ctypes.data_as(_dp), c2.ctypes.data_as(_dp), acc.ctypes.data_as(_ip),
                               ver.ctypes.data_as(_ip), summ.ctypes.data_as(_dp))
        assert k >= 0
        keys = ("rc", "iterations", "lm_iterations", "chi2_final", "lambda_final", "last_delta_norm", "lm_trials_notpd",
                "lm_trials_accepted", "lm_trials_rejected")
        return dict(n=k, lam=lam[:k], chi2=c2[:k], acc=acc[:k], verdict=ver[:k], **dict(zip(keys, summ)))
    return run


def test_the_fixtures_are_the_seven_recorded_trajectories():
    traces = {os.path.basename(f): json.load(open(f))["lm_trace"] for f in FIXTURES}
    assert len(traces) == 7 and sum(len(t) for t in traces.values()) == 94
    assert len(traces["hard_40p_6l.json"]) == 76 and sum(1 for t in traces["hard_40p_6l.json"] if not t[2]) == 40


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(f)[:-5] for f in FIXTURES])
def test_recorded_trajectory_follows_from_its_chi2_values(replay, path):
    fx = json.load(open(path))
    tr = fx["lm_trace"]
    r = replay(fx["chi2_initial"], [c for _, c, _ in tr])
    assert r["n"] == len(tr)                                       # no early stop, every recorded trial was judged
    ends_on_relative_test = os.path.basename(path) in ("hard_30p_8l.json", "hard_40p_6l.json")
    for k, (lam, chi2, accepted) in enumerate(tr):
        assert abs(r["lam"][k] - lam) <= 1e-12 * abs(lam), (k, r["lam"][k], lam)
        assert r["chi2"][k] == chi2 and bool(r["acc"][k]) == bool(accepted), k
        want = REJECTED if not accepted else (CONVERGED if ends_on_relative_test and k == len(tr) - 1 else ACCEPTED)
        assert r["verdict"][k] == want, (k, r["verdict"][k], want)
    assert r["rc"] == PPS_OK and r["iterations"] == r["lm_iterations"] == len(tr) == fx["lm_iterations"]
    assert r["chi2_final"] == fx["chi2_final"]                     # the chi2 the rule ends on: the last accepted trial's
    assert r["lm_trials_accepted"] == sum(1 for t in tr if t[2]) and r["lm_trials_rejected"] == sum(1 for t in tr if not t[2])
    assert r["lm_trials_notpd"] == 0 and r["last_delta_norm"] == 1.0


def test_max_iterations_cuts_the_loop(replay):
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "hard_40p_6l.json")))
    chi2 = [c for _, c, _ in fx["lm_trace"]]
    r = replay(fx["chi2_initial"], chi2, max_iterations=10)
    assert r["n"] == 10 and r["iterations"] == 10 and list(r["verdict"]) == [1 if a else 0 for _, _, a in fx["lm_trace"][:10]]
    assert replay(fx["chi2_initial"], chi2, max_iterations=0)["n"] == len(chi2)          # <= 0: no limit


def test_step_norm_and_absolute_chi2_end_the_loop(replay):
    # |delta| <= epsilon2 of the pending step: the loop ends before that trial is judged, lambda is the one it was solved with
    r = replay(10.0, [5.0, 4.0, 3.0], dn2=[1.0, 1.0, 1e-8])
    assert r["n"] == 2 and r["chi2_final"] == 4.0 and r["lambda_final"] == pytest.approx(1e-8, rel=1e-12) and r["last_delta_norm"] == 1e-4
    r = replay(10.0, [5.0, 5e-5, 1e-5])                                                 # chi2 <= epsilon_abs
    assert r["n"] == 2 and r["chi2_final"] == 5e-5
    assert replay(5e-5, [1e-5])["n"] == 0                                               # ... before the first trial


def test_only_a_last_trial_that_was_not_pd_is_reported(replay):
    # a not-PD factorisation leaves garbage: its chi2 is worse, LM rejects the step and raises lambda
    r = replay(10.0, [50.0, 5.0, 4.0], notpd=[1.0, 0.0, 0.0])
    assert r["n"] == 3 and list(r["verdict"]) == [REJECTED, ACCEPTED, ACCEPTED]
    assert r["rc"] == PPS_OK and r["lm_trials_notpd"] == 1
    assert r["lam"][1] == pytest.approx(1e-5, rel=1e-12)
    r = replay(10.0, [5.0, 50.0], notpd=[0.0, 1.0], max_iterations=2)                   # the trial the loop ended on
    assert r["n"] == 2 and list(r["verdict"]) == [ACCEPTED, REJECTED]
    assert r["rc"] == PPS_ENOTPD and r["lm_trials_notpd"] == 1
    # the pending step of a loop that ends on max_iterations is the last trial too (solved, never judged)
    r = replay(10.0, [5.0, 4.0], notpd=[0.0, 1.0], max_iterations=1)
    assert r["n"] == 1 and r["rc"] == PPS_ENOTPD
