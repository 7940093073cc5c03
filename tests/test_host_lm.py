"""The Levenberg-Marquardt rule of the three host loops lives in one header (csrc/pps_lm.h: loop condition, accept / reject / stop,
lambda schedule, trace, trial counters, the not-PD report).  tests/cpp/lm_host.cpp drives it without a device: the seven recorded
trajectories of tests/golden (chi2_initial and, per trial, lambda / chi2 / accepted of the reference's loop) are replayed from their
chi2 values alone, and the controller must reproduce every lambda and verdict and stop where the reference stopped.

The same header holds the scheme that lm_solve_dual and the batched rounds share (LmDualWalk): launch sets of one or two trials, the walk over
their records, the rotation of the three state copies.  A second replay entry drives it over the same sequences; it must give what the
one-step replay gives, ask for exactly the launch sets, second records and relinearisations that the accept / reject sequence implies,
and keep the three copies apart."""
import ctypes as C
import glob
import itertools
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
    lib.lm_host_replay_walk.restype = C.c_int
    lib.lm_host_replay_walk.argtypes = [_dp, C.c_double, C.c_int, _dp, _dp, _dp, C.c_int, _dp, _dp, _ip, _ip, _dp, _ip]
    lib.lm_host_rotation.restype = C.c_int
    lib.lm_host_rotation.argtypes = [C.c_int, _ip, C.c_int, _ip]

    def run(chi2_initial, chi2, dn2=None, notpd=None, walk=None, **props):
        p = dict(DEFAULTS, **props)
        n = len(chi2)
        props6 = np.array([p[k] for k in DEFAULTS], dtype=np.float64)
        chi2 = np.ascontiguousarray(chi2, dtype=np.float64)
        dn2 = np.full(n, 1.0) if dn2 is None else np.ascontiguousarray(dn2, dtype=np.float64)      # |delta| = 1 > epsilon2
        notpd = np.zeros(n) if notpd is None else np.ascontiguousarray(notpd, dtype=np.float64)
        lam, c2, acc, ver, summ = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(9)
        counts = np.zeros(6, dtype=np.int32)
        ins = (props6.ctypes.data_as(_dp), chi2_initial, n, chi2.ctypes.data_as(_dp), dn2.ctypes.data_as(_dp), notpd.ctypes.data_as(_dp))
        outs = (lam.ctypes.data_as(_dp), c2.ctypes.data_as(_dp), acc.ctypes.data_as(_ip), ver.ctypes.data_as(_ip), summ.ctypes.data_as(_dp))
        if walk is None:
            k = lib.lm_host_replay(*ins, *outs)
        else:                                                       # ... through LmDualWalk, WALK_ONE / WALK_TWO / WALK_ADAPTIVE trials per launch set
            k = lib.lm_host_replay_walk(*ins, walk, *outs, counts.ctypes.data_as(_ip))
        assert k >= 0
        keys = ("rc", "iterations", "lm_iterations", "chi2_final", "lambda_final", "last_delta_norm", "lm_trials_notpd",
                "lm_trials_accepted", "lm_trials_rejected")
        ckeys = ("sets", "second", "relaunch", "relin", "single", "final_copy")
        return dict(n=k, lam=lam[:k], chi2=c2[:k], acc=acc[:k], verdict=ver[:k], **dict(zip(keys, summ)), **dict(zip(ckeys, (int(c) for c in counts))))
    run.lib = lib
    return run


WALK_ONE, WALK_TWO, WALK_ADAPTIVE = 0, 1, 2
# the three edge-case tests below run through the one-step replay and through the walk in each of its modes
REPLAYS = pytest.mark.parametrize("walk", [None, WALK_ONE, WALK_TWO, WALK_ADAPTIVE], ids=["one_step", "walk_one", "walk_two", "walk_adaptive"])


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


@REPLAYS
def test_max_iterations_cuts_the_loop(replay, walk):
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "hard_40p_6l.json")))
    chi2 = [c for _, c, _ in fx["lm_trace"]]
    r = replay(fx["chi2_initial"], chi2, max_iterations=10, walk=walk)
    assert r["n"] == 10 and r["iterations"] == 10 and list(r["verdict"]) == [1 if a else 0 for _, _, a in fx["lm_trace"][:10]]
    assert replay(fx["chi2_initial"], chi2, max_iterations=0, walk=walk)["n"] == len(chi2)          # <= 0: no limit


@REPLAYS
def test_step_norm_and_absolute_chi2_end_the_loop(replay, walk):
    # |delta| <= epsilon2 of the pending step: the loop ends before that trial is judged, lambda is the one it was solved with
    r = replay(10.0, [5.0, 4.0, 3.0], dn2=[1.0, 1.0, 1e-8], walk=walk)
    assert r["n"] == 2 and r["chi2_final"] == 4.0 and r["lambda_final"] == pytest.approx(1e-8, rel=1e-12) and r["last_delta_norm"] == 1e-4
    r = replay(10.0, [5.0, 5e-5, 1e-5], walk=walk)                                      # chi2 <= epsilon_abs
    assert r["n"] == 2 and r["chi2_final"] == 5e-5
    assert replay(5e-5, [1e-5], walk=walk)["n"] == 0                                    # ... before the first trial


@REPLAYS
def test_only_a_last_trial_that_was_not_pd_is_reported(replay, walk):
    # a not-PD factorisation leaves garbage: its chi2 is worse, LM rejects the step and raises lambda
    r = replay(10.0, [50.0, 5.0, 4.0], notpd=[1.0, 0.0, 0.0], walk=walk)
    assert r["n"] == 3 and list(r["verdict"]) == [REJECTED, ACCEPTED, ACCEPTED]
    assert r["rc"] == PPS_OK and r["lm_trials_notpd"] == 1
    assert r["lam"][1] == pytest.approx(1e-5, rel=1e-12)
    r = replay(10.0, [5.0, 50.0], notpd=[0.0, 1.0], max_iterations=2, walk=walk)        # the trial the loop ended on
    assert r["n"] == 2 and list(r["verdict"]) == [ACCEPTED, REJECTED]
    assert r["rc"] == PPS_ENOTPD and r["lm_trials_notpd"] == 1
    # the pending step of a loop that ends on max_iterations is the last trial too (solved, never judged)
    r = replay(10.0, [5.0, 4.0], notpd=[0.0, 1.0], max_iterations=1, walk=walk)
    assert r["n"] == 1 and r["rc"] == PPS_ENOTPD
    # ... but a set's second record is a step only once it is about to be judged: trial 0 ends the loop, the not-PD word behind it is never taken
    r = replay(10.0, [5.0, 50.0], notpd=[0.0, 1.0], epsilon_rel=0.9, walk=walk)
    assert r["n"] == 1 and list(r["verdict"]) == [CONVERGED] and r["rc"] == PPS_OK and r["lm_trials_notpd"] == 0


SUMMARY = ("rc", "iterations", "lm_iterations", "chi2_final", "lambda_final", "last_delta_norm", "lm_trials_notpd", "lm_trials_accepted",
           "lm_trials_rejected")


def expected_counts(verdicts, mode):
    """What the scheme asks for, from the verdicts alone: the first set, then one set per accepted (not converged) trial -- a relinearisation --
    and one per rejection that finds no second record; every other rejection takes the second record of its set."""
    two = mode == WALK_TWO
    c = dict(sets=1, second=0, relaunch=0, relin=0, single=0 if two else 1)
    have_next, record = two, 0
    for v in verdicts:
        if v == CONVERGED:
            break
        if v == REJECTED and have_next:
            c["second"] += 1
            have_next, record = False, 1
            continue
        c["relin" if v == ACCEPTED else "relaunch"] += 1
        if mode == WALK_ADAPTIVE:
            two = v == REJECTED or record == 1                       # one trial after an immediate acceptance, two after a rejection
        c["sets"] += 1
        c["single"] += 0 if two else 1
        have_next, record = two, 0
    return c


@pytest.mark.parametrize("mode", [WALK_ONE, WALK_TWO, WALK_ADAPTIVE], ids=["one", "two", "adaptive"])
@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(f)[:-5] for f in FIXTURES])
def test_the_walk_replays_what_the_one_step_loop_replays(replay, path, mode):
    fx = json.load(open(path))
    chi2 = [c for _, c, _ in fx["lm_trace"]]
    a, b = replay(fx["chi2_initial"], chi2), replay(fx["chi2_initial"], chi2, walk=mode)
    assert b["n"] == a["n"] == len(chi2)
    for key in ("lam", "chi2", "acc", "verdict"):
        assert np.array_equal(a[key], b[key]), key                  # the trace and the verdicts, bit for bit
    assert [a[k] for k in SUMMARY] == [b[k] for k in SUMMARY]
    want = expected_counts(list(a["verdict"]), mode)
    assert {k: b[k] for k in want} == want
    n_rej = sum(1 for t in fx["lm_trace"] if not t[2])
    assert b["second"] + b["relaunch"] == n_rej                     # every rejection is answered by one of the two
    if mode == WALK_ONE:                                            # the one-step loop: never a second record
        assert b["second"] == 0 and b["single"] == b["sets"] and b["relaunch"] == n_rej
    if n_rej == 0:
        assert b["second"] == b["relaunch"] == 0


def test_the_counts_of_the_one_trajectory_with_rejections(replay):
    """hard_40p_6l, 76 trials of which 40 rejected: launch sets | second records | both-rejected relaunches | relinearisations | single-trial sets"""
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "hard_40p_6l.json")))
    chi2 = [c for _, c, _ in fx["lm_trace"]]
    got = {m: replay(fx["chi2_initial"], chi2, walk=m) for m in (WALK_TWO, WALK_ADAPTIVE)}
    keys = ("sets", "second", "relaunch", "relin", "single")
    assert [got[WALK_TWO][k] for k in keys] == [50, 26, 14, 35, 0]
    assert [got[WALK_ADAPTIVE][k] for k in keys] == [52, 24, 16, 35, 19]


def test_the_rotation_keeps_the_three_state_copies_apart(replay):
    """Every accept sequence of up to six launch sets, ended by a converged trial 0 / 1 or by a dropped step, against three labelled buffers:
    a set's trials are written to two copies that are not the linearisation point, the next linearisation point is the copy that holds the
    accepted trial, and the final copy holds the converged trial -- or the last accepted one when the pending step is dropped."""
    lib = replay.lib
    for n in range(7):
        for seq in itertools.product((0, 1), repeat=n):
            for end in (-1, 0, 1):
                cur = np.asarray(seq + (0,), dtype=np.int32)
                places = np.full(3 * (n + 1), -1, dtype=np.int32)
                fin = lib.lm_host_rotation(n, cur.ctypes.data_as(_ip), end, places.ctypes.data_as(_ip))
                buf = ["start", None, None]                         # what each copy holds
                at_x = "start"                                      # what the linearisation point must hold
                assert places[0] == 0
                for i in range(n + 1):
                    x, t0, t1 = (int(v) for v in places[3 * i:3 * i + 3])
                    assert sorted((x, t0, t1)) == [0, 1, 2], (seq, end, i)
                    assert buf[x] == at_x, (seq, end, i)
                    buf[t0], buf[t1] = (i, 0), (i, 1)               # the set writes both trials, each its whole copy
                    taken = seq[i] if i < n else end
                    if taken >= 0:
                        at_x = (i, taken)
                assert 0 <= fin <= 2 and buf[fin] == at_x, (seq, end, fin)
