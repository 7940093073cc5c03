"""GPU: the stretch between an LM trial and the next factorisation.  k_trial_lin publishes the two trial records without release fences
(the record leaves when the trial blocks are done, not when the linearisation sweep of the same launch has written its output back), and
the dual LM loop keeps only the rule, the pointer rotation and the launch between a record's arrival and the factor launch.  Neither
changes what is computed: PPS_NO_EARLY_RECORD / PPS_LM_PLAIN_HOST put each back, and every side must give the same LM trace, the same
state and the same counters, bit for bit.  A handle reads its switches when it is created, so the sides run in one process."""
import os

import numpy as np
import pytest

import pop_up_slam_amd as P
from pop_up_slam_amd import synth

pytestmark = pytest.mark.gpu

NEW_SWITCHES = ("PPS_NO_EARLY_RECORD", "PPS_LM_PLAIN_HOST")
ALL_SWITCHES = NEW_SWITCHES + ("PPS_NO_SPEC_LIN",)
GRAPHS = {"120p": lambda: synth.corridor(120, 26, seed=7), "c2": lambda: synth.corridor()}


def _graph(spec, switch=None):
    """a handle created with `switch` set (and none of the others), the variable gone again before anything runs"""
    saved = {k: os.environ.pop(k) for k in ALL_SWITCHES if k in os.environ}
    try:
        if switch:
            os.environ[switch] = "1"
        g = P.Graph()
    finally:
        for k in ALL_SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(saved)
    nid, _ = spec.replay(g)
    return g, nid


def _solve(g):
    it = g.batch_optimize()
    st = g.stats()
    return {"it": it, "trace": g.trace(), "chi2": g.chi2(), "poses": g.get_poses(), "planes": g.get_planes(),
            "n_linearize": st["n_linearize"], "n_factorize": st["n_factorize"], "accepted": st["lm_trials_accepted"], "rejected": st["lm_trials_rejected"]}


def _same(a, b, what):
    assert a["it"] == b["it"] and a["trace"] == b["trace"] and a["chi2"] == b["chi2"], what
    np.testing.assert_array_equal(a["poses"], b["poses"], err_msg=str(what))
    np.testing.assert_array_equal(a["planes"], b["planes"], err_msg=str(what))
    assert (a["accepted"], a["rejected"]) == (b["accepted"], b["rejected"]), what


@pytest.fixture(scope="module")
def default_runs(built):
    """the shipped schedule on both graphs, solved once and shared"""
    out = {}
    for name, make in GRAPHS.items():
        spec = make()
        g, _ = _graph(spec)
        out[name] = _solve(g)
        g.close()
    return out


def _launch_sets(trace):
    """Replays the dual loop's bookkeeping over an LM trace [(lambda, chi2, accepted)]: a launch set carries trial 0 (lambda) and trial 1
    (lambda * factor) of one linearisation, and the sweep inside its trial launch is made at the trial accepted LAST time.  Returns
    (launch sets, wrong predictions, launch sets with both trials rejected)."""
    sets = wrong = both_rejected = 0
    pred, k = 0, 0
    while k < len(trace):
        sets += 1
        if trace[k][2]:                         # trial 0 accepted
            wrong += pred != 0; pred = 0; k += 1
        elif k + 1 < len(trace) and trace[k + 1][2]:
            wrong += pred != 1; pred = 1; k += 2
        elif k + 1 < len(trace):
            both_rejected += 1; k += 2
        else:
            k += 1
    return sets, wrong, both_rejected


@pytest.mark.parametrize("switch", ALL_SWITCHES)
@pytest.mark.parametrize("name", list(GRAPHS))
def test_lm_trace_is_the_same_with_each_switch_off(default_runs, name, switch):
    """default against PPS_NO_EARLY_RECORD, PPS_LM_PLAIN_HOST and PPS_NO_SPEC_LIN: lambda, chi2 and verdict of every trial, the iteration
    count, the final state and the trial counters.  On C2 the trace must contain what exercises the paths behind a record: a wrong
    prediction (the plain sweep runs into the current set while the spare set may still be being written) and a launch set with both
    trials rejected (the same H is factored again)."""
    spec = GRAPHS[name]()
    g, _ = _graph(spec, switch)
    got = _solve(g)
    g.close()
    ref = default_runs[name]
    assert ref["it"] >= (10 if name == "c2" else 2)      # (the small corridor converges in a few trials; C2 takes some sixty)
    _same(got, ref, (name, switch))
    if switch != "PPS_NO_SPEC_LIN":
        assert got["n_linearize"] == ref["n_linearize"] and got["n_factorize"] == ref["n_factorize"]
    if name == "c2":
        sets, wrong, both = _launch_sets(ref["trace"])
        print("C2: %d launch sets, %d wrong predictions, %d with both trials rejected" % (sets, wrong, both))
        assert wrong >= 1 and both >= 1


@pytest.mark.parametrize("name", list(GRAPHS))
def test_a_second_solve_on_the_handle_repeats_the_first(default_runs, name):
    """the record says the trials are done, not the sweep of the same launch: a solve must still return only when everything it queued has
    ended.  restore_state + batch_optimize on the same handle, profiling off, twice: each repeats the first solve bit for bit (a sweep still
    writing the spare set, or a trial copy still being read, when the solve returned would show here), with the counters of the fenced
    schedule."""
    spec = GRAPHS[name]()
    g, _ = _graph(spec)
    g.save_state()
    first = _solve(g)
    _same(first, default_runs[name], name)
    for rep in range(2):
        g.restore_state()
        again = _solve(g)
        _same(again, first, (name, rep))
        assert again["n_linearize"] == first["n_linearize"] and again["n_factorize"] == first["n_factorize"]
    g.close()
    h, _ = _graph(spec, "PPS_NO_EARLY_RECORD")
    fenced = _solve(h)
    h.close()
    assert fenced["n_linearize"] == first["n_linearize"] and fenced["trace"] == first["trace"]
