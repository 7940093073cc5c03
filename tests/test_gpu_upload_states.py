"""GPU: incremental uploads held to a rebuild-everything twin, bit for bit.

Every script of upload_state_helpers.py goes into twin handles, both created under PPS_DEBUG_VERIFY_UPLOAD=1: I with the default switches --
kept-prefix hints, incrementally packed factor arrays, measurements that stay on the device across appending uploads -- and S under
PPS_NO_INCREMENTAL=1 and PPS_NO_INCR_COMPACT=1, whose every analysis starts from scratch on rebuilt tables and whose uploads therefore take no
kept-prefix hints.  (The incremental packing, pk_meas_ok, keep_meas and the cached frame tables do not read these switches and run in S as in
I: they are pinned by the verification switch and by the expected measurements, not by the twin.)
Both run the same kernels on arrays that must be equal, so after every solve or read chi2(), the LM trace, the iteration count,
stats()["chi2_final"] and ["last_delta_norm"], debug_solve's step, eval_factor's J and r, the covariance blocks and -- where the script reads
them -- every pose, plane and plane-observation measurement are compared bit for bit, after analysis_dump() of both.  I is also held to the
script's expected measurements (1e-15 absolute, the bound of test_refresh_measurements_feeds_the_graph) and to the oracle (the tolerances of
test_gpu_fuzz.py).  The verification switch itself checks, after every flush, the packed arrays against a pack from the host factor records,
ea_tgt / el_tgt / blk_dst against expand_ea_tgt / expand_el_lists on the host, and the zeroed block behind delta (csrc/pps_upload.cpp).

The whole set runs once more in a child process under PPS_PLAIN_SCHEDULE=8, where the lists are expanded by k_expand_ea, two fills and
k_expand_el instead of the one launch of k_expand_lists."""
import json
import os
import subprocess
import sys

import pytest

import upload_state_helpers as H

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(script, monkeypatch):
    gi, gs = H.twin_handles(monkeypatch.setenv, monkeypatch.delenv)
    run = H.TwinRun(script, gi, gs).run()
    gi.close(); gs.close()
    return run


@pytest.mark.parametrize("seed", H.SEEDS)
def test_seeded_scripts_on_twins_and_the_oracle(built, monkeypatch, seed):
    s = H.make_script(seed, H.STEPS, huber=seed == H.HUBER_SEED)
    run = _run(s, monkeypatch)
    assert run.n_checks == sum(s.solves.values()) >= H.STEPS
    assert run.n_cov_blocks == 3, (run.n_cov_blocks, run.cov_form)      # real blocks were compared, in every script
    if seed == H.HUBER_SEED:
        assert sum(1 for op in s.ops if op[0] == "cost") == 2


DIRECTED = ["keep_meas", "refresh_remove", "refresh_obs2", "set_after_refresh", "set_pose_device_newer", "remove_after_growth", "capacity_16_32",
            "unchanged_twice", "first_repop_edge"]


@pytest.mark.parametrize("name", DIRECTED)
def test_directed_scripts_on_twins_and_the_oracle(built, monkeypatch, name):
    scripts = {s.name: s for s in H.directed_scripts()}
    assert list(scripts) == DIRECTED
    run = _run(scripts[name], monkeypatch)
    assert run.n_checks == sum(scripts[name].solves.values()) >= 2


CHILD = r"""
import json, os, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import upload_state_helpers as H
print("RESULT " + json.dumps(H.run_all(os.environ.__setitem__, lambda k: os.environ.pop(k, None))))
""" % (ROOT, os.path.join(ROOT, "tests"))


def test_the_whole_set_with_the_split_expansion(built):
    """PPS_PLAIN_SCHEDULE=8 for the whole process, as tests/test_gpu_switches.py sets it: k_expand_ea + fills + k_expand_el"""
    e = dict(os.environ)
    for k in ("PPS_NO_INCREMENTAL", "PPS_NO_INCR_COMPACT", "PPS_DEBUG_VERIFY_UPLOAD"):
        e.pop(k, None)
    e["PPS_PLAIN_SCHEDULE"] = "8"
    r = subprocess.run([sys.executable, "-c", CHILD], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    got = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    assert list(got) == [f"seed{s}" for s in H.SEEDS] + DIRECTED and all(n >= 2 for n, _c in got.values()), got
    assert all(got[f"seed{s}"][1] == 3 for s in H.SEEDS), got
