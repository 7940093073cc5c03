"""CPU: the edit scripts of upload_state_helpers.py on two handles without a device -- one with the default switches, one created under
PPS_NO_INCREMENTAL=1 and PPS_NO_INCR_COMPACT=1, whose every analysis rebuilds the compacted tables and starts from scratch.  Solves, reads and
refreshes are replaced by analyze(); after every analysis every analysis_dump array must be equal.  This is the host parity of
test_host_incremental.py under the edit kinds of the upload-state scripts: re-popping observations (whose slots sit behind the fixed ones
and move), set_pose / set_plane / set_measurement(s), priors on old poses, registered frames, removal of the newest pose, repeated analyses.

The coverage conditions are asserted from the scripts' own logs, so that a run cannot pass by doing nothing.  Over the seed set every edit kind
and every solve kind occurs at least three times; every seeded script skips at most one drawn edit in four for an unmet precondition, has an
analysis that builds on the previous one (analysis_reuse()[0] > 0), one from scratch after a removal (reuse 0), and one that keeps fronts
while every buffer offset moved (analysis_kept(): fronts > 0, fronts_lists == 0 -- a Jacobian slab outgrew its capacity).  The directed scripts
are a handful of calls each and are held to the parity only."""
import collections

import numpy as np
import pytest

import pop_up_slam_amd as P
import upload_state_helpers as H

SEEDS, STEPS, HUBER_SEED = list(H.SEEDS), H.STEPS, H.HUBER_SEED


def _scratch_graph(monkeypatch):
    """a handle whose every analysis starts from scratch: the switches are read once, when the handle is created"""
    monkeypatch.setenv("PPS_NO_INCREMENTAL", "1"); monkeypatch.setenv("PPS_NO_INCR_COMPACT", "1")
    g = P.Graph()
    monkeypatch.delenv("PPS_NO_INCREMENTAL"); monkeypatch.delenv("PPS_NO_INCR_COMPACT")
    return g


def _kept_claims_hold(a, prev, kp, where):
    """Analysis::Kept names leading parts of the index arrays that the upload does not compare with its mirror again: every claim against
    the previous analysis' arrays (the checks of test_kept_parts_are_what_the_previous_analysis_held, here under every edit kind)"""
    F, Fl, B, S, Cn, ND = kp["fronts"], kp["fronts_lists"], kp["blocks"], kp["segs"], kp["contribs"], kp["nd_segs"]
    assert Fl <= F, (where, kp)

    def same(name, count):
        count = int(count)
        assert count <= len(a[name]) and count <= len(prev[name]), (where, name, count)
        np.testing.assert_array_equal(a[name][:count], prev[name][:count], err_msg=f"{where}: {name}[:{count}]")
    for name in ("f_p", "f_b", "f_poff", "f_Loff", "f_Uoff"): same(name, F)
    for name in ("f_bidx_off", "f_child_off", "f_cmap_off", "f_ea_off"): same(name, F + 1)
    same("pidx", a["f_poff"][F] if F < len(a["f_poff"]) else 0)
    same("bidx", a["f_bidx_off"][F]); same("child", a["f_child_off"][F])
    if Fl > 0:
        for name in ("f_asm_off", "f_el_off"): same(name, Fl + 1)
        for name in ("asm_blk", "asm_lrow", "asm_lcol"): same(name, a["f_asm_off"][Fl])
    for name in ("blk_rows", "blk_cols", "blk_size", "blk_nseg", "blk_hoff"): same(name, B)
    if B > 0: same("blk_doff", B + 1)
    for name in ("seg_blk", "seg_c0", "seg_cnt", "seg_hoff"): same(name, S)
    same("srec", 8 * S); same("contrib", 4 * Cn); same("nd_segs", ND)


def run_host(script, monkeypatch):
    """returns per analysis (reuse, fronts, fronts kept, fronts_lists kept, a removal since the last analysis?)"""
    gi, gs = P.Graph(), _scratch_graph(monkeypatch)
    ids = [([], []), ([], [])]
    seen = []
    removed = False
    prev = None
    for k, op in enumerate(script.ops):
        construction = [H.apply_edit(g, op, *ids[w]) for w, g in enumerate((gi, gs))][0]
        if op[0] in ("rmf", "rmn"):
            removed = True
        if construction or op[0] in ("save", "restore", "cost", "cov"):
            continue
        assert op[0] in ("solve", "refresh", "analyze"), op[0]
        gi.analyze(); gs.analyze()
        assert gs.analysis_reuse()[0] == 0
        a, b = gi.analysis_dump(), gs.analysis_dump()
        assert a.keys() == b.keys()
        for key in b:
            np.testing.assert_array_equal(np.atleast_1d(a[key]), np.atleast_1d(b[key]), err_msg=f"{script.name} op {k} {op[0]}: {key}")
        kept = gi.analysis_kept()
        if gi.analysis_reuse()[0] == 0:
            assert all(v == 0 for v in kept.values()), (script.name, k, kept)      # from scratch: nothing claimed
        elif prev is not None and kept["fronts"] > 0:
            _kept_claims_hold(a, prev, kept, f"{script.name} op {k}")
        prev = a
        seen.append((gi.analysis_reuse()[0], gi.analysis_reuse()[1], kept["fronts"], kept["fronts_lists"], removed))
        removed = False
    assert ids[0] == ids[1]
    gi.close(); gs.close()
    return seen


@pytest.fixture(scope="module")
def scripts():
    return {seed: H.make_script(seed, STEPS, huber=seed == HUBER_SEED) for seed in SEEDS}


def test_scripts_are_pure_functions_of_their_seed():
    a, b = H.make_script(5, STEPS), H.make_script(5, STEPS)
    assert len(a.ops) == len(b.ops) and a.log == b.log
    for x, y in zip(a.ops, b.ops):
        assert x[0] == y[0] and len(x) == len(y)
        for u, v in zip(x[1:], y[1:]):
            assert np.array_equal(np.asarray(u), np.asarray(v)), (x[0], u, v)


def test_the_seed_set_covers_every_edit_and_solve_kind(scripts):
    edits, solves = collections.Counter(), collections.Counter()
    for s in scripts.values():
        edits.update(kind for kind, ok in s.log if ok)
        solves.update(s.solves)
        assert sum(1 for op in s.ops if op[0] == "cov") == 1
    assert all(edits[k] >= 3 for k in H.EDIT_KINDS), {k: edits[k] for k in H.EDIT_KINDS}
    assert all(solves[k] >= 3 for k in H.SOLVE_KINDS), dict(solves)
    starts = [sum(1 for op in s.ops[:s.ops.index(next(o for o in s.ops if o[0] == "solve"))] if op[0] == "pose") for s in scripts.values()]
    assert any(6 <= n <= 30 for n in starts) and any(120 <= n <= 300 for n in starts), starts


@pytest.mark.parametrize("seed", SEEDS)
def test_incremental_analysis_equals_analysis_from_scratch_under_every_edit_kind(built, monkeypatch, scripts, seed):
    s = scripts[seed]
    assert len(s.log) == STEPS and 4 * s.skipped() <= len(s.log), s.log
    assert s.crossed
    seen = run_host(s, monkeypatch)
    assert any(reuse > 0 for reuse, *_ in seen), seen
    assert any(reuse == 0 and removed for reuse, _n, _f, _fl, removed in seen), seen
    assert any(f > 0 and fl == 0 for _r, _n, f, fl, _rm in seen), seen


@pytest.mark.parametrize("k", range(9))
def test_directed_scripts_on_the_host(built, monkeypatch, k):
    s = H.directed_scripts()[k]
    seen = run_host(s, monkeypatch)
    assert len(seen) >= 2
