"""Plane association and re-projection against an arbitrary-precision statement (oracle/mp_assoc.py, mpmath at 60 digits) -- on the host.

tests/golden/mp_assoc_cases.json holds atoms (one query, a handful of landmarks, the exact per-pair quantities, their conditioning units
and the gate each pair leaves the loop at), three synth.assoc_scene tables classified by the statement, and re-projection cases.  The
statement says for every pair whether rounding may change the outcome (decidedness); wherever it may not, the winner must be equal and the
score within K u(total), K = max(8, 4 rho of the CPU oracle) <= 256 from the fixture's "measured" block.  Held to it here: the C oracle
(oracle/pps_oracle.c) and oracle/numpy_assoc.py.  The mutant table is the evidence that tests/test_gpu_mp_assoc.py would fail on a subtly
wrong kernel: a parameterised copy of the gates and the fold (tests/assoc_mp_helpers.py -- test code, never the product) is run with one
mutation at a time, and every mutation must change the answer of at least one named atom.

Equality of a double gate (angle, plane distance) with its threshold is not tested: stored planes are re-normalised, so no API input
produces it."""
import os

import numpy as np
import pytest

import assoc_mp_helpers as H
from oracle import mp_assoc as MA
from oracle import numpy_assoc as NA
from oracle import oracle_py as O


@pytest.fixture(scope="module")
def fx():
    return H.load()


def _queries(fx):
    """(name, pose, frame, query, landmarks, params, best, err, u_err) of every decided query: atoms, then scenes under both parameter sets"""
    for a in fx["atoms"]:
        yield a["name"], a["pose"], a["frame_seq_id"], a["query"], a["landmarks"], MA.atom_params(fx, a), a["best"], a["err"], a["u_err"]
    for s in fx["scenes"]:
        for pname, rows in s["results"].items():
            for i, (q, r) in enumerate(zip(s["queries"], rows)):
                if r["decided"]:
                    yield "%s/%s/%d" % (s["name"], pname, i), s["pose"], s["frame_seq_id"], q, s["landmarks"], fx["params"][pname], r["best"], \
                        r["err"], r["u_err"]


def test_fixture_holds_what_it_claims(fx):
    tags = {t for a in fx["atoms"] for t in a["tags"]}
    assert not [t for t in H.REQUIRED_TAGS if t not in tags]
    assert {a["params"] for a in fx["atoms"] if isinstance(a["params"], str)} == {"defaults", "tum"}
    assert all(a["decided"] and all(p["decided"] for p in a["pairs"]) for a in fx["atoms"])             # no undecided atom
    rows = [r for s in fx["scenes"] for rs in s["results"].values() for r in rs]
    assert len(fx["scenes"]) == 3 and sum(not r["decided"] for r in rows) <= MA.SCENE_UNDECIDED_CAP * len(rows)
    assert sum(r["best"] >= 0 for r in rows) >= len(rows) // 2 and sum(r["n_pass"] > 1 for r in rows) >= 6
    assert os.path.getsize(MA.FIXTURE) < 300_000
    assert set(fx["measured"]) == {"total", "reproject"}
    for key, v in fx["measured"].items():
        assert v["K"] == float("%.3g" % MA.R.bound(v["rho_oracle"])) and 8.0 <= v["K"] <= 256.0, key
    # the stored verdicts are what the stored quantities give under the unmutated copy of the gates, pair by pair, and the stored fold
    for a in fx["atoms"]:
        (best, err), pairs = H.atom_answer(fx, a)
        assert [g for g, _ in pairs] == [p["gate"] for p in a["pairs"]], a["name"]
        assert best == a["best"] == H.stored_answer(a)[0], a["name"]
        assert H.same_score(err, a["err"], 1e-15 * max(1.0, abs(a["err"])), 8), a["name"]
    # every one of the seven gates is reached by a rejected subject whose twin passes
    rej = {a["claims"]["gate"] for a in fx["atoms"] if a["name"].endswith("/reject")}
    assert rej == set(MA.GATES)


def test_fixture_regenerates_bit_for_bit(fx):
    """every committed number is what the 60-digit statement rounds to, and the generator's own assertions hold (every atom decided and
    holding its claim, at most 2 % of the scene queries undecided)"""
    try:
        import mpmath  # noqa: F401
    except ImportError:
        pytest.skip("mpmath is not installed: the committed fixture cannot be regenerated here")
    new = MA.generate()
    for part in ("atoms", "scenes", "reproject"):
        assert [c["name"] for c in new[part]] == [c["name"] for c in fx[part]]
        for a, b in zip(new[part], fx[part]):
            assert _canon(a) == _canon(b), a["name"]


def _canon(x):
    """floats by their bits (NaN equal to NaN), tuples as lists"""
    if isinstance(x, dict):
        return {k: _canon(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_canon(v) for v in x]
    if isinstance(x, float):
        return np.float64(x).tobytes()
    if isinstance(x, (int, np.integer)) and not isinstance(x, bool):
        return np.float64(x).tobytes()
    return x


def test_measure_reproduces_the_stored_rho(fx):
    got = MA.measure(fx)
    assert set(got) == set(fx["measured"])
    for key, v in fx["measured"].items():
        assert got[key]["rho_oracle"] <= max(1.3 * v["rho_oracle"], v["rho_oracle"] + 0.5), (key, got[key], v)     # another libm may move it
        assert got[key]["K"] <= max(v["K"], 8.0), key


@pytest.mark.parametrize("who", ["c_oracle", "numpy_assoc"])
def test_restatements_against_the_statement(fx, who):
    """every decided query: the winner is equal, the score within K u(total), NaN where the statement says NaN"""
    K, worst, n = H.K_of(fx, "total"), 0.0, 0
    for name, pose, fsi, q, lms, prm, best, err, u in _queries(fx):
        if who == "c_oracle":
            b, e = O.find_closest_plane(pose, q["plane"], q["fpi"], fsi, q["seg2d"], q["seg3d"], lms, **prm)
        else:
            b, e = NA.find_closest_plane(pose, q["plane"], q["fpi"], fsi, q["seg2d"], q["seg3d"], lms, **prm)
        assert b == best, (who, name, b, best)
        assert H.same_score(e, err, u, K), (who, name, e, err, u)
        worst = max(worst, H.score_ratio(e, err, u))
        n += 1
    assert n >= len(fx["atoms"]) + 40
    print("\n%s against the 60-digit statement: %d decided queries, worst score ratio %.3g (K = %g)" % (who, n, worst, K))


def test_reprojection_oracle_against_the_statement(fx):
    K = H.K_of(fx, "reproject")
    for c in fx["reproject"]:
        assert MA.reproject_ratio(c, O.project_to_plane(c["plane"], c["point"])) <= K, c["name"]


@pytest.mark.parametrize("mut", H.MUTANTS)
def test_every_mutant_is_caught_by_a_named_atom(fx, mut):
    caught = []
    for a in fx["atoms"]:
        (best, err), _ = H.atom_answer(fx, a, mut)
        if best != a["best"] or not H.same_score(err, a["err"], max(a["u_err"], 1e-15), H.K_of(fx, "total")):
            caught.append(a["name"])
    print("\n%s: caught by %s" % (mut, ", ".join(caught)))
    assert caught, mut


def test_the_symmetric_swap_changes_nothing(fx):
    """d2 and d2c enter the gate and the score symmetrically: swapping their roles is not a mutation of the decision function"""
    for mut in H.EQUIVALENT_MUTANTS:
        for a in fx["atoms"]:
            (best, err), _ = H.atom_answer(fx, a, mut)
            assert best == a["best"] and H.same_score(err, a["err"], 1e-15 * max(1.0, abs(a["err"])), 8), (mut, a["name"])
