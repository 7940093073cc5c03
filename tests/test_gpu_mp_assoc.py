"""GPU: plane association (k_assoc behind pps_find_closest_planes) and re-projection (k_reproject behind pps_reproject_points) against the
arbitrary-precision statement of oracle/mp_assoc.py.

Reads tests/golden/mp_assoc_cases.json only (no mpmath here).  The statement says per (query, landmark) pair which gate the pair leaves the
loop at and whether rounding may change that (decidedness); on every decided query the device must name the same landmark and give the
score within K u(total) -- NaN where the statement says NaN --, K = max(8, 4 rho of the CPU oracle) <= 256 from the fixture's "measured"
block.  tests/test_host_mp_assoc.py shows with a table of mutants that each gate, rule and tie-break is pinned by a named atom.
  * atoms and scenes, the planes once from host values (no solve yet) and once from the solver state: every plane pinned at the fixture's
    value by a plane prior, batch_optimize, the margins re-checked against the downloaded estimate (assoc_mp_helpers.shift_bounds)
  * tables of 1 ... 1025 landmarks composed of an atom's landmarks and decided-reject fillers: the strided loop, cand_merge, first against
    best, ties inside a thread and between neighbours, the NaN rule across threads, 1 / 64 / 65 queries per call
  * one handle across calls: both capacities grow, the landmark records are re-uploaded when the source of the planes switches
  * pps_reproject_points against point - n (n . point - d) on the stored 4-vector, in units of u = one ulp of each of the four doubles +
    half an fp32 ulp of the result, bound K of `reproject`.  tests/test_gpu_map.py ties k_map_build to these bits.
`pytest -s` prints the device's worst ratio per quantity (profiles/mp_assoc_device_rho.txt is one such run).  Equality of a double gate with
its threshold is not tested: stored planes are re-normalised, no API input produces it."""
import numpy as np
import pytest

import assoc_mp_helpers as H
import pop_up_slam_amd as P
from oracle import mp_assoc as MA

pytestmark = pytest.mark.gpu
STRONG = [1e3, 0.0, 0.0, 1e3, 0.0, 1e3]             # sqrt information of the pinning priors, packed upper triangle
WORST = {}


@pytest.fixture(scope="module")
def fx():
    return H.load()


def _graph(lms, priors=False):
    g = P.Graph()
    nodes = []
    for L in lms:
        n = g.add_plane(L["plane"])
        nodes.append(n)
        g.landmark_update(n, L["fpi"], L["seq"], L["seg2d"], L["seg3d"])
        if L["deleted"]:
            g.landmark_set_merged(n)
        if priors:
            g.add_plane_prior(n, L["plane"], STRONG)
    return g, nodes


class Pool:
    """one graph whose n landmark records are rewritten in place (set_plane, landmark_update, the pinning prior's measurement): a handle
    per table would cost more than every launch of this file together.  A merged landmark cannot be revived, so tables that hold one get a
    graph of their own (_table_graph)"""
    BLANK = dict(plane=[0.0, 0.0, -1.0, 0.0], fpi=0, seq=0, deleted=0, seg2d=[0.0] * 4, seg3d=[0.0] * 4)

    def __init__(self, n, priors=False):
        self.g = P.Graph()
        self.nodes = [self.g.add_plane(self.BLANK["plane"]) for _ in range(n)]
        self.fids = [self.g.add_plane_prior(k, self.BLANK["plane"], STRONG) for k in self.nodes] if priors else None
        self.cur = [None] * n

    def load(self, lms):
        """the table becomes lms (as long as the pool); only the records that differ are rewritten"""
        assert len(lms) == len(self.cur) and not any(L["deleted"] for L in lms)
        for i, L in enumerate(lms):
            if self.cur[i] is not L and repr(self.cur[i]) != repr(L):         # repr: a NaN in seg3d equals itself
                self.g.set_plane(self.nodes[i], L["plane"])
                self.g.landmark_update(self.nodes[i], L["fpi"], L["seq"], L["seg2d"], L["seg3d"])
                if self.fids:
                    self.g.set_measurement(self.fids[i], L["plane"])
                self.cur[i] = L
        return self.g, self.nodes


_POOLS = {}


def _table_graph(lms):
    """(graph, nodes) holding the table lms, planes from host values"""
    if any(L["deleted"] for L in lms):
        return _graph(lms)
    if len(lms) not in _POOLS:
        _POOLS[len(lms)] = Pool(len(lms))
    return _POOLS[len(lms)].load(lms)


def _find(g, pose, fsi, queries, prm):
    return g.find_closest_planes(pose, fsi, [q["plane"] for q in queries], [q["fpi"] for q in queries], [q["seg2d"] for q in queries],
                                 [q["seg3d"] for q in queries], **prm)


def _check(fx, name, got_id, got_err, nodes, best, err, u, extra=0.0):
    want = nodes[best] if best >= 0 else -1
    assert got_id == want, "%s: landmark %d, the statement says %d" % (name, got_id, want)
    K = H.K_of(fx, "total")
    assert H.same_score(got_err, err, u + extra / K, K), "%s: score %r, the statement says %r, unit %.3g, K = %g" % (name, got_err, err, u, K)
    if u > 0 and err == err:
        WORST["total"] = max(WORST.get("total", 0.0), max(abs(got_err - err) - extra, 0.0) / u)


def _still_decided(fx, pose, lms, est, rows, ang_thr):
    """the solver state moved the planes by `est - fixture`: the shift any angle, plane distance and score can take, and whether the
    margins of the statement survive it.  rows: (m_angle, u_angle, m_plane_dist, u_plane_dist, sep) of what must stay decided"""
    da = dp = 0.0
    for L, e in zip(lms, est):
        a, p = H.shift_bounds(pose, L["plane"], e)
        da, dp = max(da, a), max(dp, p)
    dt = 3 * da / ang_thr + dp / 4
    K2 = 2 * MA.K_DECIDE
    ok = all(ma > K2 * ua + da and mp > K2 * up + dp and (sep is None or sep > 2 * dt) for ma, ua, mp, up, sep in rows)
    return ok, dt


def _atom_rows(a):
    return [(p.get("m_angle", 1.0), p.get("u_angle", 0.0), p.get("m_plane_dist", 1.0), p.get("u_plane_dist", 0.0), a["sep"]) for p in a["pairs"]]


@pytest.mark.parametrize("source", ["host_values", "solver_state"])
def test_atoms_and_scenes(built, fx, source):
    solver = source == "solver_state"
    n_seen = n_skipped = 0
    width = max(len(a["landmarks"]) for a in fx["atoms"])
    pool = Pool(width, priors=solver)
    for a in fx["atoms"]:
        prm = MA.atom_params(fx, a)
        if any(L["deleted"] for L in a["landmarks"]):
            g, nodes = _graph(a["landmarks"], priors=solver)
        else:                                                                 # the atom's landmarks, then fillers its query rejects by class
            g, nodes = pool.load(a["landmarks"] + [H.filler(a, k) for k in range(len(a["landmarks"]), width)])
            nodes = nodes[:len(a["landmarks"])]
        extra = 0.0
        n_seen += 1
        if solver:
            g.batch_optimize()
            est = g.get_planes(nodes)
            same = np.array_equal(est, np.array([L["plane"] for L in a["landmarks"]]))
            ok, extra = _still_decided(fx, a["pose"], a["landmarks"], est, _atom_rows(a), prm["edge_asso_angle"])
            if not ok or (a["artefacts"] and not same):                       # an artefact lives in the bits of its plane
                n_skipped += 1
                continue
        ids, errs = _find(g, a["pose"], a["frame_seq_id"], [a["query"]], prm)
        _check(fx, "%s (%s)" % (a["name"], source), ids[0], errs[0], nodes, a["best"], a["err"], a["u_err"], extra)
    for s in fx["scenes"]:
        g, nodes = _graph(s["landmarks"], priors=solver)
        est = None
        if solver:
            g.batch_optimize()
            est = g.get_planes(nodes)
        for pname, rows in s["results"].items():
            prm = fx["params"][pname]
            ids, errs = _find(g, s["pose"], s["frame_seq_id"], s["queries"], prm)
            for i, r in enumerate(rows):
                n_seen += 1
                extra = 0.0
                if r["decided"] and solver:
                    ok, extra = _still_decided(fx, s["pose"], s["landmarks"], est, [(r["slack_angle"], 0.0, r["slack_plane_dist"], 0.0, r["sep"])],
                                               prm["edge_asso_angle"])
                    r = dict(r, decided=ok)
                if not r["decided"]:
                    n_skipped += 1
                    continue
                _check(fx, "%s/%s/%d (%s)" % (s["name"], pname, i, source), ids[i], errs[i], nodes, r["best"], r["err"], r["u_err"], extra)
    print("\n%s: %d queries, %d not decided and skipped" % (source, n_seen, n_skipped))
    assert n_skipped <= MA.SCENE_UNDECIDED_CAP * n_seen, (n_skipped, n_seen)


def _atom(fx, name):
    return next(a for a in fx["atoms"] if a["name"] == name)


def _run_table(fx, a, n, places, name, n_queries=1):
    lms, pairs = H.compose(a, n, places)
    best, err, u = H.expected(a, pairs)
    g, nodes = _table_graph(lms)
    ids, errs = _find(g, a["pose"], a["frame_seq_id"], [a["query"]] * n_queries, MA.atom_params(fx, a))
    for i in range(n_queries):
        _check(fx, "%s n=%d %r" % (name, n, places), ids[i], errs[i], nodes, best, err, u)
    return best


SIZES = [1, 255, 256, 257, 511, 512, 513, 1025]


@pytest.mark.parametrize("n", SIZES)
def test_reduction_shapes(built, fx, n):
    """tie/duplicates holds ground, decoy D (passes, poor score), winner W and a bit-identical copy of W.  W at 0, 255, 256 and last; D --
    the first candidate that passes -- before and after it, in another thread and another stride; copies of W in the same thread (i + 256)
    and in the neighbouring one (i + 1)"""
    a = _atom(fx, "tie/duplicates")
    D, W = 1, 2
    assert a["pairs"][D]["gate"] == a["pairs"][W]["gate"] == "pass" and a["pairs"][W]["total"] < a["pairs"][D]["total"]
    done = 0
    for w in sorted({0, 255, 256, n - 1}):
        if w >= n:
            continue
        assert _run_table(fx, a, n, {W: w}, "winner alone") == w
        done += 1
        for d in (w + 257, w - 257, w + 1, w - 1, w + 256, w - 256, 0, n - 1):
            if 0 <= d < n and d != w:
                assert _run_table(fx, a, n, {W: w, D: d}, "first against best") == w
                done += 1
    for i in (0, 3, 255):
        for step in (1, 256):
            if i + step < n:
                assert _run_table(fx, a, n, {W: [i, i + step], D: (i + 2) % n if (i + 2) % n not in (i, i + step) else 5 % n}, "ties") == i
                done += 1
    assert done >= (1 if n == 1 else 8)


def test_nan_rule_across_threads(built, fx):
    """nan/segment_first holds ground, a landmark whose score is NaN by the reference's own comparisons, winner W and decoy D.  The NaN and
    the finite best sit in different threads and strides: NaN first of all sticks; a finite first keeps the NaN out; a NaN that is first
    in its thread but not first overall neither sticks nor hides the better candidate behind it in that thread"""
    a = _atom(fx, "nan/segment_first")
    N, W, D = 1, 2, 3
    assert a["pairs"][N].get("nan_segment") and a["pairs"][N]["gate"] == "pass"
    for n, places, want in ((513, {N: 3, W: 300, D: 7}, 3), (513, {N: 259, W: 2, D: 400}, 2), (513, {N: 300, W: 301, D: 2}, 301),
                            (1025, {D: 5, N: 262, W: 518}, 518), (1025, {N: 262, W: 518}, 262), (257, {N: 256, W: 0}, 0), (257, {N: 0, W: 256}, 0)):
        assert _run_table(fx, a, n, places, "nan") == want
    art = _atom(fx, "nan/artefact_first")
    assert art["pairs"][0]["artefact"]
    assert _run_table(fx, art, 600, {0: 2, 1: 300}, "artefact") == 2
    assert _run_table(fx, art, 600, {1: 2, 0: 300}, "artefact") == 2


def test_other_tables_and_query_counts(built, fx):
    for name, n, places, want in (("deleted/all", 513, {0: 0, 1: 256, 2: 512}, -1),
                                  ("ground/first_live", 513, {2: 0, 0: 5}, 0),                     # first live ground at index 0
                                  ("ground/first_live", 513, {1: 0, 0: 1, 3: 255, 2: 300, 4: 301}, 300),   # ... at 300 behind a deleted ground and walls
                                  ("class/grounds_only", 513, {0: 0, 1: 300}, -1)):
        a = _atom(fx, name)
        if name == "deleted/all":                                              # every entry deleted, the fillers too
            lms, _ = H.compose(a, n, places)
            g, nodes = _graph([dict(L, deleted=1) for L in lms])
            ids, errs = _find(g, a["pose"], a["frame_seq_id"], [a["query"]], MA.atom_params(fx, a))
            assert ids[0] == -1 and errs[0] == -1.0
            continue
        if name == "class/grounds_only":                                       # a wall query against grounds only: the fillers are grounds as well
            assert all(L["fpi"] == 0 for L in H.compose(a, n, places)[0])
        assert _run_table(fx, a, n, places, name) == want
    a = _atom(fx, "tie/duplicates")
    for nq in (1, 64, 65):
        assert _run_table(fx, a, 300, {1: 3, 2: 280}, "queries per call", n_queries=nq) == 280
    # 65 different queries in one call: the first scene's, cycled
    s = fx["scenes"][0]
    g, nodes = _graph(s["landmarks"])
    for pname, rows in s["results"].items():
        qs = [s["queries"][i % len(rows)] for i in range(65)]
        ids, errs = _find(g, s["pose"], s["frame_seq_id"], qs, fx["params"][pname])
        for i in range(65):
            r = rows[i % len(rows)]
            if r["decided"]:
                _check(fx, "scene query %d of 65" % i, ids[i], errs[i], nodes, r["best"], r["err"], r["u_err"])


def test_one_handle_across_calls(built, fx):
    """120 -> 200 -> 300 landmarks (the record capacity of 256 grows), 10 -> 70 queries (the query capacity of 64 grows), and the planes now
    from host values, now from the solver state: find, solve, find, grow, find, solve, find, set_plane, find, landmark_set_merged, find,
    remove_node, find, set_plane back, find, solve, find.  After every step the answer is the fold over the exact data of the table as it
    then is.  The angle twins differ in the plane alone, so set_plane turns the winner into a decided reject and back"""
    win, rej = _atom(fx, "gate/defaults/angle/twin"), _atom(fx, "gate/defaults/angle/reject")
    assert win["query"] == rej["query"] and win["landmarks"][1] == rej["landmarks"][1]
    assert {k: v for k, v in win["landmarks"][2].items() if k != "plane"} == {k: v for k, v in rej["landmarks"][2].items() if k != "plane"}
    D, W = 1, 2
    prm = MA.atom_params(fx, win)
    lms, pairs = H.compose(win, 120, {D: [10, 100]})
    g, nodes = _graph(lms, priors=True)
    gq = dict(plane=[0.0, 0.0, -1.0, 0.0], fpi=0, seg2d=[0.0] * 4, seg3d=[0.0] * 4)
    state = {"pairs": pairs, "nq": 10}

    def find(step, extra=0.0):
        best, err, u = H.expected(win, state["pairs"])
        qs = [win["query"]] * (state["nq"] - 1) + [gq]
        ids, errs = _find(g, win["pose"], win["frame_seq_id"], qs, prm)
        for i in range(state["nq"] - 1):
            _check(fx, "%s, query %d" % (step, i), ids[i], errs[i], nodes, best, err, u, extra)
        assert ids[-1] == nodes[0] and errs[-1] == -1.0, step                    # the ground query: filler 0 is the first live ground
        return best

    def solve(step):
        g.batch_optimize()
        est = g.get_planes([nodes[i] for i in range(len(lms)) if live[i]])
        rows = [(p.get("m_angle", 1.0), p.get("u_angle", 0.0), p.get("m_plane_dist", 1.0), p.get("u_plane_dist", 0.0), win["sep"])
                for p in win["pairs"] + rej["pairs"]]
        ok, extra = _still_decided(fx, win["pose"], [L for i, L in enumerate(lms) if live[i]], est, rows, prm["edge_asso_angle"])
        assert ok, step
        return extra

    def grow(n, places):
        more, mp = H.compose(win, n, places)
        for k in range(len(lms), n):
            L = more[k]
            node = g.add_plane(L["plane"])
            nodes.append(node)
            g.landmark_update(node, L["fpi"], L["seq"], L["seg2d"], L["seg3d"])
            g.add_plane_prior(node, L["plane"], STRONG)
            lms.append(L)
            state["pairs"].append(mp[k])
            live.append(True)
    live = [True] * len(lms)
    assert find("120 landmarks, host values") == 10
    extra = solve("first solve")
    assert find("120 landmarks, solver state", extra) == 10
    grow(200, {})
    assert find("200 landmarks, host values after growth") == 10
    grow(300, {W: 250})
    state["nq"] = 70
    assert find("300 landmarks, 70 queries, host values") == 250
    extra = solve("second solve")
    assert find("300 landmarks, solver state", extra) == 250
    g.set_plane(nodes[250], rej["landmarks"][W]["plane"])
    p = rej["pairs"][W]
    state["pairs"][250] = (p["gate"], None, 0.0)
    assert p["gate"] == "angle" and find("set_plane: the winner fails the angle gate") == 10
    g.landmark_set_merged(nodes[10])
    state["pairs"][10] = ("deleted", None, 0.0)
    assert find("landmark_set_merged") == 100
    g.remove_node(nodes[100])
    state["pairs"][100] = ("deleted", None, 0.0)
    live[100] = False
    assert find("remove_node of the landmark's plane") == -1
    g.set_plane(nodes[250], win["landmarks"][W]["plane"])
    lms[250] = win["landmarks"][W]
    p = win["pairs"][W]
    state["pairs"][250] = (p["gate"], p["total"], p["u_total"])
    assert find("set_plane back") == 250
    extra = solve("third solve")
    assert find("after the removal, solver state", extra) == 250


REPROJECT_SIZES = [1, 255, 256, 257, 1000]


@pytest.mark.parametrize("source", ["host_values", "solver_state"])
def test_reprojection_against_the_statement(built, fx, source):
    """the exact projection onto the stored 4-vector, rounded once to fp32: planes as the solver stores them (unit 4-vector, |n| < 1; |n| = 1e-3
    with |d| dominant; through the origin), points 1e3 away, on the plane already and the origin.  Ids of removed planes, of a pose and
    unknown ids pass through bit for bit (pps.h: a merged landmark is one whose node was removed).  k_map_build is tied to these bits by
    tests/test_gpu_map.py."""
    cases = fx["reproject"]
    g = P.Graph()
    node = {}
    for c in cases:
        key = tuple(c["plane"])
        if key not in node:
            node[key] = g.add_plane(c["plane"])
            g.add_plane_prior(node[key], c["plane"], STRONG)
    pose = g.add_pose([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])
    g.add_pose_prior(pose, [0.0] * 6, [1.0 if i in (0, 6, 11, 15, 18, 20) else 0.0 for i in range(21)])
    dead = g.add_plane([0.0, 0.6, 0.8, -2.0])
    g.add_plane_prior(dead, [0.0, 0.6, 0.8, -2.0], STRONG)
    g.remove_node(dead)
    K = H.K_of(fx, "reproject")
    if source == "solver_state":
        g.batch_optimize()
        est = g.get_planes(list(node.values()))
        assert np.max(np.abs(est - np.array(list(node.keys())))) < 1e-12
    through = [dead, pose, -1, g.num_nodes(), 1 << 30]
    worst = 0.0
    for n in REPROJECT_SIZES:
        ids = np.zeros(n, dtype=np.int32)
        pts = np.zeros((n, 3), dtype=np.float32)
        which = []
        for i in range(n):
            if i % 7 == 3:
                ids[i] = through[(i // 7) % len(through)]
                pts[i] = cases[i % len(cases)]["point"]
                which.append(None)
            else:
                c = cases[(i + n) % len(cases)]
                ids[i], pts[i] = node[tuple(c["plane"])], c["point"]
                which.append(c)
        out = g.reproject_points(ids, pts)
        for i, c in enumerate(which):
            if c is None:
                assert out[i].tobytes() == pts[i].tobytes(), (n, i, int(ids[i]))
                continue
            extra = 0.0
            if source == "solver_state":                                       # the estimate moved: the projection is 1 + |point| + |d| Lipschitz in it
                e = est[list(node.keys()).index(tuple(c["plane"]))]
                a = np.linalg.norm(np.array(c["plane"][:3]))
                extra = float(np.linalg.norm(e - c["plane"])) / a * (4 * np.linalg.norm(pts[i].astype(np.float64)) + 4 * abs(c["plane"][3]) / a + 1)
            err = np.maximum(np.abs(out[i].astype(np.float64) - c["out"]) - extra, 0.0)
            u = np.array(c["u_out"])
            assert np.all(err <= K * u), "%s (%s, %d points, index %d): %r against %r, unit %r" % (c["name"], source, n, i, out[i], c["out"], u)
            worst = max(worst, float(np.max(np.where(err == 0, 0.0, err / np.where(u > 0, u, 1e-300)))))
    WORST["reproject"] = max(WORST.get("reproject", 0.0), worst)


def test_report(built, fx):
    """the device's worst ratio per quantity, next to the CPU oracle's and the bound"""
    if not WORST:
        pytest.skip("nothing measured: the report collects what the other tests of this file saw")
    rows = ["%-12s %-12s %-12s %s" % ("quantity", "rho", "rho(oracle)", "K")]
    for k in sorted(WORST):
        rows.append("%-12s %-12.3g %-12.3g %g" % (k, WORST[k], fx["measured"][k]["rho_oracle"], fx["measured"][k]["K"]))
        assert WORST[k] <= fx["measured"][k]["K"]
    print("\ndevice against the 60-digit statement of association and re-projection, worst ratio per quantity\n" + "\n".join(rows))
