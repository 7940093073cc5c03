"""What tests/test_host_mp_assoc.py and tests/test_gpu_mp_assoc.py share: the arbitrary-precision fixture of plane association and
re-projection (tests/golden/mp_assoc_cases.json, written by oracle/mp_assoc.py), the fold that turns the per-pair statements into the
expected answer, a parameterised copy of the gates for the sensitivity table, and the composition of large tables.  No mpmath here."""
import math

import numpy as np

from oracle import mp_assoc as MA

REQUIRED_TAGS = ["gate_" + g for g in ("deleted", "class", "frame", "angle", "plane_dist", "dist2d_d2", "dist2d_d2c", "overlap_cov_on",
                                       "overlap_cov_no")] + \
    ["frame_equality", "angle_25", "angle_10", "plane_dist_1.5", "thre2d_x1.5", "tum_overlap_cannot_fail", "exact_dist2d_both",
     "exact_dist2d_d2", "exact_dist2d_d2c", "exact_cov_half", "degenerate_segment", "clamp_0", "clamp_1", "score_max", "tie", "ground_first",
     "ground_none", "wall_on_grounds", "all_deleted", "nan_first", "nan_later", "artefact"] + \
    ["term_" + t for t in ("angle_1e-7rad", "angle_1e-7rad_bare", "angle_near_threshold", "cov_cancelling", "dist2d_near_thre2d",
                           "plane_dist_near_4", "d_1e3", "pitch_plus", "pitch_minus")]


def load():
    return MA.load()


def K_of(fx, quantity):
    return fx["measured"][quantity]["K"]


def fold(fpi, pairs, tie_later=False, nan_unsticks=False, nan_displaces=False, ground_last=False):
    """Mapping.cpp:274-380 over (gate, total) per landmark in index order -> (index or -1, score); the flags are the fold's mutants"""
    n, best, err = 0, -1, -1.0
    for i, (gate, total) in enumerate(pairs):
        if gate != "pass":
            continue
        n += 1
        if fpi == 0:
            best = i
            if not ground_last:
                break
        elif n == 1 or total < err or (tie_later and total == err) or (nan_unsticks and err != err and total == total) or \
                (nan_displaces and total != total):
            best, err = i, total
    return best, err


# ---- the gates once more, from the fixture's exact per-pair quantities, with one switch per mutation ------------------------------------
MUTANTS = ["frame_ge", "dist2d_ge", "overlap_le", "swap_3_2", "no_10_rule", "no_1.5_halving", "no_thre2d_x1.5", "drop_d2", "drop_d2c",
           "endpoint_max", "score_min", "tie_later", "nan_unsticks", "nan_displaces", "ground_last"]
# the issue's "d2 <-> d2c roles swapped" has no observable effect: the gate is `d2 > t || d2c > t` and the score takes max(d2, d2c), both
# symmetric in the two.  It is kept in the table as the one mutant that must change nothing; dropping either side stands in for it.
EQUIVALENT_MUTANTS = ["swap_d2_d2c"]


def _endpoint_max(q, s):
    """d2 / d2c with max for min over the end-point distances (fp32 inputs, double arithmetic: only used far from any threshold)"""
    Q, S = np.array(q, dtype=np.float64).reshape(2, 2), np.array(s, dtype=np.float64).reshape(2, 2)
    d = np.linalg.norm(Q[:, None, :] - S[None, :, :], axis=2)
    return float(d.max(axis=1).sum() / 2), float(d.max(axis=0).sum() / 2)


def pair_verdict(q, L, p, fsi, prm, mut=None):
    """(gate, total) of one pair from the stored exact quantities (rounded to double; the twins sit 1e-9 and more from their thresholds,
    the equalities are floats).  mut: one of MUTANTS or None"""
    if L["deleted"]:
        return "deleted", None
    if (q["fpi"] == 0) != (L["fpi"] == 0):
        return "class", None
    if q["fpi"] == 0:
        return "pass", -1.0
    gap = fsi - L["seq"]
    if gap >= prm["assoc_near_frames"] if mut == "frame_ge" else gap > prm["assoc_near_frames"]:
        return "frame", None
    angle = float("nan") if p.get("artefact") else p["angle"]
    if angle > prm["edge_asso_angle"]:
        return "angle", None
    a3, a2 = (2, 3) if mut == "swap_3_2" else (3, 2)
    thre2d, thre_cov = prm["edge_asso_2ddist"], prm["edge_asso_proj"]
    if angle < 25.0:
        thre_cov = prm["edge_asso_proj"] / a3
        if mut != "no_thre2d_x1.5":
            thre2d = prm["edge_asso_2ddist"] * 1.5
        if angle <= 10.0 and mut != "no_10_rule":
            thre_cov = prm["edge_asso_proj"] / a2
    pd = p["plane_dist"]
    if pd > prm["edge_asso_planedist"]:
        return "plane_dist", None
    if pd < 1.5 and mut != "no_1.5_halving":
        thre_cov = thre_cov / 2
    d2, d2c = p["d2"], p["d2c"]
    if mut == "endpoint_max":
        d2, d2c = _endpoint_max(q["seg2d"], L["seg2d"])
    if mut == "swap_d2_d2c":
        d2, d2c = d2c, d2
    over = (lambda x: x >= thre2d) if mut == "dist2d_ge" else (lambda x: x > thre2d)
    if (mut != "drop_d2" and over(d2)) or (mut != "drop_d2c" and over(d2c)):
        return "dist2d", None
    if p.get("nan_segment"):
        return "pass", float("nan")
    on, no = p["cov_on"], p["cov_no"]
    under = (lambda x: x <= thre_cov) if mut == "overlap_le" else (lambda x: x < thre_cov)
    if under(on) or under(no):
        return "overlap", None
    dm = min(d2, d2c) if mut == "score_min" else max(d2, d2c)
    return "pass", angle / prm["edge_asso_angle"] * 3 + (1 - on) + (1 - no) + dm / thre2d + pd / 4


def atom_answer(fx, a, mut=None):
    prm = MA.atom_params(fx, a)
    pairs = [pair_verdict(a["query"], L, p, a["frame_seq_id"], prm, mut) for L, p in zip(a["landmarks"], a["pairs"])]
    flags = {m: mut == m for m in ("tie_later", "nan_unsticks", "nan_displaces", "ground_last")}
    return fold(a["query"]["fpi"], pairs, **flags), pairs


def stored_answer(a):
    return fold(a["query"]["fpi"], [(p["gate"], p.get("total", -1.0 if a["query"]["fpi"] == 0 else None)) for p in a["pairs"]])


def same_score(got, want, u, K):
    if want != want:
        return got != got
    return got == got and abs(got - want) <= K * u


def score_ratio(got, want, u):
    if want != want or u == 0:
        return 0.0 if (got != got) == (want != want) and (want != want or got == want) else math.inf
    return abs(got - want) / u


# ---- large tables out of atoms ------------------------------------------------------------------------------------------------------------
def filler(a, k):
    """a landmark every query of atom `a` rejects decidedly whatever its planes are: the wrong class for the query (the class gate is
    integer work), with planes and segments that vary with k so that a kernel reading the wrong record would show"""
    fpi = 0 if a["query"]["fpi"] != 0 else 1 + k % 4
    pl = np.array([math.cos(0.1 * k), math.sin(0.1 * k), 0.3, -1.0 - 0.01 * k])
    pl /= np.linalg.norm(pl)
    return dict(plane=[float(x) for x in pl], fpi=fpi, seq=a["frame_seq_id"] - 1, deleted=0,
                seg2d=[float(np.float32(x)) for x in (100 + k, 200, 400 + k, 200)], seg3d=[float(np.float32(x)) for x in (0.1 * k, 0, 4, 0)])


def compose(a, n, places):
    """a table of n landmarks: the atom's landmark j at index places[j] (a dict j -> index, or j -> list of indices for bit-identical
    copies), fillers elsewhere -> (landmarks, per-index (gate, total, u_total))"""
    lms = [filler(a, k) for k in range(n)]
    pairs = [("class", None, 0.0)] * n
    for j, where in places.items():
        for i in ([where] if isinstance(where, int) else where):
            lms[i] = a["landmarks"][j]
            p = a["pairs"][j]
            pairs[i] = (p["gate"], p.get("total", -1.0 if a["query"]["fpi"] == 0 else None), p.get("u_total", 0.0))
    return lms, pairs


def expected(a, pairs):
    best, err = fold(a["query"]["fpi"], [(g, t) for g, t, _ in pairs])
    return best, err, (pairs[best][2] if best >= 0 else 0.0)


# ---- the planes of a solved graph against the fixture's ---------------------------------------------------------------------------------------
def shift_bounds(pose, want, got):
    """how far angle (degrees) and plane distance of any pair with this landmark may move when its stored 4-vector moves from `want` to
    `got`.  With delta = |got - want| and a = |abc|: the unit normal moves by at most 2 delta / a and the angle between unit vectors is
    1-Lipschitz in the geodesic sense, pi / 2 in the chord: <= pi delta / a rad.  The plane in the sensor frame is T^T pi normalised, a
    rotation of abc and d' = -(t . abc + p3) / a, so point0 = d' n' moves by at most 2 |d'| delta / a + (|t| + 1 + |d'|) delta / a, and
    the plane distance, a projection of point0, by no more."""
    want, got = np.asarray(want, float), np.asarray(got, float)
    delta = float(np.linalg.norm(got - want))
    a = float(np.linalg.norm(want[:3]))
    t = np.asarray(pose[:3], float)
    dl = abs(float(t @ want[:3] + want[3])) / a
    return math.degrees(math.pi * delta / a), (3 * dl + float(np.linalg.norm(t)) + 1) * delta / a
