"""CPU: what the five queries on the factor -- pps_cov_block, pps_assoc_gate, pps_merge_gate, pps_loop_gate, pps_factor_gate -- and their
_last / _records companions answer when they refuse without a device: the return code AND the text of pps_last_error of every such refusal,
character for character, against tests/golden/query_contract.json.

The fixture was recorded with the library of the commit BEFORE the five calls were moved onto one host scaffold (csrc/pps_query.h), not with the
code under test: build that commit elsewhere and run `PPS_LIB=<its libpps.so> python tests/test_host_query_contract.py` to write it again.
The order of the cases is part of the contract (a handle is taken through removals and a cost function), so a new case goes at the end of
its section.  The texts of std::bad_alloc are not covered: nothing here can provoke them."""
import ctypes as C
import json
import os

import numpy as np

import pop_up_slam_amd as P
from pop_up_slam_amd import synth

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "query_contract.json")
IP, DP = C.POINTER(C.c_int), C.POINTER(C.c_double)
SENTINEL_FORM = 7      # pps_debug_cov_path_form(g, 7) is refused with a text of its own: what pps_last_error holds before every case


def _ints(v):
    return np.array(v, dtype=np.int32)


def _ip(a):
    return None if a is None else a.ctypes.data_as(IP)


def _dp(a):
    return None if a is None else a.ctypes.data_as(DP)


def run_cases():
    """[(name, return code, text)]: text is what the call left in pps_last_error, "" where it left what was there (or has no handle to ask)"""
    spec = synth.small_world(5, 3, seed=1)
    g = P.Graph(); nid, fid = spec.replay(g)
    L = g.L
    poses = [int(n) for n, t in zip(nid, spec.node_type) if t == synth.NODE_POSE]
    planes = [int(n) for n, t in zip(nid, spec.node_type) if t != synth.NODE_POSE]
    fids = [int(f) for f in fid]
    bad = len(spec.node_type) + 7
    L.pps_debug_cov_path_form(g.h, SENTINEL_FORM)
    sentinel = L.pps_last_error(g.h)
    assert sentinel
    out = []
    keep = []      # arrays the ctypes pointers of a case point into

    def case(name, fn, *args):
        assert name not in [o[0] for o in out], name
        L.pps_debug_cov_path_form(g.h, SENTINEL_FORM)
        rc = fn(*args)
        text = L.pps_last_error(g.h)
        out.append((name, int(rc), "" if (args and args[0] is None) or text == sentinel else text.decode()))

    def arr(v, dtype=np.int32):
        keep.append(np.ascontiguousarray(v, dtype=dtype))
        return keep[-1]

    # ---- pps_cov_block(g, nr, rows, nc, cols, out) ----
    cb_out = np.full(36 * 4, -7.0)
    rows = _ints(poses[:2]); cols = _ints([planes[0], poses[0]])

    def block(**k):
        return [k.get("h", g.h), k.get("nr", 2), k.get("rows", _ip(rows)), k.get("nc", 2), k.get("cols", _ip(cols)), k.get("out", _dp(cb_out))]

    for name, k in (("null handle", {"h": None}), ("null rows", {"rows": None}), ("null out", {"out": None}), ("negative nr", {"nr": -1}),
                    ("negative nc", {"nc": -1}), ("negative nc without cols", {"nc": -1, "cols": None}),
                    ("unknown row id", {"rows": _ip(arr([poses[0], bad]))}), ("negative row id", {"rows": _ip(arr([-1, poses[0]]))}),
                    ("unknown col id", {"cols": _ip(arr([planes[0], bad]))}),
                    ("row twice", {"nr": 3, "rows": _ip(arr([poses[0], poses[1], poses[0]]))}),
                    ("col twice", {"nc": 3, "cols": _ip(arr([planes[0], planes[1], planes[0]]))}),
                    ("joint twice", {"rows": _ip(arr([planes[1], planes[1]])), "cols": None}),
                    ("no recovery", {}), ("no recovery joint", {"cols": None}), ("no recovery nr 0", {"nr": 0}), ("no recovery nc 0", {"nc": 0})):
        case("cov_block: " + name, L.pps_cov_block, *block(**k))
    sec = C.c_double(-1.0); n = C.c_int(-1); cnt = C.c_int(-1); need = C.c_int64(-1)
    case("cov_block_last: null handle", L.pps_cov_block_last, None, C.byref(sec), C.byref(n))
    case("cov_block_last: before any call", L.pps_cov_block_last, g.h, C.byref(sec), C.byref(n))
    case("cov_block_last: null outputs", L.pps_cov_block_last, g.h, None, None)
    assert (sec.value, n.value) == (0.0, 0) and np.all(cb_out == -7.0)

    # ---- pps_assoc_gate(g, pose, n_meas, meas4, sqrtinf, n_planes, plane_ids, d2, best) ----
    m = np.array([[0.0, 0, 1, -1]]); w = synth._ut_diag([50.0] * 3)[None].copy()
    ag_d2 = np.full(8, -7.0); ag_best = np.full(2, -7, dtype=np.int32); ag_ids = _ints(planes[:2])
    m_nan = arr([[np.nan, 0, 1, 0]], np.float64); w_inf = arr([[np.inf] * 6], np.float64)
    many_m = np.tile(m, (65536, 1)); many_w = np.tile(w, (65536, 1))

    def assoc(**k):
        return [k.get("h", g.h), k.get("pose", poses[0]), k.get("nm", 1), k.get("m", _dp(m)), k.get("w", _dp(w)), k.get("np", 2), k.get("ids", _ip(ag_ids)),
                k.get("d2", _dp(ag_d2)), k.get("best", _ip(ag_best))]

    assoc_cases = (("null handle", {"h": None}), ("null meas", {"m": None}), ("null sqrtinf", {"w": None}), ("null d2", {"d2": None}),
                   ("negative n_meas", {"nm": -1}), ("negative n_planes", {"np": -1}), ("unknown pose", {"pose": bad}), ("negative pose", {"pose": -1}),
                   ("pose is a plane", {"pose": planes[0]}), ("too many measurements", {"nm": 65536, "m": _dp(many_m), "w": _dp(many_w)}),
                   ("unknown plane", {"np": 1, "ids": _ip(arr([bad]))}), ("negative plane", {"np": 1, "ids": _ip(arr([-1]))}),
                   ("plane is a pose", {"np": 1, "ids": _ip(arr([poses[1]]))}), ("plane twice", {"np": 3, "ids": _ip(arr([planes[0], planes[1], planes[0]]))}),
                   ("non-finite measurement", {"m": _dp(m_nan)}), ("non-finite sqrtinf", {"w": _dp(w_inf)}),
                   ("no measurement", {"nm": 0}), ("no plane", {"np": 0}), ("no recovery", {}), ("no recovery all planes", {"np": -5, "ids": None}),
                   ("no recovery without best", {"best": None}))
    for name, k in assoc_cases:
        case("assoc_gate: " + name, L.pps_assoc_gate, *assoc(**k))
    case("assoc_gate_last: null handle", L.pps_assoc_gate_last, None, C.byref(sec), C.byref(n))
    case("assoc_gate_last: before any call", L.pps_assoc_gate_last, g.h, C.byref(sec), C.byref(n))
    case("assoc_gate_last: null outputs", L.pps_assoc_gate_last, g.h, None, None)
    case("assoc_gate_records: null handle", L.pps_debug_assoc_gate_records, None, 0, None, C.byref(need))
    case("assoc_gate_records: null needed", L.pps_debug_assoc_gate_records, g.h, 0, None, None)
    case("assoc_gate_records: before any call", L.pps_debug_assoc_gate_records, g.h, 0, None, C.byref(need))
    assert (sec.value, n.value, need.value) == (0.0, 0, -1) and np.all(ag_d2 == -7.0) and np.all(ag_best == -7)

    # ---- pps_merge_gate(g, n, plane_ids, floor_var, threshold, d2, best, cap_pairs, pairs, n_pairs) ----
    mg_d2 = np.full(9, -7.0); mg_best = np.full(3, -7, dtype=np.int32); mg_pairs = np.full(6, -7, dtype=np.int32); mg_cnt = C.c_int(-7)
    mg_ids = _ints(planes[:2])

    def merge(**k):
        return [k.get("h", g.h), k.get("n", 2), k.get("ids", _ip(mg_ids)), C.c_double(k.get("fv", 0.0)), C.c_double(k.get("thr", 7.815)),
                k.get("d2", _dp(mg_d2)), k.get("best", _ip(mg_best)), k.get("cap", 3), k.get("pairs", _ip(mg_pairs)), k.get("cnt", C.byref(mg_cnt))]

    merge_cases = (("null handle", {"h": None}), ("negative n", {"n": -1}), ("negative cap", {"cap": -1}), ("negative floor", {"fv": -1e-9}),
                   ("nan floor", {"fv": np.nan}), ("inf floor", {"fv": np.inf}), ("nan threshold", {"thr": np.nan}), ("inf threshold", {"thr": np.inf}),
                   ("no output", {"d2": None, "best": None, "pairs": None, "cnt": None}), ("pairs without count", {"cnt": None}),
                   ("count without pairs", {"pairs": None}), ("unknown plane", {"ids": _ip(arr([planes[0], bad]))}),
                   ("negative plane", {"ids": _ip(arr([planes[0], -1]))}), ("plane is a pose", {"ids": _ip(arr([planes[0], poses[0]]))}),
                   ("plane twice", {"n": 3, "ids": _ip(arr([planes[0], planes[1], planes[0]]))}), ("one unknown plane", {"n": 1, "ids": _ip(arr([bad]))}),
                   ("no plane", {"n": 0}), ("one plane", {"n": 1}), ("no recovery", {}), ("no recovery all planes", {"n": -5, "ids": None}),
                   ("no recovery count alone", {"pairs": None, "cap": 0}), ("no recovery pairs alone", {"d2": None, "best": None}))
    for name, k in merge_cases:
        case("merge_gate: " + name, L.pps_merge_gate, *merge(**k))
    case("merge_gate_last: null handle", L.pps_merge_gate_last, None, C.byref(sec), C.byref(n), C.byref(cnt))
    case("merge_gate_last: before any call", L.pps_merge_gate_last, g.h, C.byref(sec), C.byref(n), C.byref(cnt))
    case("merge_gate_last: null outputs", L.pps_merge_gate_last, g.h, None, None, None)
    case("merge_gate_records: null handle", L.pps_debug_merge_gate_records, None, 0, None, C.byref(need))
    case("merge_gate_records: null needed", L.pps_debug_merge_gate_records, g.h, 0, None, None)
    case("merge_gate_records: before any call", L.pps_debug_merge_gate_records, g.h, 0, None, C.byref(need))
    assert (sec.value, n.value, cnt.value, need.value) == (0.0, 0, 0, -1)
    assert np.all(mg_d2 == -7.0) and np.all(mg_best == -7) and np.all(mg_pairs == -7) and mg_cnt.value == -7

    # ---- pps_loop_gate(g, n, pose_a, pose_b, meas6, sqrtinf, threshold, d2, S, cap_accepted, accepted, n_accepted) ----
    ia = _ints(poses[:2]); ib = _ints([poses[2], poses[0]])
    meas = np.zeros((2, 6)); sq = np.array([synth._ut_diag([4.0] * 3 + [20.0] * 3)] * 2)
    lg_d2 = np.full(2, -7.0); lg_S = np.full(72, -7.0); lg_acc = np.full(2, -7, dtype=np.int32); lg_cnt = C.c_int(-7)
    bad_meas = meas.copy(); bad_meas[1, 4] = np.nan
    bad_sq = sq.copy(); bad_sq[0, 20] = np.inf

    def loop(**k):
        return [k.get("h", g.h), k.get("n", 2), k.get("ia", _ip(ia)), k.get("ib", _ip(ib)), k.get("meas", _dp(meas)), k.get("sq", _dp(sq)),
                C.c_double(k.get("thr", 12.592)), k.get("d2", _dp(lg_d2)), k.get("S", _dp(lg_S)), k.get("cap", 2), k.get("acc", _ip(lg_acc)),
                k.get("cnt", C.byref(lg_cnt))]

    loop_cases = (("null handle", {"h": None}), ("null pose_a", {"ia": None}), ("null pose_b", {"ib": None}), ("null meas", {"meas": None}),
                  ("null sqrtinf", {"sq": None}), ("negative n", {"n": -1}), ("negative cap", {"cap": -1}),
                  ("no output", {"d2": None, "S": None, "acc": None, "cnt": None}), ("accepted without count", {"cnt": None}),
                  ("count without accepted", {"acc": None}), ("nan threshold", {"thr": np.nan}), ("inf threshold", {"thr": np.inf}),
                  ("non-finite measurement", {"meas": _dp(bad_meas)}), ("non-finite sqrtinf", {"sq": _dp(bad_sq)}),
                  ("unknown pose", {"ib": _ip(arr([poses[2], bad]))}), ("negative pose", {"ia": _ip(arr([-1, poses[1]]))}),
                  ("pose is a plane", {"ib": _ip(arr([poses[2], planes[0]]))}), ("pose with itself", {"ib": _ip(arr([poses[2], poses[1]]))}),
                  ("no candidate", {"n": 0}), ("no recovery", {}), ("no recovery count alone", {"acc": None, "cap": 0}),
                  ("no recovery accepted alone", {"d2": None, "S": None}), ("no recovery d2 alone", {"S": None, "acc": None, "cnt": None, "cap": 0}),
                  ("no recovery unread threshold", {"acc": None, "cnt": None, "cap": 0, "thr": np.nan}))
    for name, k in loop_cases:
        case("loop_gate: " + name, L.pps_loop_gate, *loop(**k))
    case("loop_gate_last: null handle", L.pps_loop_gate_last, None, C.byref(sec), C.byref(n), C.byref(cnt))
    case("loop_gate_last: before any call", L.pps_loop_gate_last, g.h, C.byref(sec), C.byref(n), C.byref(cnt))
    case("loop_gate_last: null outputs", L.pps_loop_gate_last, g.h, None, None, None)
    case("loop_gate_records: null handle", L.pps_debug_loop_gate_records, None, 0, None, C.byref(need))
    case("loop_gate_records: null needed", L.pps_debug_loop_gate_records, g.h, 0, None, None)
    case("loop_gate_records: before any call", L.pps_debug_loop_gate_records, g.h, 0, None, C.byref(need))
    assert (sec.value, n.value, cnt.value, need.value) == (0.0, 0, 0, -1)
    assert np.all(lg_d2 == -7.0) and np.all(lg_S == -7.0) and np.all(lg_acc == -7) and lg_cnt.value == -7

    # ---- pps_factor_gate(g, n, fids, thr3, thr6, d2, leverage, cap_flagged, flagged, n_flagged) ----
    fg_d2 = np.full(4, -7.0); fg_lev = np.full(4, -7.0); fg_flag = np.full(4, -7, dtype=np.int32); fg_cnt = C.c_int(-7)
    fg_ids = _ints(fids[:3])

    def factor(**k):
        return [k.get("h", g.h), k.get("n", 3), k.get("ids", _ip(fg_ids)), C.c_double(k.get("thr3", 7.815)), C.c_double(k.get("thr6", 12.592)),
                k.get("d2", _dp(fg_d2)), k.get("lev", _dp(fg_lev)), k.get("cap", 4), k.get("flagged", _ip(fg_flag)), k.get("cnt", C.byref(fg_cnt))]

    factor_cases = (("null handle", {"h": None}), ("negative n", {"n": -1}), ("negative cap", {"cap": -1}),
                    ("no output", {"d2": None, "lev": None, "flagged": None, "cnt": None}), ("flagged without count", {"cnt": None}),
                    ("count without flagged", {"flagged": None}), ("nan thr3", {"thr3": np.nan}), ("inf thr6", {"thr6": np.inf}),
                    ("unknown factor", {"n": 2, "ids": _ip(arr([fids[0], len(fids) + 7]))}), ("negative factor", {"n": 1, "ids": _ip(arr([-1]))}),
                    ("no factor", {"n": 0}), ("no recovery", {}), ("no recovery all factors", {"n": -5, "ids": None}),
                    ("no recovery count alone", {"flagged": None, "cap": 0}), ("no recovery flagged alone", {"d2": None, "lev": None}),
                    ("no recovery unread thresholds", {"flagged": None, "cnt": None, "cap": 0, "thr3": np.nan, "thr6": np.nan}))
    for name, k in factor_cases:
        case("factor_gate: " + name, L.pps_factor_gate, *factor(**k))
    case("factor_gate_last: null handle", L.pps_factor_gate_last, None, C.byref(sec), C.byref(n), C.byref(cnt))
    case("factor_gate_last: before any call", L.pps_factor_gate_last, g.h, C.byref(sec), C.byref(n), C.byref(cnt))
    case("factor_gate_last: null outputs", L.pps_factor_gate_last, g.h, None, None, None)
    case("factor_gate_records: null handle", L.pps_debug_factor_gate_records, None, 0, None, C.byref(need))
    case("factor_gate_records: null needed", L.pps_debug_factor_gate_records, g.h, 0, None, None)
    case("factor_gate_records: before any call", L.pps_debug_factor_gate_records, g.h, 0, None, C.byref(need))
    assert (sec.value, n.value, cnt.value, need.value) == (0.0, 0, 0, -1)
    assert np.all(fg_d2 == -7.0) and np.all(fg_lev == -7.0) and np.all(fg_flag == -7) and fg_cnt.value == -7

    # ---- a robust cost function: refused after the argument checks (and, in the loop gate, after the empty list) ----
    g.set_cost_function(P.COST_HUBER, 1.0)
    case("robust: cov_block", L.pps_cov_block, *block())
    case("robust: assoc_gate", L.pps_assoc_gate, *assoc())
    case("robust: assoc_gate argument first", L.pps_assoc_gate, *assoc(pose=bad))
    case("robust: assoc_gate no plane", L.pps_assoc_gate, *assoc(np=0))
    case("robust: merge_gate", L.pps_merge_gate, *merge())
    case("robust: loop_gate", L.pps_loop_gate, *loop())
    case("robust: loop_gate argument first", L.pps_loop_gate, *loop(n=-1))
    case("robust: loop_gate no candidate", L.pps_loop_gate, *loop(n=0))
    case("robust: factor_gate", L.pps_factor_gate, *factor())
    case("robust: factor_gate argument first", L.pps_factor_gate, *factor(n=-1))
    case("robust: factor_gate no factor", L.pps_factor_gate, *factor(n=0))
    g.set_cost_function(P.COST_NONE)

    # ---- removed ids are unknown ids ----
    g.remove_factor(fids[-1])
    case("removed: factor_gate", L.pps_factor_gate, *factor(n=2, ids=_ip(arr([fids[0], fids[-1]]))))
    g.remove_node(planes[-1])
    case("removed: cov_block", L.pps_cov_block, *block(cols=_ip(arr([planes[0], planes[-1]]))))
    case("removed: assoc_gate plane", L.pps_assoc_gate, *assoc(np=1, ids=_ip(arr([planes[-1]]))))
    case("removed: merge_gate", L.pps_merge_gate, *merge(ids=_ip(arr([planes[0], planes[-1]]))))
    g.remove_node(poses[-1])
    case("removed: assoc_gate pose", L.pps_assoc_gate, *assoc(pose=poses[-1]))
    case("removed: loop_gate", L.pps_loop_gate, *loop(ib=_ip(arr([poses[2], poses[-1]]))))
    g.close()
    return out


def test_every_refusal_without_a_device_answers_as_recorded(built):
    want = json.load(open(FIXTURE))["cases"]
    got = [[name, rc, text] for name, rc, text in run_cases()]
    assert [c[0] for c in got] == [c[0] for c in want]
    for g, w in zip(got, want):
        assert g == w
    # the fixture covers what it is meant to: all five calls, all three kinds of companion, and every code a refusal without a device can have
    names = " ".join(c[0] for c in want)
    for part in ("cov_block:", "assoc_gate:", "merge_gate:", "loop_gate:", "factor_gate:", "_last:", "_records:", "robust:", "removed:"):
        assert part in names
    assert {c[1] for c in want} == {P.PPS_OK, P.PPS_EINVAL, P.PPS_ESTATE}
    assert sum(1 for c in want if c[2]) > 80


if __name__ == "__main__":
    cases = run_cases()
    with open(FIXTURE, "w") as f:
        json.dump({"library": "the parent of the commit that added csrc/pps_query.h", "cases": [list(c) for c in cases]}, f, indent=0)
        f.write("\n")
    print(f"{len(cases)} cases -> {FIXTURE}")
