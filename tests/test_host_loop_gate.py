"""CPU: the algorithm of pps_loop_gate (csrc/pps_loop.hip, csrc/pps_loop.cpp) before any kernel runs on a device.

d2 = r' S^-1 r of a candidate odometry factor between two existing poses, S = I + Jw Sigma_(a,b) Jw', without forming Sigma:
(a) the kernel source itself compiled for the host (tests/cpp/loop_emu.cpp: k_cov_path, then k_loop_gate) on the panels of a dense Cholesky
factor of a random positive definite H of the graph's sparsity (the construction of tests/test_host_merge_gate.py), for corridor_60_14 and
loop_graph(60, 40), in both Jacobian modes, against the dense formula with Sigma = the dense inverse.  e = the largest relative error, of d2
over the candidates and of the entries of S relative to max |S|; d = the same distance between the two CPU inverses of
cov_helpers.cpu_inverses; bound e <= max(16 d, 1e-12), factor and floor of tests/test_gpu_cov.py.  Jw and r of the kernel are compared with
K1's thread form on the host (csrc/pps_lin.h).
(b) the C-ABI surface without a device: symbols, argument checks, the answers that need no recovery."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pop_up_slam_amd as P
from cov_block_helpers import elimination_positions, request_tables, root_lengths
from cov_helpers import cpu_inverses, node_layout
from linsolve_helpers import loop_graph
from loop_gate_helpers import CAND, CHI2_6_095, WAVES, choose_pairs, errors, joint_sigma, make_candidates, pose_paths, reference, tree_case
from pop_up_slam_amd import synth
from test_host_cov_block import _random_h, _spec_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAPHS = {"corridor_60_14": (lambda: synth.corridor(60, 14, seed=7), 5), "loops_60p_40l": (lambda: loop_graph(60, 40), 6)}


@pytest.fixture(scope="module")
def emu(built, tmp_path_factory):
    so = tmp_path_factory.mktemp("loop_emu") / "libloopemu.so"
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-Wno-attributes", "-Wno-unknown-pragmas",
                           "-I", os.path.join(ROOT, "tests", "cpp", "block_emu"), "-I", os.path.join(ROOT, "pop_up_slam_amd", "csrc"), "-x", "c++",
                           os.path.join(ROOT, "tests", "cpp", "loop_emu.cpp"), "-o", str(so)])
    return C.CDLL(str(so))


_SCENES = {}


def _scene(name):
    """the analysis, a random H of the graph's sparsity with its two CPU inverses, the factor panels in the device layout, the pose states (the
    graph's initial values), the candidates"""
    if name in _SCENES:
        return _SCENES[name]
    make, seed = GRAPHS[name]
    spec = make()
    g, dims, f_nodes, f_dim = _spec_graph(spec)
    g.analyze()
    A = g.analysis_dump()
    g.close()
    lay = node_layout(A, dims)
    H = _random_h(A, lay, f_nodes, f_dim, seed)
    S1, S2 = cpu_inverses(H)
    pidx, epos = elimination_positions(A)
    Lg = np.linalg.cholesky(H[np.ix_(pidx, pidx)])
    L = np.full(A["L_size"], np.nan)
    for s in range(A["n_fronts"]):
        p, b, po = int(A["f_p"][s]), int(A["f_b"][s]), int(A["f_poff"][s])
        piv = np.arange(po, po + p); bnd = epos[A["bidx"][A["f_bidx_off"][s]:A["f_bidx_off"][s + 1]]]
        pan = np.vstack([Lg[np.ix_(piv, piv)], Lg[np.ix_(bnd, piv)], np.full((1, p), np.nan)])
        pan[:p][np.triu_indices(p, 1)] = np.nan
        L[A["f_Loff"][s]:A["f_Loff"][s] + (p + b + 1) * p] = pan.ravel()
    poses = [n for n in sorted(lay) if lay[n][1] == 6]
    path = pose_paths(A, lay, poses)
    pairs, present = choose_pairs(poses, path)
    pose_of = {n: spec.node_init[n, :7] for n in poses}
    meas, sq = make_candidates(pose_of, pairs, seed=seed + 40)
    sc = dict(A=A, lay=lay, S=(S1, S2), L=L, poses=poses, path=path, pairs=pairs, present=present, pose_of=pose_of, meas=meas, sq=sq,
              span=lambda n: slice(lay[n][0], lay[n][0] + lay[n][1]))
    _SCENES[name] = sc
    return sc


def _run(emu, sc, sel, mode, threshold=CHI2_6_095, sq=None, meas=None, want_S=True):
    """the two kernels on the candidates `sel` (indices into sc['pairs'])"""
    A, lay, poses = sc["A"], sc["lay"], sc["poses"]
    pairs = [sc["pairs"][k] for k in sel]
    sq = sc["sq"] if sq is None else sq
    meas = sc["meas"] if meas is None else meas
    distinct = list(dict.fromkeys(n for p in pairs for n in p))
    walks, steps, _, K, n_strip, _ = request_tables(A, lay, distinct)
    where = {n: w for w, n in enumerate(distinct)}
    cand = np.zeros(len(pairs), dtype=CAND)
    for k, (a, b) in enumerate(pairs):
        cand[k] = (walks[where[a]]["strip"], walks[where[b]]["strip"], poses.index(a), poses.index(b), sc["path"][a][0], sc["path"][b][0], meas[sel[k]],
                   sq[sel[k]])
    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)
    tabs = [i32(A["f_p"]), i32(A["f_b"]), np.ascontiguousarray(A["f_Loff"], dtype=np.int64), i32(A["f_cmap_off"]), i32(A["cmap"]), sc["L"]]
    parent, rl = i32(A["f_parent"]), i32(root_lengths(A))
    max_p = int(max(A["f_p"])); max_front = int(max(np.asarray(A["f_p"]) + np.asarray(A["f_b"])))
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    pose_ld = len(poses) + 3
    pose_est = np.full((7, pose_ld), np.nan); pose_est[:, :len(poses)] = np.array([sc["pose_of"][n] for n in poses]).T
    n = len(pairs)
    Y = np.full(n_strip, np.nan); status = np.zeros(1)
    flag = np.full(n, 9, dtype=np.uint8); d2 = np.full(n, -7.0); S = np.full((n, 6, 6), -7.0) if want_S else None; rec = np.full((n, 78), np.nan)
    rc = emu.emu_loop(int(A["n_fronts"]), *[ptr(t) for t in tabs], ptr(walks), len(walks), ptr(steps), len(steps), K, max_p, max_front, ptr(Y),
                      C.c_longlong(n_strip), len(poses), pose_ld, ptr(pose_est), ptr(cand), n, ptr(parent), ptr(rl), C.c_double(threshold), mode,
                      ptr(status), ptr(flag), ptr(d2), ptr(S), ptr(rec))
    assert rc == 0 and status[0] == 0.0
    return d2, S, flag, rec[:, :72].reshape(n, 6, 12), rec[:, 72:]


def _ref(sc, sel, Jw, r, which):
    Sig = np.array([joint_sigma(sc["S"][which], sc["span"](a), sc["span"](b)) for a, b in (sc["pairs"][k] for k in sel)])
    return reference(Jw, r, Sig)


@pytest.mark.parametrize("name", list(GRAPHS))
def test_candidates_cover_the_tree_cases(built, name):
    sc = _scene(name)
    pairs, path = sc["pairs"], sc["path"]
    cases = {tree_case(path[a], path[b]) for a, b in pairs}
    assert cases == {"same", "nested", "apart"}, (name, cases, sc["present"])
    assert max(sum(n in p for p in pairs) for n in sc["poses"]) >= 3 and len(set(pairs)) < len(pairs) and len(pairs) % WAVES != 0
    assert any(a > b for a, b in pairs) and any(a < b for a, b in pairs)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_kernel_source_emulated_on_the_host(emu, name, mode):
    sc = _scene(name)
    n = len(sc["pairs"]); sel = list(range(n))
    d2, S, flag, Jw, r = _run(emu, sc, sel, mode)
    # the records: K1's thread form on the host (pose_exmap instead of the step quaternions: the same bits, pps_geom.h)
    out = np.zeros(78); dp = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.c_void_p)
    for k, (a, b) in enumerate(sc["pairs"]):
        emu.emu_lin_odometry(mode, dp(sc["pose_of"][a]), dp(sc["pose_of"][b]), dp(sc["meas"][k]), dp(sc["sq"][k]), dp(out))
        assert np.array_equal(Jw[k][:, :6], out[:36].reshape(6, 6)) and np.array_equal(Jw[k][:, 6:], out[36:72].reshape(6, 6)), (name, mode, k)
        assert np.array_equal(r[k], out[72:]), (name, mode, k)
    (ref, refS, cond), (ref2, ref2S, _) = _ref(sc, sel, Jw, r, 0), _ref(sc, sel, Jw, r, 1)
    assert cond < 1e8, cond                                    # asserted on the reference alone
    assert np.all(np.isfinite(d2)) and np.all(np.isfinite(S)) and np.array_equal(S, np.transpose(S, (0, 2, 1)))
    e, d = errors(d2, S, ref, refS), errors(ref2, ref2S, ref, refS)
    print(f"LOOP host-emulated kernels {name} mode {mode}: candidates {n} e {e:.3e} d {d:.3e} bound {max(16 * d, 1e-12):.3e} cond {cond:.2e} "
          f"d2 {ref.min():.3g} .. {ref.max():.3g}")
    assert e <= max(16 * d, 1e-12), (e, d)
    # decisions.  Sigma of a random H is no pose uncertainty, so 12.592 decides nothing here (the GPU tests have real graphs for that): the
    # threshold is put between the two middle d2 of the REFERENCE, which must be 2 % apart, and the kernels run once more with it
    lo, hi = np.sort(ref)[n // 2 - 1:n // 2 + 1]
    thr = float(np.sqrt(lo * hi))
    assert np.all(np.abs(ref - thr) > 0.01 * thr), (lo, hi)
    d2t, St, flag, _, _ = _run(emu, sc, sel, mode, threshold=thr)
    assert np.array_equal(d2t, d2) and np.array_equal(St, S)
    assert list(flag) == [1 if v < thr else 0 for v in ref] and int(flag.sum()) == n // 2
    dup = [k for k in range(n) if sc["pairs"][k] == sc["pairs"][0]]
    assert len(dup) == 2                                       # the pair listed twice: its own measurement each time, so only S is shared ...
    sq_same, meas_same = sc["sq"].copy(), sc["meas"].copy()
    sq_same[dup[1]] = sq_same[dup[0]]; meas_same[dup[1]] = meas_same[dup[0]]
    d2d, Sd, _, _, _ = _run(emu, sc, sel, mode, sq=sq_same, meas=meas_same)      # ... and with the same measurement and weights every bit
    assert d2d[dup[0]] == d2d[dup[1]] and np.array_equal(Sd[dup[0]], Sd[dup[1]])
    # independence: every candidate alone, the list reversed, a sub-list -- the same bits (other poses change K and the strips' places)
    for k in sel:
        d2k, Sk, _, _, _ = _run(emu, sc, [k], mode)
        assert d2k[0] == d2[k] and np.array_equal(Sk[0], S[k]), k
    for sub in (sel[::-1], sel[1::3]):
        d2s, Ss, fs, _, _ = _run(emu, sc, sub, mode, threshold=thr)
        assert np.array_equal(d2s, d2[sub]) and np.array_equal(Ss, S[sub]) and np.array_equal(fs, flag[sub])
    d2n, none, fn, _, _ = _run(emu, sc, sel, mode, threshold=thr, want_S=False)                # without S: the same d2 and flags
    assert none is None and np.array_equal(d2n, d2) and np.array_equal(fn, flag)


def test_a_candidate_without_a_positive_definite_s_is_nan_and_alone(emu):
    """sqrt information 1e200: Jw Sigma Jw' overflows, the first pivot is not finite.  That candidate is NaN with flag 2; every other entry
    keeps its bits."""
    sc = _scene("corridor_60_14")
    n = len(sc["pairs"]); sel = list(range(n))
    d2, S, flag, _, _ = _run(emu, sc, sel, 0)
    sq = sc["sq"].copy(); sq[2] = synth._ut_diag([1e200] * 6)
    d2b, Sb, flagb, _, rb = _run(emu, sc, sel, 0, sq=sq)
    assert np.isnan(d2b[2]) and flagb[2] == 2 and list(flagb).count(2) == 1 and np.all(np.isfinite(rb[2]))
    keep = [k for k in sel if k != 2]
    assert np.array_equal(d2b[keep], d2[keep]) and np.array_equal(Sb[keep], S[keep]) and np.array_equal(flagb[keep], flag[keep])
    assert not np.all(np.isfinite(Sb[2]))


def test_symbols_are_declared_exported_and_bound(built):
    hdr = open(os.path.join(ROOT, "include", "pps.h")).read()
    lib = C.CDLL(P.LIB_PATH)
    for name in ("pps_loop_gate", "pps_loop_gate_last", "pps_debug_loop_gate_records"):
        assert re.search(r"\b" + name + r"\s*\(", hdr) and name in P.SYMBOLS and getattr(lib, name) is not None
    assert P.lib().pps_version() == 305                    # detected by symbol lookup, not by a version bump


def test_arguments_and_state_without_a_device(built):
    spec = synth.small_world(5, 3, seed=1)
    g = P.Graph(); nid, _ = spec.replay(g)
    poses = [int(n) for n, t in zip(nid, spec.node_type) if t == synth.NODE_POSE]
    planes = [int(n) for n, t in zip(nid, spec.node_type) if t != synth.NODE_POSE]
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    ia = np.array(poses[:2], dtype=np.int32); ib = np.array([poses[2], poses[0]], dtype=np.int32)
    meas = np.zeros((2, 6)); sq = np.array([synth._ut_diag([4.0] * 3 + [20.0] * 3)] * 2)
    d2 = np.full(2, -7.0); S = np.full(72, -7.0); acc = np.full(2, -7, dtype=np.int32); cnt = C.c_int(-7)
    args = lambda **k: [k.get("h", g.h), k.get("n", 2), k.get("ia", ia.ctypes.data_as(ip)), k.get("ib", ib.ctypes.data_as(ip)),
                        k.get("meas", meas.ctypes.data_as(dp)), k.get("sq", sq.ctypes.data_as(dp)), C.c_double(k.get("thr", CHI2_6_095)),
                        k.get("d2", d2.ctypes.data_as(dp)), k.get("S", S.ctypes.data_as(dp)), k.get("cap", 2), k.get("acc", acc.ctypes.data_as(ip)),
                        k.get("cnt", C.byref(cnt))]
    untouched = lambda: np.all(d2 == -7.0) and np.all(S == -7.0) and np.all(acc == -7) and cnt.value == -7
    arr = lambda v: np.array(v, dtype=np.int32).ctypes.data_as(ip)
    bad_meas = meas.copy(); bad_meas[1, 4] = np.nan
    bad_sq = sq.copy(); bad_sq[0, 20] = np.inf
    removed = poses[-1]; g.remove_node(removed)
    for k in ({"h": None}, {"ia": None}, {"ib": None}, {"meas": None}, {"sq": None}, {"n": -1}, {"cap": -1},
              {"d2": None, "S": None, "acc": None, "cnt": None}, {"cnt": None}, {"acc": None}, {"thr": np.nan}, {"thr": np.inf},
              {"meas": bad_meas.ctypes.data_as(dp)}, {"sq": bad_sq.ctypes.data_as(dp)},
              {"ib": arr([poses[2], len(spec.node_type) + 7])}, {"ia": arr([-1, poses[1]])}, {"ib": arr([poses[2], removed])},
              {"ib": arr([poses[2], planes[0]])}, {"ib": arr([poses[2], poses[1]])}):                       # the last: pose_a[1] == pose_b[1]
        assert g.L.pps_loop_gate(*args(**k)) == P.PPS_EINVAL, k
    assert untouched()
    # what is no PPS_EINVAL: the count alone, one output of the three, a threshold nobody reads -- each goes on to ask for the recovery
    for k in ({"acc": None, "cap": 0}, {"d2": None, "S": None}, {"S": None, "acc": None, "cnt": None, "cap": 0},
              {"acc": None, "cnt": None, "cap": 0, "thr": np.nan}, {"d2": None, "acc": None, "cnt": None, "cap": 0}):
        assert g.L.pps_loop_gate(*args(**k)) == P.PPS_ESTATE, k
        assert "no valid covariance recovery" in g.L.pps_last_error(g.h).decode()
    with pytest.raises(P.PpsError) as e:
        g.loop_gate(ia, ib, meas, sq)
    assert e.value.code == P.PPS_ESTATE and "no valid covariance recovery" in str(e.value)
    # n == 0: PPS_OK before the recovery is looked at, outputs untouched
    assert g.L.pps_loop_gate(*args(n=0)) == P.PPS_OK and untouched()
    e2, eS, ea = g.loop_gate([], [], np.zeros((0, 6)), np.zeros((0, 21)), want_S=True)
    assert len(e2) == 0 and eS.shape == (0, 6, 6) and len(ea) == 0
    # a cost function: refused after the argument checks and after n == 0, without a device, naming the cost function
    g.set_cost_function(P.COST_HUBER, 1.0)
    assert g.L.pps_loop_gate(*args(n=-1)) == P.PPS_EINVAL and g.L.pps_loop_gate(*args(n=0)) == P.PPS_OK
    assert g.L.pps_loop_gate(*args()) == P.PPS_ESTATE and "cost function" in g.L.pps_last_error(g.h).decode() and untouched()
    with pytest.raises(P.PpsError) as e:
        g.loop_gate(ia, ib, meas, sq)
    assert e.value.code == P.PPS_ESTATE and "pps_set_cost_function" in str(e.value)
    g.set_cost_function(P.COST_NONE)
    assert g.L.pps_loop_gate(*args()) == P.PPS_ESTATE and "no valid covariance recovery" in g.L.pps_last_error(g.h).decode()
    # the _last call and the records before any successful call
    sec = C.c_double(-1.0); n = C.c_int(-1); npd = C.c_int(-1)
    assert g.L.pps_loop_gate_last(g.h, C.byref(sec), C.byref(n), C.byref(npd)) == P.PPS_OK and (sec.value, n.value, npd.value) == (0.0, 0, 0)
    assert g.L.pps_loop_gate_last(g.h, None, None, None) == P.PPS_OK and g.L.pps_loop_gate_last(None, None, None, None) == P.PPS_EINVAL
    need = C.c_int64(-1)
    assert g.L.pps_debug_loop_gate_records(g.h, 0, None, C.byref(need)) == P.PPS_ESTATE      # no loop gate has run on this handle
    assert g.L.pps_debug_loop_gate_records(g.h, 0, None, None) == P.PPS_EINVAL
    with pytest.raises(ValueError):
        g.loop_gate(ia, ib[:1], meas, sq)
    assert g.num_nodes() == len(spec.node_type) - 1                                           # the handle stays usable
    g.close()
