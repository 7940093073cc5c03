"""CPU: the algorithm of pps_assoc_gate (csrc/pps_gate.hip, csrc/pps_gate.cpp) before any kernel runs on a device.

d2 = r' (I + Jw Sigma Jw')^-1 r without forming Sigma: with the strips Y_x, Y_l of the root-path walks (tests/cov_block_helpers.py) and
Z_x = Y_x Jp', Z_l = Y_l Jl', S = I + Z_x'Z_x + Z_l'Z_l + (Z_x'Z_l + Z_l'Z_x over the COMMON suffix of the two paths).  (a) a numpy
restatement driven only by pps_analysis_dump, (b) the kernel source itself compiled for the host (tests/cpp/gate_emu.cpp), both against
the dense formula with Sigma = the dense inverse of a random positive definite H of the graph's sparsity (the construction of
tests/test_host_cov_block.py).  Measure: e = the largest relative error of d2 (of the entries of S in (a)) over all candidates, d = the same
distance between the two CPU inverses of cov_helpers.cpu_inverses; bound e <= max(16 d, 1e-12).  (c) the C-ABI surface without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pop_up_slam_amd as P
from cov_block_helpers import common_suffix, elimination_positions, node_front, path_to_root, request_tables, root_lengths, walk
from cov_helpers import cpu_inverses
from pop_up_slam_amd import synth
from test_host_cov_block import CASES, _setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAND = np.dtype([("strip", "<i8"), ("slot", "<i4"), ("rootlen", "<i4"), ("common", "<i4"), ("pad", "<i4")])


def _pose_and_planes(A, lay):
    """the last pose whose path to the root DIVERGES from some plane's below the root (common suffix shorter than both paths), all planes,
    and the planes it diverges from"""
    _, epos = elimination_positions(A)
    poses = [n for n in sorted(lay) if lay[n][1] == 6]; planes = [n for n in sorted(lay) if lay[n][1] == 3]
    path = {n: path_to_root(A, node_front(A, epos, lay[n][0])[0]) for n in poses + planes}
    plen = lambda n: sum(int(A["f_p"][s]) for s in path[n])
    for x in reversed(poses):
        div = [l for l in planes if 0 < common_suffix(A, path[x], path[l]) < min(plen(x), plen(l))]
        if div:
            return x, planes, div, path
    return poses[-1], planes, [], path


def _sigma9(S, span, x, l):
    ix = np.r_[np.arange(span(x).start, span(x).stop), np.arange(span(l).start, span(l).stop)]
    return S[np.ix_(ix, ix)]


@pytest.mark.parametrize("case", ["corridor_60_14", "corridor_150_32"])
def test_strip_algebra_reproduces_the_dense_innovation_covariance(built, case):
    A, lay, H, S1, S2, span = _setup(case, seed=13)
    x, planes, div, path = _pose_and_planes(A, lay)
    assert div, "no pose of this graph has a path that leaves a plane's below the root"
    pidx, epos = elimination_positions(A)
    Lg = np.linalg.cholesky(H[np.ix_(pidx, pidx)])
    rng = np.random.default_rng(4)
    _, Yx = walk(A, Lg, epos, lay[x][0], 6)
    e = d = 0.0
    wrong = 0.0
    for l in planes:
        _, Yl = walk(A, Lg, epos, lay[l][0], 3)
        n = common_suffix(A, path[x], path[l])
        Jw = rng.normal(size=(3, 9)); r = rng.normal(size=3)
        K = max(len(Yx), len(Yl))
        Zx = np.vstack([np.zeros((K - len(Yx), 3)), Yx @ Jw[:, :6].T]); Zl = np.vstack([np.zeros((K - len(Yl), 3)), Yl @ Jw[:, 6:].T])
        S = np.eye(3) + Zx.T @ Zx + Zl.T @ Zl + Zx[K - n:].T @ Zl[K - n:] + Zl[K - n:].T @ Zx[K - n:]
        ref, ref2 = (np.eye(3) + Jw @ _sigma9(Sx, span, x, l) @ Jw.T for Sx in (S1, S2))
        d2, d2r, d2r2 = (r @ np.linalg.solve(M, r) for M in (S, ref, ref2))
        e = max(e, abs(d2 - d2r) / d2r); d = max(d, abs(d2r2 - d2r) / d2r)
        if l in div:                                   # the trap: strips added row by row before the product count cross terms of fronts the paths do not share
            Sw = np.eye(3) + (Zx + Zl).T @ (Zx + Zl)
            wrong = max(wrong, np.linalg.norm(Sw - ref) / np.linalg.norm(ref))
    print(f"GATE numpy {case}: pose {x} planes {len(planes)} diverging {len(div)} e {e:.3e} d {d:.3e} bound {max(16 * d, 1e-12):.3e} row-wise sum off by {wrong:.1e}")
    assert e <= max(16 * d, 1e-12), (case, e, d)
    assert wrong > 1e-6                               # (the diverging pairs do tell the two forms apart)


@pytest.mark.parametrize("mode", [0, 1])
def test_kernel_source_emulated_on_the_host(built, tmp_path, mode):
    so = tmp_path / "libgateemu.so"
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-Wno-attributes", "-Wno-unknown-pragmas",
                           "-I", os.path.join(ROOT, "tests", "cpp", "block_emu"), "-I", os.path.join(ROOT, "pop_up_slam_amd", "csrc"), "-x", "c++",
                           os.path.join(ROOT, "tests", "cpp", "gate_emu.cpp"), "-o", str(so)])
    lib = C.CDLL(str(so))
    A, lay, H, S1, S2, span = _setup("corridor_60_14", seed=5)
    x, planes, div, path = _pose_and_planes(A, lay)
    assert div
    planes = planes[::2] + [l for l in div[:2] if l not in planes[::2]]          # 7 .. 9 candidates: more than one workgroup, the last one partly empty
    pidx, epos = elimination_positions(A)
    Lg = np.linalg.cholesky(H[np.ix_(pidx, pidx)])
    L = np.full(A["L_size"], np.nan)
    for s in range(A["n_fronts"]):
        p, b, po = int(A["f_p"][s]), int(A["f_b"][s]), int(A["f_poff"][s])
        piv = np.arange(po, po + p); bnd = epos[A["bidx"][A["f_bidx_off"][s]:A["f_bidx_off"][s + 1]]]
        pan = np.vstack([Lg[np.ix_(piv, piv)], Lg[np.ix_(bnd, piv)], np.full((1, p), np.nan)])
        pan[:p][np.triu_indices(p, 1)] = np.nan
        L[A["f_Loff"][s]:A["f_Loff"][s] + (p + b + 1) * p] = pan.ravel()
    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)
    tabs = [i32(A["f_p"]), i32(A["f_b"]), np.ascontiguousarray(A["f_Loff"], dtype=np.int64), i32(A["f_cmap_off"]), i32(A["cmap"]), L]
    max_p = int(max(A["f_p"])); max_front = int(max(np.asarray(A["f_p"]) + np.asarray(A["f_b"])))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rl = root_lengths(A)
    # node states: one pose, the candidate planes; measurements near the prediction of some candidate and far from it
    rng = np.random.default_rng(9)
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    pose = np.concatenate([rng.normal(size=3), q])
    pl = rng.normal(size=(len(planes), 4)); pl /= np.linalg.norm(pl, axis=1)[:, None]
    pose_ld, plane_ld = 4, len(planes) + 3
    pose_est = np.full((7, pose_ld), np.nan); pose_est[:, 2] = pose
    plane_est = np.full((4, plane_ld), np.nan); plane_est[:, :len(planes)] = pl.T
    M = 3
    meas = np.zeros((M, 10))
    for i in range(M):
        meas[i, :4] = synth.plane_exmap(synth.plane_transform_to(pl[i], pose), 0.02 * (i + 1) * rng.normal(size=3))
        meas[i, 4:] = synth._ut_diag([30.0, 40.0, 50.0]) + np.array([0, 3.0, -2.0, 0, 1.0, 0])

    def run(cols, rows_m):
        walks, steps, _, K, n_strip, _ = request_tables(A, lay, [x], cols)
        cands = np.zeros(len(cols), dtype=CAND)
        for k, l in enumerate(cols):
            cands[k] = (walks[1 + k]["strip"], planes.index(l), rl[path[l][0]], common_suffix(A, path[x], path[l]), 0)
        m = np.ascontiguousarray(meas[rows_m])
        Y = np.full(n_strip, np.nan)
        n_d2 = len(m) * len(cols)
        out = np.full(1 + n_d2 + (len(m) + 1) // 2, np.nan); out[0] = 0.0
        ticket = np.zeros(len(m), dtype=np.uint32)
        rc = lib.emu_gate(int(A["n_fronts"]), *[ptr(t) for t in tabs], ptr(walks), len(walks), ptr(steps), len(steps), K, max_p, max_front, ptr(Y),
                          C.c_longlong(n_strip), 3, pose_ld, ptr(pose_est), len(planes), plane_ld, ptr(plane_est), ptr(cands), len(cols), ptr(m), len(m),
                          C.c_longlong(int(walks[0]["strip"])), 2, int(rl[path[x][0]]), mode, ptr(ticket), ptr(out))
        assert rc == 0 and out[0] == 0.0 and not ticket.any()
        return out[1:1 + n_d2].reshape(len(m), len(cols)).copy(), out[1 + n_d2:].view(np.int32)[:len(m)].copy()

    d2, best = run(planes, list(range(M)))
    ref = np.zeros_like(d2); ref2 = np.zeros_like(d2)
    rec = np.zeros(30)
    for i in range(M):
        for k, l in enumerate(planes):
            lib.emu_lin_plane_obs(mode, ptr(pose), ptr(np.ascontiguousarray(pl[k])), ptr(np.ascontiguousarray(meas[i, :4])), ptr(np.ascontiguousarray(meas[i, 4:])), ptr(rec))
            Jw = np.hstack([rec[:18].reshape(3, 6), rec[18:27].reshape(3, 3)]); r = rec[27:]
            ref[i, k], ref2[i, k] = (r @ np.linalg.solve(np.eye(3) + Jw @ _sigma9(Sx, span, x, l) @ Jw.T, r) for Sx in (S1, S2))
    e = float(np.max(np.abs(d2 - ref) / ref)); d = float(np.max(np.abs(ref2 - ref) / ref))
    print(f"GATE host-emulated kernels mode {mode}: M {M} L {len(planes)} e {e:.3e} d {d:.3e} bound {max(16 * d, 1e-12):.3e}")
    assert e <= max(16 * d, 1e-12), (e, d)
    assert list(best) == [int(np.argmin(ref[i])) for i in range(M)] == [0, 1, 2]
    # a candidate's bits do not depend on the rest of the call (other candidates change K and the strips' places)
    sub = [planes[k] for k in (4, 1, 6)]
    d2s, bs = run(sub, [2, 0])
    assert np.array_equal(d2s, d2[[2, 0]][:, [4, 1, 6]])
    assert list(bs) == [int(np.argmin(d2s[0])), int(np.argmin(d2s[1]))]


def test_symbols_are_declared_exported_and_bound(built):
    hdr = open(os.path.join(ROOT, "include", "pps.h")).read()
    lib = C.CDLL(P.LIB_PATH)
    for name in ("pps_assoc_gate", "pps_assoc_gate_last", "pps_debug_assoc_gate_records"):
        assert re.search(r"\b" + name + r"\s*\(", hdr) and name in P.SYMBOLS and getattr(lib, name) is not None
    assert P.lib().pps_version() == 305                    # detected by symbol lookup, not by a version bump


def test_arguments_and_state_without_a_device(built):
    spec = synth.small_world(5, 3, seed=1)
    g = P.Graph(); nid, _ = spec.replay(g)
    poses = [int(n) for n, t in zip(nid, spec.node_type) if t == synth.NODE_POSE]
    planes = [int(n) for n, t in zip(nid, spec.node_type) if t != synth.NODE_POSE]
    m = np.array([[0.0, 0, 1, -1]]); w = synth._ut_diag([50.0] * 3)[None]
    for call in (lambda: g.assoc_gate(poses[-1], m, w), lambda: g.assoc_gate(poses[0], m, w, planes[:1])):
        with pytest.raises(P.PpsError) as e:
            call()
        assert e.value.code == P.PPS_ESTATE and "no valid covariance recovery" in str(e.value)
    bad = len(spec.node_type) + 7
    for call in (lambda: g.assoc_gate(bad, m, w), lambda: g.assoc_gate(-1, m, w), lambda: g.assoc_gate(planes[0], m, w),       # unknown id / not a pose
                 lambda: g.assoc_gate(poses[0], m, w, [bad]), lambda: g.assoc_gate(poses[0], m, w, [poses[1]]),                 # unknown / not a plane
                 lambda: g.assoc_gate(poses[0], m, w, [planes[0], planes[1], planes[0]]),                                        # a plane twice
                 lambda: g.assoc_gate(poses[0], [[np.nan, 0, 1, 0]], w), lambda: g.assoc_gate(poses[0], m, [[np.inf] * 6])):
        with pytest.raises(P.PpsError) as e:
            call()
        assert e.value.code == P.PPS_EINVAL
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    d2 = np.full(8, -7.0); best = np.full(2, -7, dtype=np.int32)
    ids = np.array(planes[:2], dtype=np.int32)
    args = lambda **k: [k.get("h", g.h), poses[0], k.get("nm", 1), k.get("m", m.ctypes.data_as(dp)), k.get("w", w.ctypes.data_as(dp)), k.get("np", 2),
                        k.get("ids", ids.ctypes.data_as(ip)), k.get("d2", d2.ctypes.data_as(dp)), best.ctypes.data_as(ip)]
    for k in ({"h": None}, {"m": None}, {"w": None}, {"d2": None}, {"nm": -1}, {"np": -1}):
        assert g.L.pps_assoc_gate(*args(**k)) == P.PPS_EINVAL, k
    assert g.L.pps_assoc_gate(*args(np=-5, ids=None)) == P.PPS_ESTATE                 # plane_ids NULL: n_planes is ignored
    assert g.L.pps_assoc_gate(*args(nm=0)) == P.PPS_OK and g.L.pps_assoc_gate(*args(np=0)) == P.PPS_OK
    assert np.all(d2 == -7.0) and np.all(best == -7)                                  # zero counts: outputs untouched
    sec = C.c_double(-1.0); n = C.c_int(-1)
    assert g.L.pps_assoc_gate_last(g.h, C.byref(sec), C.byref(n)) == P.PPS_OK and (sec.value, n.value) == (0.0, 0)
    assert g.L.pps_assoc_gate_last(g.h, None, None) == P.PPS_OK and g.L.pps_assoc_gate_last(None, None, None) == P.PPS_EINVAL
    need = C.c_int64(-1)
    assert g.L.pps_debug_assoc_gate_records(g.h, 0, None, C.byref(need)) == P.PPS_ESTATE      # no gate has run on this handle
    assert g.L.pps_debug_assoc_gate_records(g.h, 0, None, None) == P.PPS_EINVAL
    removed = planes[-1]; g.remove_node(removed)
    with pytest.raises(P.PpsError) as e:
        g.assoc_gate(poses[0], m, w, [removed])
    assert e.value.code == P.PPS_EINVAL
    g.close()
