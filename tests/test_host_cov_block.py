"""CPU: the algorithm of pps_cov_block (csrc/pps_cov.hip: k_cov_path, k_cov_gram; csrc/pps_query.cpp) before any kernel runs on a device.

Sigma(R, C) = (L^-1 E_R)' (L^-1 E_C): one walk up the elimination tree per node, one Gram product over the pivots of common ancestors.
A numpy restatement (tests/cov_block_helpers.py), driven only by what pps_analysis_dump exports, and the kernel source itself compiled
for the host (tests/cpp/cov_block_emu.cpp) are compared with the dense inverse of a random positive definite H of the graph's sparsity.
Error measure per node pair: e = |M - M0|_F / sqrt(|S0(r, r)|_F |S0(c, c)|_F); yardstick d = the same measure between two CPU inverses
that share no code path (cov_helpers.cpu_inverses), maximum over the same blocks; bound e <= max(16 d, 1e-12), factor and floor of
tests/test_gpu_cov.py.  e and d are printed per case (-s).  Then the C-ABI surface without a device: symbol, state and argument errors."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pop_up_slam_amd as P
from cov_block_helpers import (common_suffix, elimination_positions, emulate_block, node_front, path_to_root, query_errors, request_tables,
                               root_lengths)
from cov_helpers import cpu_inverses, node_layout
from pop_up_slam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = {
    "small_world_5_3": lambda: synth.small_world(5, 3),
    "corridor_60_14": lambda: synth.corridor(60, 14, seed=7),
    "corridor_150_32": lambda: synth.corridor(150, 32, seed=8),
}


def _spec_graph(spec):
    g = P.Graph(); spec.replay(g)
    dims = [6 if t == synth.NODE_POSE else 3 for t in spec.node_type]
    return g, dims, [(int(a), int(b)) for a, b in spec.f_nodes], [int(m) for m in np.where(spec.f_type <= 1, 6, 3)]


def _random_h(A, lay, f_nodes, f_dim, seed):
    rng = np.random.default_rng(seed)
    H = 1e-3 * np.eye(A["n_scalars"])
    for (a, b), m in zip(f_nodes, f_dim):
        cols = list(range(lay[a][0], lay[a][0] + lay[a][1]))
        if b >= 0:
            cols += list(range(lay[b][0], lay[b][0] + lay[b][1]))
        J = rng.normal(size=(m, len(cols)))
        H[np.ix_(cols, cols)] += J.T @ J
    return H


def _setup(case, seed):
    g, dims, f_nodes, f_dim = _spec_graph(CASES[case]())
    g.analyze()
    A = g.analysis_dump()
    lay = node_layout(A, dims)
    H = _random_h(A, lay, f_nodes, f_dim, seed)
    S1, S2 = cpu_inverses(H)
    span = lambda n: slice(lay[n][0], lay[n][0] + lay[n][1])
    return A, lay, H, S1, S2, span


def _queries(lay):
    """(rows, cols or None): the pose pairs (first, last), (first, middle), (middle, last) and the joint of every tenth node"""
    poses = [n for n in sorted(lay) if lay[n][1] == 6]
    first, mid, last = poses[0], poses[len(poses) // 2], poses[-1]
    return [([first], [last]), ([first], [mid]), ([mid], [last]), (sorted(lay)[::10], None)]


@pytest.mark.parametrize("case", sorted(CASES))
def test_path_walk_and_suffix_gram_reproduce_the_dense_inverse(built, case):
    A, lay, H, S1, S2, span = _setup(case, seed=11)
    e = d = 0.0
    for rows, cols in _queries(lay):
        M = emulate_block(A, H, lay, rows, cols)
        assert np.all(np.isfinite(M))                                    # (the padding in front of a strip is NaN: it is never read)
        if cols is None:
            assert np.array_equal(M, M.T)
        eq, dq = query_errors(M, S1, S2, rows, rows if cols is None else cols, span)
        e, d = max(e, eq), max(d, dq)
    print(f"COVBLOCK numpy {case}: fronts {A['n_fronts']} e {e:.3e} d {d:.3e} bound {max(16 * d, 1e-12):.3e}")
    assert e <= max(16 * d, 1e-12), (case, e, d)


@pytest.mark.parametrize("case", sorted(CASES))
def test_kernel_source_emulated_on_the_host_reproduces_the_dense_inverse(built, case, tmp_path):
    """k_cov_path / k_cov_gram themselves, one std::thread per GPU thread, on the panels of a dense Cholesky factor in the device layout
    (above the diagonal of L_A, the rhs row and the strips before they are written: NaN), with the request tables of csrc/pps_query.cpp
    restated in tests/cov_block_helpers.py.  Same measure and bound; the joint is symmetric bit for bit, and Sigma(r, c) is the transpose
    of Sigma(c, r) bit for bit."""
    so = tmp_path / "libcovblockemu.so"
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-I", os.path.join(ROOT, "tests", "cpp", "block_emu"),
                           "-I", os.path.join(ROOT, "pop_up_slam_amd", "csrc"), "-x", "c++", os.path.join(ROOT, "tests", "cpp", "cov_block_emu.cpp"), "-o", str(so)])
    lib = C.CDLL(str(so))
    A, lay, H, S1, S2, span = _setup(case, seed=5)
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

    def run(rows, cols):
        walks, steps, pairs, K, n_strip, shape = request_tables(A, lay, rows, cols)
        Y = np.full(n_strip, np.nan); out = np.full(1 + shape[0] * shape[1], np.nan); out[0] = 0.0
        rc = lib.emu_cov_block(int(A["n_fronts"]), *[ptr(t) for t in tabs], ptr(walks), len(walks), ptr(steps), len(steps), K, max_p, max_front,
                               ptr(Y), C.c_longlong(n_strip), ptr(pairs), len(pairs), ptr(out), C.c_longlong(shape[0] * shape[1]))
        assert rc == 0 and out[0] == 0.0                         # status word: every index inside its front and its strip
        return out[1:].reshape(shape)

    e = d = 0.0
    for rows, cols in _queries(lay):
        M = run(rows, cols)
        assert np.all(np.isfinite(M))
        if cols is None:
            assert np.array_equal(M, M.T)
        else:
            assert np.array_equal(run(cols, rows), M.T)
        eq, dq = query_errors(M, S1, S2, rows, rows if cols is None else cols, span)
        e, d = max(e, eq), max(d, dq)
    print(f"COVBLOCK host-emulated kernels {case}: e {e:.3e} d {d:.3e} bound {max(16 * d, 1e-12):.3e}")
    assert e <= max(16 * d, 1e-12), (case, e, d)
    # a step that names a front outside the tree raises the status word instead of reading there
    walks, steps, pairs, K, n_strip, shape = request_tables(A, lay, *_queries(lay)[0])
    steps["front"][-1] = A["n_fronts"] + 3
    Y = np.zeros(n_strip); out = np.zeros(1 + shape[0] * shape[1])
    lib.emu_cov_block(int(A["n_fronts"]), *[ptr(t) for t in tabs], ptr(walks), len(walks), ptr(steps), len(steps), K, max_p, max_front,
                      ptr(Y), C.c_longlong(n_strip), ptr(pairs), len(pairs), ptr(out), C.c_longlong(shape[0] * shape[1]))
    assert out[0] == 64.0


@pytest.mark.parametrize("case", sorted(CASES))
def test_strips_aligned_at_the_root_end_share_their_common_ancestors(built, case):
    """for random node pairs: the common-suffix length computed from the two paths equals the number of pivots in their common ancestors,
    and every common ancestor starts at the same row of both strips"""
    g, dims, _, _ = _spec_graph(CASES[case]())
    g.analyze()
    A = g.analysis_dump()
    lay = node_layout(A, dims)
    _, epos = elimination_positions(A)
    rl = root_lengths(A)
    rng = np.random.default_rng(3)
    nodes = sorted(lay)
    for _ in range(200):
        a, b = (int(x) for x in rng.choice(nodes, 2, replace=False))
        pa, pb = (path_to_root(A, node_front(A, epos, lay[n][0])[0]) for n in (a, b))
        shared = set(pa) & set(pb)
        assert common_suffix(A, pa, pb) == sum(int(A["f_p"][s]) for s in shared)
        K = max(rl[pa[0]], rl[pb[0]])
        for s in shared:                                                  # (row of front s in a strip: K - rootlen(s), the same for both)
            assert K - rl[s] >= max(K - rl[pa[0]], K - rl[pb[0]])
        if shared:
            assert pa[len(pa) - len(shared):] == pb[len(pb) - len(shared):]


def test_symbol_is_declared_exported_and_bound(built):
    hdr = open(os.path.join(ROOT, "include", "pps.h")).read()
    lib = C.CDLL(P.LIB_PATH)
    assert re.search(r"\bpps_cov_block\s*\(", hdr)
    assert "pps_cov_block" in P.SYMBOLS
    assert getattr(lib, "pps_cov_block") is not None
    assert P.lib().pps_version() == 305                    # detected by symbol lookup, not by a version bump (305: pps_debug_solve)


def test_block_without_a_recovery_and_bad_arguments(built):
    spec = synth.small_world(5, 3, seed=1)
    g = P.Graph(); nid, _ = spec.replay(g)
    a, b = int(nid[0]), int(nid[1])
    for call in (lambda: g.cov_block([a]), lambda: g.cov_block([a], [b]), lambda: g.cov_block([a, b], [a, b])):
        with pytest.raises(P.PpsError) as e:
            call()
        assert e.value.code == P.PPS_ESTATE and "no valid covariance recovery" in str(e.value)
    bad = len(spec.node_type) + 7
    for call in (lambda: g.cov_block([bad]), lambda: g.cov_block([-1]), lambda: g.cov_block([a], [bad]), lambda: g.cov_block([a, a]),
                 lambda: g.cov_block([a, b, a], [b]), lambda: g.cov_block([a], [b, b])):
        with pytest.raises(P.PpsError) as e:
            call()
        assert e.value.code == P.PPS_EINVAL
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    out = np.zeros(144)
    ids = np.array([a, b], dtype=np.int32)
    assert g.L.pps_cov_block(g.h, 2, None, 0, None, out.ctypes.data_as(dp)) == P.PPS_EINVAL                    # NULL rows
    assert g.L.pps_cov_block(g.h, 2, ids.ctypes.data_as(ip), 0, None, None) == P.PPS_EINVAL                    # NULL out
    assert g.L.pps_cov_block(None, 2, ids.ctypes.data_as(ip), 0, None, out.ctypes.data_as(dp)) == P.PPS_EINVAL
    assert g.L.pps_cov_block(g.h, -1, ids.ctypes.data_as(ip), 0, None, out.ctypes.data_as(dp)) == P.PPS_EINVAL
    assert g.L.pps_cov_block(g.h, 1, ids.ctypes.data_as(ip), -1, ids.ctypes.data_as(ip), out.ctypes.data_as(dp)) == P.PPS_EINVAL
    assert g.L.pps_cov_block(g.h, 2, ids.ctypes.data_as(ip), -5, None, out.ctypes.data_as(dp)) == P.PPS_ESTATE  # cols NULL: nc is ignored
    removed = int(nid[-1]); g.remove_node(removed)
    with pytest.raises(P.PpsError) as e:
        g.cov_block([removed])
    assert e.value.code == P.PPS_EINVAL
