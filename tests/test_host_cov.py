"""CPU: the index plan of the covariance recovery (csrc/pps_cov.hip, csrc/pps_cov.cpp) before any kernel runs.

A numpy emulation of the per-front recursion (tests/cov_helpers.py), driven only by what pps_analysis_dump exports, must reproduce
np.linalg.inv(H) on every entry inside the pattern of the factor: whole fronts, the diagonal block of every node and the cross block
of every pair of nodes joined by a factor, each at 1e-9 relative (Frobenius).  H is a random positive definite matrix with the
graph's sparsity (a random Jacobian per factor): the plan depends on the structure alone.  Then the C-ABI surface without a device:
symbols, state and argument errors."""
import subprocess
import sys

import numpy as np
import pytest

import pop_up_slam_amd as P
from cov_helpers import block_from_fronts, emulate_selected_inverse, factor_pairs, locate_block, node_layout, rel_err
from pop_up_slam_amd import pipeline, synth

COV_SYMBOLS = ["pps_cov_recover", "pps_cov_marginals", "pps_cov_access", "pps_cov_joint", "pps_cov_last_times"]


def _spec_graph(spec):
    g = P.Graph(); spec.replay(g)
    dims = [6 if t == synth.NODE_POSE else 3 for t in spec.node_type]
    return g, dims, [(int(a), int(b)) for a, b in spec.f_nodes], [int(m) for m in np.where(spec.f_type <= 1, 6, 3)]


def _grown_graph(frames=40):
    """the topology of the C5 frame loop (tools/c5_fronts_cpu.py), one incremental analysis per frame"""
    fr_list = pipeline.popup_sequence(frames)
    g = P.Graph()
    ut6 = pipeline.PopupSlamPipeline.POSE_UT; ut3 = synth._ut_diag([1.0] * 3)
    dims, f_nodes, f_dim, poses, lm = [], [], [], [], {}
    for fr in fr_list:
        est = fr.true_pose if hasattr(fr, "true_pose") else fr.odo
        p = g.add_pose(np.asarray(est, dtype=np.float64)); dims.append(6)
        if poses:
            g.add_odometry(poses[-1], p, np.zeros(6), ut6); f_nodes.append((poses[-1], p))
        else:
            g.add_pose_prior(p, np.zeros(6), ut6); f_nodes.append((p, -1))
        f_dim.append(6)
        poses.append(p)
        for key in ["g"] + list(fr.ids):
            if key not in lm:
                lm[key] = g.add_plane(np.array([0.0, 0.0, -1.0, 0.0])); dims.append(3)
                if key == "g":
                    g.add_plane_prior(lm[key], synth.GROUND, ut3); f_nodes.append((lm[key], -1)); f_dim.append(3)
            g.add_plane_obs(p, lm[key], np.array([0.0, 0.0, -1.0, 0.0]), ut3); f_nodes.append((p, lm[key])); f_dim.append(3)
        g.analyze()
    assert g.analysis_reuse()[0] > 0                      # the last analysis was an incremental one
    return g, dims, f_nodes, f_dim


CASES = {
    "small_world": lambda: _spec_graph(synth.small_world(5, 3)),
    "corridor60": lambda: _spec_graph(synth.corridor(60, 14, seed=7)),
    "grown40": _grown_graph,
}


def _random_h(A, lay, f_nodes, f_dim, seed):
    rng = np.random.default_rng(seed)
    n = A["n_scalars"]
    H = 1e-3 * np.eye(n)
    for (a, b), m in zip(f_nodes, f_dim):
        cols = list(range(lay[a][0], lay[a][0] + lay[a][1]))
        if b >= 0:
            cols += list(range(lay[b][0], lay[b][0] + lay[b][1]))
        J = rng.normal(size=(m, len(cols)))
        H[np.ix_(cols, cols)] += J.T @ J
    return H


@pytest.mark.parametrize("case", sorted(CASES))
def test_recursion_over_the_dumped_fronts_reproduces_the_dense_inverse(built, case):
    g, dims, f_nodes, f_dim = CASES[case]()
    g.analyze()
    A = g.analysis_dump()
    lay = node_layout(A, dims)
    H = _random_h(A, lay, f_nodes, f_dim, seed=11)
    S = np.linalg.inv(H)
    full, epos = emulate_selected_inverse(A, H)
    worst = 0.0
    for s in range(A["n_fronts"]):                                            # every entry the device computes
        p, po = int(A["f_p"][s]), int(A["f_poff"][s])
        idx = np.concatenate([A["pidx"][po:po + p], A["bidx"][A["f_bidx_off"][s]:A["f_bidx_off"][s + 1]]]).astype(np.int64)
        e = rel_err(full[s], S[np.ix_(idx, idx)]); worst = max(worst, e)
        assert e <= 1e-9, (case, "front", s, e)
        assert np.array_equal(full[s][:p, :p], full[s][:p, :p].T)
    pairs = [(i, i) for i in lay] + factor_pairs(f_nodes) + [(b, a) for a, b in factor_pairs(f_nodes)]
    for r, c in pairs:                                                        # ... found where the read calls look for it
        loc = locate_block(A, epos, lay, r, c)
        assert loc is not None, (case, r, c, "a factor-joined pair must share a front")
        got = block_from_fronts(full, loc, lay[r][1], lay[c][1])
        ref = S[lay[r][0]:lay[r][0] + lay[r][1], lay[c][0]:lay[c][0] + lay[c][1]]
        e = rel_err(got, ref); worst = max(worst, e)
        assert e <= 1e-9, (case, r, c, e)
    print(f"{case}: {A['n_fronts']} fronts, {len(pairs)} blocks, worst relative error {worst:.2e}")
    # a pair that shares no front is reported as outside the pattern, not looked up somewhere else
    poses = [i for i in lay if lay[i][1] == 6]
    if len(poses) >= 30:
        assert locate_block(A, epos, lay, poses[0], poses[-1]) is None or A["n_fronts"] == 1


@pytest.mark.parametrize("case", sorted(CASES))
def test_kernel_source_emulated_on_the_host_reproduces_the_dense_inverse(built, case, tmp_path):
    """csrc/pps_cov.hip compiled for the host (tests/cpp/cov_emu.cpp: one std::thread per thread of a workgroup) on the panels of a dense
    Cholesky factor in the device layout; entries the device leaves unspecified (above the diagonal of L_A, the buffers before they are
    written) are NaN.  Every entry of [S_AA; S_BA] and of S_BB against np.linalg.inv at 1e-9 relative per front; S_AA symmetric bit for bit."""
    import ctypes as C
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = tmp_path / "libcovemu.so"
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-fPIC", "-shared", "-pthread", "-I", os.path.join(root, "tests", "cpp", "block_emu"),
                           "-I", os.path.join(root, "pop_up_slam_amd", "csrc"), "-x", "c++", os.path.join(root, "tests", "cpp", "cov_emu.cpp"), "-o", str(so)])
    lib = C.CDLL(str(so))
    g, dims, f_nodes, f_dim = CASES[case]()
    g.analyze()
    A = g.analysis_dump()
    lay = node_layout(A, dims)
    H = _random_h(A, lay, f_nodes, f_dim, seed=5)
    Sref = np.linalg.inv(H)
    pidx = np.asarray(A["pidx"]); n = len(pidx)
    Lg = np.linalg.cholesky(H[np.ix_(pidx, pidx)])
    epos = np.empty(n, dtype=np.int64); epos[pidx] = np.arange(n)
    L = np.full(A["L_size"], np.nan); U = np.full(A["U_size"], np.nan); S = np.full(A["L_size"], np.nan)
    for s in range(A["n_fronts"]):
        p, b, po = int(A["f_p"][s]), int(A["f_b"][s]), int(A["f_poff"][s])
        piv = np.arange(po, po + p); bnd = epos[A["bidx"][A["f_bidx_off"][s]:A["f_bidx_off"][s + 1]]]
        pan = np.vstack([Lg[np.ix_(piv, piv)], Lg[np.ix_(bnd, piv)], np.zeros((1, p))])
        pan[:p][np.triu_indices(p, 1)] = np.nan
        L[A["f_Loff"][s]:A["f_Loff"][s] + (p + b + 1) * p] = pan.ravel()
    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)
    i64 = lambda v: np.ascontiguousarray(v, dtype=np.int64)
    arrs = [i32(A["level_off"]), i32(A["level_fronts"]), i32(A["f_p"]), i32(A["f_b"]), i64(A["f_Loff"]), i64(A["f_Uoff"]), i32(A["f_cmap_off"]),
            i32(A["cmap"]), i32(A["f_parent"]), L, U, S, np.zeros(4)]
    lib.emu_cov(int(A["n_fronts"]), int(A["n_levels"]), *[a.ctypes.data_as(C.c_void_p) for a in arrs])
    assert arrs[-1][2] == 0.0                                # status word: positive definite, every index inside its front
    for s in range(A["n_fronts"]):
        p, b, po = int(A["f_p"][s]), int(A["f_b"][s]), int(A["f_poff"][s])
        idxp = pidx[po:po + p]; idxb = np.asarray(A["bidx"][A["f_bidx_off"][s]:A["f_bidx_off"][s + 1]])
        pan = S[A["f_Loff"][s]:A["f_Loff"][s] + (p + b) * p].reshape(p + b, p)
        assert np.array_equal(pan[:p], pan[:p].T)
        assert rel_err(pan[:p], Sref[np.ix_(idxp, idxp)]) <= 1e-9, (case, s)
        if b:
            assert rel_err(pan[p:], Sref[np.ix_(idxb, idxp)]) <= 1e-9, (case, s)
            assert rel_err(U[A["f_Uoff"][s]:A["f_Uoff"][s] + b * b].reshape(b, b), Sref[np.ix_(idxb, idxb)]) <= 1e-9, (case, s)
    # a singular system (its last pivot collapsed) raises the not-positive-definite status instead of delivering noise
    s = A["n_fronts"] - 1; p = int(A["f_p"][s])
    L[A["f_Loff"][s] + (p - 1) * p + (p - 1)] *= 1e-9
    arrs[-1][:] = 0
    lib.emu_cov(int(A["n_fronts"]), int(A["n_levels"]), *[a.ctypes.data_as(C.c_void_p) for a in arrs])
    assert arrs[-1][2] == 1.0


def test_symbols_are_declared_exported_and_bound(built):
    import ctypes as C
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pps.h")).read()
    lib = C.CDLL(P.LIB_PATH)
    for s in COV_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in P.SYMBOLS
        assert getattr(lib, s) is not None
    assert P.lib().pps_version() == 305                    # detected by symbol lookup, not by a version bump (305: pps_debug_solve)


def test_reads_without_a_recovery_and_bad_ids(built):
    spec = synth.small_world(5, 3, seed=1)
    g = P.Graph(); nid, _ = spec.replay(g)
    for call in (lambda: g.cov_marginals(), lambda: g.cov_marginals([int(nid[0])]), lambda: g.cov_access([(int(nid[0]), int(nid[1]))]),
                 lambda: g.cov_joint([int(nid[0]), int(nid[1])])):
        with pytest.raises(P.PpsError) as e:
            call()
        assert e.value.code == P.PPS_ESTATE and "no valid covariance recovery" in str(e.value)
    bad = len(spec.node_type) + 7
    for call in (lambda: g.cov_marginals([bad]), lambda: g.cov_marginals([-1]), lambda: g.cov_access([(int(nid[0]), bad)]),
                 lambda: g.cov_access([(bad, int(nid[0]))])):
        with pytest.raises(P.PpsError) as e:
            call()
        assert e.value.code == P.PPS_EINVAL
    import ctypes as C
    out = np.zeros(72)
    ids = np.array([int(nid[0]), bad], dtype=np.int32)
    assert g.L.pps_cov_joint(g.h, 2, ids.ctypes.data_as(C.POINTER(C.c_int)), out.ctypes.data_as(C.POINTER(C.c_double))) == P.PPS_EINVAL
    ids[1] = ids[0]                                         # the same node twice
    assert g.L.pps_cov_joint(g.h, 2, ids.ctypes.data_as(C.POINTER(C.c_int)), out.ctypes.data_as(C.POINTER(C.c_double))) == P.PPS_EINVAL
    assert g.L.pps_cov_marginals(g.h, 3, None, out.ctypes.data_as(C.POINTER(C.c_double)), None) == P.PPS_EINVAL     # NULL ids: n must be all nodes
    assert g.L.pps_cov_recover(None) == P.PPS_EINVAL
    removed = int(nid[-1]); g.remove_node(removed)
    with pytest.raises(P.PpsError) as e:
        g.cov_marginals([removed])
    assert e.value.code == P.PPS_EINVAL
    e2 = P.Graph()
    with pytest.raises(P.PpsError) as e:
        e2.cov_recover()
    assert e.value.code == P.PPS_ESTATE                    # empty graph


def test_dense_front_graph_is_refused_before_the_device_is_touched(built):
    """a loop-closure graph in the dense-front class: PPS_ESTATE from the host-side analysis alone (no device needed)"""
    import os
    from pop_up_slam_amd import graphio
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "isam_data", "sphere2500.txt")
    spec = graphio.load_edge3_log(path, max_lines=1400)
    g = P.Graph(); spec.replay(g); g.analyze()
    assert g.stats()["max_front"] > 127
    with pytest.raises(P.PpsError) as e:
        g.cov_recover()
    assert e.value.code == P.PPS_ESTATE and "dense-front" in str(e.value)


def test_recover_without_gpu_fails_loudly(built):
    probe = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.is_available())"], capture_output=True,
                           text=True, timeout=300)
    if probe.stdout.strip().endswith("True"):
        pytest.skip("GPU present")
    spec = synth.small_world(5, 3, seed=1)
    g = P.Graph(); spec.replay(g)
    with pytest.raises(P.PpsError) as e:
        g.cov_recover()
    assert e.value.code == P.PPS_EHIP
    with pytest.raises(P.PpsError) as e:
        g.cov_marginals()
    assert e.value.code == P.PPS_ESTATE
