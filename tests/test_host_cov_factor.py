"""CPU: pps_cov_factor and the path walk for wide fronts (csrc/pps_cov_wide.hip: k_cov_path_wide, k_cov_pivots) before any kernel runs on a
device.

  1. the C-ABI surface without a device: symbols, NULL handle, empty graph, no factor, PPS_EHIP without a GPU, the read calls' texts
  2. the shape contract of the node sets the GPU tests query (tests/cov_factor_helpers.py), from pps_analysis_dump alone
  3. the wide kernel's source compiled for the host (tests/cpp/cov_wide_emu.cpp: one std::thread per GPU thread, std::barrier as the
     workgroup barrier) on the panels of a dense Cholesky factor of a random positive definite H of the graph's sparsity, in the device
     layout with NaN wherever the device leaves memory unspecified: against the dense inverse on two dense-front graphs (and on the
     graph whose fronts pass 1 024 rows), bit for bit against the host-compiled k_cov_path on a band graph
  4. the graphs of the not-positive-definite GPU test: H from the CPU oracle's Jacobians, factored in the analysis's elimination order,
     has a pivot that is not positive or below 1e-7 of its front's largest

Error measure and bound of tests/test_host_cov_block.py: e = |M - M0|_F / sqrt(|S0(r, r)|_F |S0(c, c)|_F) per node pair, d the same between
two CPU inverses, e <= max(16 d, 1e-12); one line per graph (-s)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pop_up_slam_amd as P
from cov_block_helpers import elimination_positions, query_errors, request_tables
from cov_factor_helpers import DENSE, GRAPHS, WIDE, assert_contract, choose_nodes
from cov_helpers import cpu_inverses
from linsolve_helpers import assert_case_shapes, loop_graph, spec_layout
from pop_up_slam_amd import graphio, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPHERE = os.path.join(ROOT, "tests", "golden", "isam_data", "sphere2500.txt")


def _analysed(spec, mode=1):
    g = P.Graph(jacobian_mode=mode); spec.replay(g); g.analyze()
    A = g.analysis_dump()
    return g, A, spec_layout(spec, A)


# ---- 1. the surface ---------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound(built):
    hdr = open(os.path.join(ROOT, "include", "pps.h")).read()
    lib = C.CDLL(P.LIB_PATH)
    for name in ("pps_cov_factor", "pps_debug_cov_path_form"):
        assert re.search(r"\b" + name + r"\s*\(", hdr) and name in P.SYMBOLS and getattr(lib, name) is not None
    assert P.lib().pps_version() == 305                    # detected by symbol lookup, not by a version bump


def test_argument_and_state_contract_without_a_device(built):
    L = P.lib()
    assert L.pps_cov_factor(None) == P.PPS_EINVAL and L.pps_debug_cov_path_form(None, 0) == P.PPS_EINVAL
    empty = P.Graph()
    with pytest.raises(P.PpsError) as e:
        empty.cov_factor()
    assert e.value.code == P.PPS_ESTATE and "empty graph" in str(e.value)
    nofactor = P.Graph(); nofactor.add_pose([0, 0, 0, 0, 0, 0, 1])
    with pytest.raises(P.PpsError) as e:
        nofactor.cov_factor()
    assert e.value.code == P.PPS_ENOTPD
    spec = synth.small_world(5, 3, seed=1)
    g = P.Graph(); nid, _ = spec.replay(g)
    a, b = int(nid[0]), int(nid[1])
    g.debug_cov_path_form(1); g.debug_cov_path_form(0)
    for form in (-1, 2):
        with pytest.raises(P.PpsError) as e:
            g.debug_cov_path_form(form)
        assert e.value.code == P.PPS_EINVAL
    reads = (lambda: g.cov_block([a]), lambda: g.cov_block([a], [b]), lambda: g.cov_marginals([a]), lambda: g.cov_access([(a, b)]), lambda: g.cov_joint([a, b]))
    for read in reads:                                     # neither call made: today's text, word for word
        with pytest.raises(P.PpsError) as e:
            read()
        assert e.value.code == P.PPS_ESTATE and str(e.value).endswith(
            "no valid covariance recovery: call pps_cov_recover (a recovery ends with every change of the estimate, the measurements or the topology)")
    try:
        g.cov_factor()
    except P.PpsError as err:                              # no device here: loudly, and nothing valid is left behind
        assert err.code == P.PPS_EHIP
        for read in reads:
            with pytest.raises(P.PpsError) as e:
                read()
            assert e.value.code == P.PPS_ESTATE and "no valid covariance recovery" in str(e.value)
    else:                                                  # a device: the factor is held, the selected inverse is not, and the text says so
        assert np.all(np.isfinite(g.cov_block([a], [b])))
        for read in reads[2:]:
            with pytest.raises(P.PpsError) as e:
                read()
            assert e.value.code == P.PPS_ESTATE and "pps_cov_factor" in str(e.value) and "pps_cov_recover" in str(e.value)


def test_dense_front_graph_is_still_refused_by_the_full_recovery(built):
    g, A, _ = _analysed(graphio.load_edge3_log(SPHERE, max_lines=1400))
    assert A["max_front"] > 127
    with pytest.raises(P.PpsError) as e:
        g.cov_recover()
    assert e.value.code == P.PPS_ESTATE and "dense-front" in str(e.value)


# ---- 2. the node sets -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GRAPHS) + ["sphere2500_1400"])
def test_node_sets_meet_their_shape_contract(built, name):
    """per graph: a walk through a front wider than MIN_ROWS (256 on dense_100p_400l: a thread of the wide kernel takes more than one row;
    1 024 on the fifth graph), a node of the root front (b = 0), a node off the first pivot of its front, two nodes whose paths diverge,
    two nodes one of whose fronts is an ancestor of the other's"""
    spec = GRAPHS[name]() if name in GRAPHS else graphio.load_edge3_log(SPHERE, max_lines=1400)
    g, A, lay = _analysed(spec)
    if name in DENSE:
        assert_case_shapes(name, A)
    assert A["max_front"] > 127 and max(A["f_p"]) <= 64
    sel = choose_nodes(A, lay)
    c = assert_contract(name, A, lay, sel)
    assert 8 <= len(sel) <= 14 and len(set(sel)) == len(sel)
    if any(d == 3 for _, d in lay.values()):
        assert any(lay[n][1] == 3 for n in sel) and any(lay[n][1] == 6 for n in sel)
    print(f"COVFACTOR nodes {name}: max front {A['max_front']} fronts {A['n_fronts']} nodes {sel} widest front on their paths {c['rows']} rows")


# ---- 3. the kernel source on the host ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = tmp_path_factory.mktemp("covwide") / "libcovwideemu.so"
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-I", os.path.join(ROOT, "tests", "cpp", "block_emu"),
                           "-I", os.path.join(ROOT, "pop_up_slam_amd", "csrc"), "-x", "c++", os.path.join(ROOT, "tests", "cpp", "cov_wide_emu.cpp"), "-o", str(so)])
    return C.CDLL(str(so))


def _random_h(A, lay, spec, seed):
    rng = np.random.default_rng(seed)
    H = 1e-3 * np.eye(A["n_scalars"])
    for (a, b), t in zip(spec.f_nodes, spec.f_type):
        cols = list(range(lay[int(a)][0], lay[int(a)][0] + lay[int(a)][1]))
        if b >= 0:
            cols += list(range(lay[int(b)][0], lay[int(b)][0] + lay[int(b)][1]))
        J = rng.normal(size=(6 if t <= 1 else 3, len(cols)))
        H[np.ix_(cols, cols)] += J.T @ J
    return H


def _device_panels(A, H):
    """the factor of H as the device holds it: [L_A; L_B; rhs row] per front, NaN above the diagonal of L_A and in the rhs row"""
    pidx, epos = elimination_positions(A)
    Lg = np.linalg.cholesky(H[np.ix_(pidx, pidx)])
    L = np.full(A["L_size"], np.nan)
    for s in range(A["n_fronts"]):
        p, b, po = int(A["f_p"][s]), int(A["f_b"][s]), int(A["f_poff"][s])
        piv = np.arange(po, po + p); bnd = epos[A["bidx"][A["f_bidx_off"][s]:A["f_bidx_off"][s + 1]]]
        pan = np.vstack([Lg[np.ix_(piv, piv)], Lg[np.ix_(bnd, piv)], np.full((1, p), np.nan)])
        pan[:p][np.triu_indices(p, 1)] = np.nan
        L[A["f_Loff"][s]:A["f_Loff"][s] + (p + b + 1) * p] = pan.ravel()
    return L


class _Emu:
    def __init__(self, lib, A, lay, L):
        self.lib, self.A, self.lay, self.L = lib, A, lay, L
        i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)
        self.tabs = [i32(A["f_p"]), i32(A["f_b"]), np.ascontiguousarray(A["f_Loff"], dtype=np.int64), i32(A["f_cmap_off"]), i32(A["cmap"]), L]
        self.max_p = int(max(A["f_p"])); self.rows = np.asarray(A["f_p"]) + np.asarray(A["f_b"])

    def walks(self, wide, rows, cols=None, break_step=False, short=0):
        """(strips Y, status, tables) of a query by k_cov_path_wide (wide) or k_cov_path"""
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        t = request_tables(self.A, self.lay, rows, cols)
        walks, steps, pairs, K, n_strip, shape = t
        if break_step:
            steps["front"][-1] = self.A["n_fronts"] + 3
        mf = int(max(self.rows[[s for s in steps["front"] if s < self.A["n_fronts"]]])) if wide else int(max(self.rows))      # the widest front of THIS query
        Z = np.full(len(walks) * 2 * mf * 6, np.nan)
        Y = np.full(n_strip, np.nan); status = np.zeros(1)
        rc = self.lib.emu_cov_walks(int(wide), int(self.A["n_fronts"]), *[ptr(x) for x in self.tabs], ptr(walks), len(walks), ptr(steps), len(steps), K, self.max_p, mf,
                                    ptr(Z), C.c_longlong(len(Z) - short), ptr(Y), C.c_longlong(n_strip), ptr(status))
        return Y, (rc, float(status[0])), t

    def block(self, rows, cols=None):
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        Y, st, (walks, steps, pairs, K, n_strip, shape) = self.walks(True, rows, cols)
        assert st == (0, 0.0)
        out = np.full(1 + shape[0] * shape[1], np.nan); out[0] = 0.0
        assert self.lib.emu_cov_gram(ptr(pairs), len(pairs), ptr(Y), C.c_longlong(n_strip), ptr(out), C.c_longlong(shape[0] * shape[1])) == 0 and out[0] == 0.0
        return out[1:].reshape(shape)


@pytest.mark.parametrize("name", ["dense_48p_150l_10x5", "dense_64p_200l", WIDE])
def test_wide_kernel_emulated_on_the_host_reproduces_the_dense_inverse(built, emu, name):
    spec = GRAPHS[name]()
    g, A, lay = _analysed(spec)
    H = _random_h(A, lay, spec, seed=5)
    S1, S2 = cpu_inverses(H)
    span = lambda n: slice(lay[n][0], lay[n][0] + lay[n][1])
    E = _Emu(emu, A, lay, _device_panels(A, H))
    sel = choose_nodes(A, lay)
    assert_contract(name, A, lay, sel)
    e = d = 0.0
    for rows, cols in ((sel, None), (sel[:4], sel[2:7])):
        M = E.block(rows, cols)
        assert np.all(np.isfinite(M))
        if cols is None:
            assert np.array_equal(M, M.T)
        eq, dq = query_errors(M, S1, S2, rows, rows if cols is None else cols, span)
        e, d = max(e, eq), max(d, dq)
    print(f"COVFACTOR host-emulated wide kernel {name}: max front {A['max_front']} e {e:.3e} d {d:.3e} bound {max(16 * d, 1e-12):.3e}")
    assert e <= max(16 * d, 1e-12), (name, e, d)
    # a step outside the tree raises the status word instead of reading there; a scratch buffer one double short is refused by the
    # launcher before anything runs (the kernel's own check of the extent: the stand-alone program of tests/cpp/cov_wide_emu.cpp)
    Y, st, _ = E.walks(True, sel[:2], None, break_step=True)
    assert st == (0, 64.0)
    Y, st, _ = E.walks(True, sel[:2], None, short=1)
    assert st == (1, 0.0) and np.all(np.isnan(Y))
    # the pivot criterion on the same panels: clean; a collapsed pivot; a NaN pivot
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    s = int(np.argmax(A["f_p"])); p = int(A["f_p"][s]); k = int(A["f_Loff"][s]) + (p - 1) * p + (p - 1)
    for value, want in ((None, 0.0), (1e-8 * E.L[k], 1.0), (np.nan, 1.0), (-1.0, 1.0)):
        L = E.L.copy(); res = np.zeros(4)
        if value is not None:
            L[k] = value
        assert emu.emu_cov_pivots(int(A["n_fronts"]), ptr(E.tabs[0]), ptr(E.tabs[2]), ptr(L), ptr(res)) == 0 and res[2] == want, (value, res)


def test_wide_kernel_writes_the_bits_of_the_wave_kernel_on_a_band_graph(built, emu):
    spec = synth.corridor(60, 14, seed=7)
    g, A, lay = _analysed(spec, mode=0)
    assert A["max_front"] <= 127
    H = _random_h(A, lay, spec, seed=9)
    E = _Emu(emu, A, lay, _device_panels(A, H))
    ids = sorted(lay)
    for rows, cols in ((ids[::5], None), ([ids[0]], [ids[-1]]), ([n for n in ids if lay[n][1] == 3], [ids[0], ids[len(ids) // 2]])):
        Yw, sw, _ = E.walks(True, rows, cols)
        Yn, sn, _ = E.walks(False, rows, cols)
        assert sw == (0, 0.0) and sn == (0, 0.0)
        assert Yw.tobytes() == Yn.tobytes()                # (the padding ahead of a path is NaN in both: never written)
        assert np.any(np.isfinite(Yw))


# ---- 4. the singular graphs of the GPU test ------------------------------------------------------------------------------------
def _front_pivot_check(spec, A, lay):
    """(flagged, smallest ratio): right-looking Cholesky of the oracle's H in elimination order; per front min / max of the pivots of L"""
    from oracle import oracle_py as O
    o = O.OracleGraph(); spec.replay(o)
    H = np.zeros((A["n_scalars"],) * 2)
    for fid, (a, b) in enumerate(spec.f_nodes):
        J, _ = o.factor_jacobian(fid, 1)
        cols = list(range(lay[int(a)][0], lay[int(a)][0] + lay[int(a)][1]))
        if b >= 0:
            cols += list(range(lay[int(b)][0], lay[int(b)][0] + lay[int(b)][1]))
        H[np.ix_(cols, cols)] += J.T @ J
    pidx = np.asarray(A["pidx"])
    M = H[np.ix_(pidx, pidx)].copy()
    n = len(M); piv = np.zeros(n)
    for k in range(n):
        piv[k] = M[k, k]
        if not piv[k] > 0:
            return True, 0.0
        col = M[k + 1:, k] / np.sqrt(piv[k])
        M[k + 1:, k + 1:] -= np.outer(col, col)
    worst = 1.0
    for s in range(A["n_fronts"]):
        l = np.sqrt(piv[int(A["f_poff"][s]):int(A["f_poff"][s]) + int(A["f_p"][s])])
        worst = min(worst, float(l.min() / l.max()))
    return worst < 1e-7, worst


def _without_priors(spec):
    keep = [k for k, (a, b) in enumerate(spec.f_nodes) if b >= 0]
    return synth.GraphSpec(name=spec.name + "_noprior", node_type=spec.node_type, node_init=spec.node_init, f_type=spec.f_type[keep], f_nodes=spec.f_nodes[keep],
                           f_meas=spec.f_meas[keep], f_sqrtinf=spec.f_sqrtinf[keep], truth=None, meta={})


SINGULAR = {"loops_64p_200l_noprior": lambda: loop_graph(64, 200, prior=False),
            "small_world_12_4_noprior": lambda: _without_priors(synth.small_world(12, 4, seed=3, obs_per_pose=4))}


@pytest.mark.parametrize("name", sorted(SINGULAR))
def test_prior_free_graphs_have_a_collapsed_pivot_in_front_order(built, name):
    spec = SINGULAR[name]()
    g, A, lay = _analysed(spec)
    flagged, worst = _front_pivot_check(spec, A, lay)
    print(f"COVFACTOR singular {name}: max front {A['max_front']} smallest pivot ratio of a front {worst:.3e} (criterion 1e-7)")
    assert flagged, (name, worst)
