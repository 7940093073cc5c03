"""CPU: pps_cov_select -- the selected inverse on dense-front trees (csrc/pps_cov_dense.hip) -- before any kernel runs on a device.

  1. the C-ABI surface without a device: symbols, version, NULL handle, empty graph, no factor, the diagnostic's arguments, the read calls' text
  2. the recursion in the formulation and the storage of the device pass, in numpy over pps_analysis_dump alone: G = L_B L_A^-1 and
     W = L_A^-T L_A^-1 of all fronts first, then level by level from the root the gather of Sigma_BB (full b x b, ld = b, into the front's
     update-matrix slot, from the parent's panel of S and the parent's slot through cmap, its last entry ignored), Sigma_BA = -Sigma_BB G
     and Sigma_AA = W - G' Sigma_BA.  Every node's diagonal block and every factor-joined pair, read where pps_cov_marginals / _access
     look for it, against np.linalg.inv(H) at 1e-9 relative (Frobenius), the bound of tests/test_host_cov.py.  The level lists are
     checked on the way: every front on the level f_level names, every parent on a higher one.
  3. the kernel source compiled for the host (tests/cpp/cov_dense_emu.cpp: one std::thread per GPU thread, the MFMA emulation of
     tests/cpp/wave_emu.h restated for threads) on the panels of numpy's Cholesky factor in the device layout, NaN wherever the device leaves
     memory unspecified (above the diagonal of L_A, the rhs rows, S, the G scratch and the update-matrix slots before they are written):
     e <= max(16 d, 1e-12), e = |M - M0|_F / sqrt(|S0(r, r)|_F |S0(c, c)|_F) per block, d the same between np.linalg.inv and cho_solve.
     Then, on a graph of a few fronts, the same bits from two runs and the refusals: a collapsed pivot (status 1), a child map entry outside
     the parent and an update-matrix array that ends inside a front's Sigma_BB (status 64, nothing of that front written).
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pop_up_slam_amd as P
from cov_block_helpers import elimination_positions
from cov_factor_helpers import GRAPHS, WIDE
from cov_helpers import cpu_inverses, factor_pairs, locate_block, rel_err
from linsolve_helpers import spec_layout
from pop_up_slam_amd import synth
from test_host_cov_factor import _device_panels, _random_h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_RECOVERY = "no valid covariance recovery: call pps_cov_recover (a recovery ends with every change of the estimate, the measurements or the topology)"


# ---- 1. the surface ---------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound(built):
    hdr = open(os.path.join(ROOT, "include", "pps.h")).read()
    lib = C.CDLL(P.LIB_PATH)
    for name in ("pps_cov_select", "pps_debug_cov_select_form"):
        assert re.search(r"\b" + name + r"\s*\(", hdr) and name in P.SYMBOLS and getattr(lib, name) is not None
    assert P.lib().pps_version() == 305 and P.PPS_VERSION == 305      # detected by symbol lookup, not by a version bump
    assert "void select() const" in open(os.path.join(ROOT, "include", "pps_isam.hpp")).read()


def test_argument_and_state_contract_without_a_device(built):
    L = P.lib()
    assert L.pps_cov_select(None) == P.PPS_EINVAL and L.pps_debug_cov_select_form(None, 0) == P.PPS_EINVAL
    empty = P.Graph()
    with pytest.raises(P.PpsError) as e:
        empty.cov_select()
    assert e.value.code == P.PPS_ESTATE and "empty graph" in str(e.value)
    nofactor = P.Graph(); nofactor.add_pose([0, 0, 0, 0, 0, 0, 1])
    with pytest.raises(P.PpsError) as e:
        nofactor.cov_select()
    assert e.value.code == P.PPS_ENOTPD                    # (decided on the host: a graph without any factor)
    spec = synth.small_world(5, 3, seed=1)
    g = P.Graph(); nid, _ = spec.replay(g)
    a, b = int(nid[0]), int(nid[1])
    g.debug_cov_select_form(1); g.debug_cov_select_form(0)
    for form in (-1, 2):
        with pytest.raises(P.PpsError) as e:
            g.debug_cov_select_form(form)
        assert e.value.code == P.PPS_EINVAL
    reads = (lambda: g.cov_marginals([a]), lambda: g.cov_access([(a, b)]), lambda: g.cov_joint([a, b]), lambda: g.cov_block([a], [b]))
    for read in reads:
        with pytest.raises(P.PpsError) as e:
            read()
        assert e.value.code == P.PPS_ESTATE and str(e.value).endswith(NO_RECOVERY)
    for form in (0, 1):
        g.debug_cov_select_form(form)
        try:
            g.cov_select()
        except P.PpsError as err:                          # no device here: loudly, and nothing valid is left behind
            assert err.code == P.PPS_EHIP
            for read in reads:
                with pytest.raises(P.PpsError) as e:
                    read()
                assert e.value.code == P.PPS_ESTATE and "no valid covariance recovery" in str(e.value)
        else:                                              # a device: the selected inverse and the factor are both held
            assert all(np.all(np.isfinite(m)) for m in g.cov_marginals()) and np.all(np.isfinite(g.cov_block([a], [b])))


# ---- 2. the recursion as the device pass stores it ---------------------------------------------------------------------------
def _analysed(spec, mode=1):
    g = P.Graph(jacobian_mode=mode); spec.replay(g); g.analyze()
    A = g.analysis_dump()
    return g, A, spec_layout(spec, A)


def numpy_dense_pass(A, L):
    """(S, U) from the factor panels L in the device layout, by the steps of csrc/pps_cov_dense.hip; both start as NaN"""
    F = A["n_fronts"]
    S = np.full(A["L_size"], np.nan); G = np.full(A["L_size"], np.nan); U = np.full(A["U_size"], np.nan)
    panel = lambda buf, s: buf[A["f_Loff"][s]:A["f_Loff"][s] + (int(A["f_p"][s]) + int(A["f_b"][s])) * int(A["f_p"][s])].reshape(-1, int(A["f_p"][s]))
    for s in range(F):                                      # the pre-pass: L alone
        p, b = int(A["f_p"][s]), int(A["f_b"][s])
        pan = panel(L, s)
        X = np.linalg.inv(np.tril(pan[:p]))
        panel(G, s)[p:] = pan[p:] @ X
        W = X.T @ X
        panel(S, s)[:p] = np.tril(W) + np.tril(W, -1).T
    seen = np.zeros(F, dtype=bool)
    for l in range(A["n_levels"] - 1, -1, -1):              # root level first; a level reads what the levels above it wrote
        for s in (int(v) for v in A["level_fronts"][A["level_off"][l]:A["level_off"][l + 1]]):
            assert int(A["f_level"][s]) == l and not seen[s]
            seen[s] = True
            p, b = int(A["f_p"][s]), int(A["f_b"][s])
            if b == 0:
                continue
            q = int(A["f_parent"][s])
            assert 0 <= q < F and int(A["f_level"][q]) > l and seen[q]
            pq, bq = int(A["f_p"][q]), int(A["f_b"][q])
            cm = np.asarray(A["cmap"][A["f_cmap_off"][s]:A["f_cmap_off"][s + 1]])
            assert len(cm) == b + 1 and cm[b] == pq + bq and np.all(cm[:b] >= 0) and np.all(cm[:b] < pq + bq)      # the last entry: the rhs row
            assert A["f_Uoff"][s] + b * b <= (A["f_Uoff"][s + 1] if s + 1 < F else A["U_size"])
            Sq = panel(S, q); Bq = U[A["f_Uoff"][q]:A["f_Uoff"][q] + bq * bq].reshape(bq, bq)
            hi, lo = np.maximum.outer(cm[:b], cm[:b]), np.minimum.outer(cm[:b], cm[:b])
            SBB = np.where(lo < pq, Sq[hi, np.minimum(lo, pq - 1)], Bq[np.maximum(hi - pq, 0), np.maximum(lo - pq, 0)] if bq else 0.0)
            assert np.array_equal(SBB, SBB.T)                # symmetric bit for bit because its source is
            U[A["f_Uoff"][s]:A["f_Uoff"][s] + b * b] = SBB.ravel()
            Gs = panel(G, s)[p:]
            SBA = -SBB @ Gs
            panel(S, s)[p:] = SBA
            M = panel(S, s)[:p] - Gs.T @ SBA
            panel(S, s)[:p] = np.tril(M) + np.tril(M, -1).T
    assert seen.all()
    return S, U


def read_block(A, S, epos, lay, r, c):
    """Sigma(node r, node c) where pps_cov_marginals / _access look for it (csrc/pps_cov.cpp: cov_request), or None"""
    loc = locate_block(A, epos, lay, r, c)
    if loc is None:
        return None
    s, lo, le, tr = loc
    p = int(A["f_p"][s])
    pan = S[A["f_Loff"][s]:A["f_Loff"][s] + (p + int(A["f_b"][s])) * p].reshape(-1, p)
    dr, dc = lay[r][1], lay[c][1]
    return pan[lo:lo + dc, le:le + dr].T if tr else pan[lo:lo + dr, le:le + dc]


def _pairs(spec, lay):
    fp = factor_pairs([(int(a), int(b)) for a, b in spec.f_nodes])
    return [(n, n) for n in sorted(lay)] + fp + [(b, a) for a, b in fp]


@pytest.mark.parametrize("name", ["dense_48p_150l_10x5", "dense_64p_200l", "dense_100p_100l_30x8", WIDE])
def test_recursion_in_the_device_formulation_reproduces_the_dense_inverse(built, name):
    spec = GRAPHS[name]()
    g, A, lay = _analysed(spec)
    assert A["max_front"] > 127 and max(A["f_p"]) <= 64
    if name == WIDE:
        assert max(int(p) + int(b) for p, b in zip(A["f_p"], A["f_b"])) == 1290
    H = _random_h(A, lay, spec, seed=11)
    Sref = np.linalg.inv(H)
    S, U = numpy_dense_pass(A, _device_panels(A, H))
    _, epos = elimination_positions(A)
    span = lambda n: slice(lay[n][0], lay[n][0] + lay[n][1])
    worst = 0.0
    pairs = _pairs(spec, lay)
    for r, c in pairs:
        M = read_block(A, S, epos, lay, r, c)
        assert M is not None, (name, r, c, "a factor-joined pair must share a front")
        if r == c:
            assert np.array_equal(M, M.T)
        e = rel_err(M, Sref[span(r), span(c)]); worst = max(worst, e)
        assert e <= 1e-9, (name, r, c, e)
    print(f"COVSEL numpy {name}: fronts {A['n_fronts']} levels {A['n_levels']} max front {A['max_front']} blocks {len(pairs)} worst relative error {worst:.2e}")


# ---- 3. the kernel source on the host ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = tmp_path_factory.mktemp("covdense") / "libcovdenseemu.so"
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-Wno-psabi", "-I", os.path.join(ROOT, "tests", "cpp", "block_emu"),
                           "-I", os.path.join(ROOT, "pop_up_slam_amd", "csrc"), "-x", "c++", os.path.join(ROOT, "tests", "cpp", "cov_dense_emu.cpp"), "-o", str(so)])
    return C.CDLL(str(so))


def _run_emu(lib, A, L, cmap=None, n_U=None):
    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)
    i64 = lambda v: np.ascontiguousarray(v, dtype=np.int64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    tabs = [i32(A["f_p"]), i32(A["f_b"]), i64(A["f_Loff"]), i64(A["f_Uoff"]), i32(A["f_cmap_off"]), i32(A["cmap"] if cmap is None else cmap), i32(A["f_parent"]),
            i32(A["level_off"]), i32(A["level_fronts"])]
    L = np.ascontiguousarray(L)
    U = np.full(A["U_size"], np.nan); S = np.full(A["L_size"], np.nan); G = np.full(A["L_size"], np.nan); res = np.zeros(4)
    rc = lib.emu_cov_dense(int(A["n_fronts"]), int(A["n_levels"]), *[ptr(t) for t in tabs], ptr(L), ptr(U), C.c_longlong(A["U_size"] if n_U is None else n_U),
                           ptr(S), ptr(G), C.c_longlong(A["L_size"]), ptr(res))
    assert rc == 0
    return S, U, float(res[2])


EMU_GRAPHS = {"dense_48p_150l_10x5": (GRAPHS["dense_48p_150l_10x5"], 1), "dense_64p_200l": (GRAPHS["dense_64p_200l"], 1),
              "corridor_60_14": (lambda: synth.corridor(60, 14, seed=7), 0)}


@pytest.mark.parametrize("name", sorted(EMU_GRAPHS))
def test_kernels_emulated_on_the_host_reproduce_the_dense_inverse(built, emu, name):
    make, mode = EMU_GRAPHS[name]
    spec = make()
    g, A, lay = _analysed(spec, mode)
    if name == "corridor_60_14":                            # band-shaped fronts: p and b no multiples of 16
        assert A["max_front"] <= 127 and any(int(p) % 16 and int(b) % 16 for p, b in zip(A["f_p"], A["f_b"]))
    H = _random_h(A, lay, spec, seed=5)
    S1, S2 = cpu_inverses(H)
    L = _device_panels(A, H)
    S, U, status = _run_emu(emu, A, L)
    assert status == 0.0
    _, epos = elimination_positions(A)
    span = lambda n: slice(lay[n][0], lay[n][0] + lay[n][1])
    nrm = lambda M: float(np.linalg.norm(M))
    e = d = 0.0
    for r, c in _pairs(spec, lay):
        M = read_block(A, S, epos, lay, r, c)
        assert M is not None and np.all(np.isfinite(M)), (name, r, c)
        if r == c:
            assert np.array_equal(M, M.T), (name, r, "diagonal block not symmetric bit for bit")
        scale = np.sqrt(nrm(S1[span(r), span(r)]) * nrm(S1[span(c), span(c)]))
        e = max(e, nrm(M - S1[span(r), span(c)]) / scale); d = max(d, nrm(S2[span(r), span(c)] - S1[span(r), span(c)]) / scale)
    for s in range(A["n_fronts"]):                          # Sigma_BB of every front: symmetric bit for bit, nothing beyond b x b touched
        b = int(A["f_b"][s]); slot = U[A["f_Uoff"][s]:A["f_Uoff"][s] + (b + 1) ** 2]
        B = slot[:b * b].reshape(b, b)
        assert np.all(np.isfinite(B)) and np.array_equal(B, B.T) and np.all(np.isnan(slot[b * b:]))
    print(f"COVSEL host-emulated kernels {name}: fronts {A['n_fronts']} max front {A['max_front']} e {e:.3e} d {d:.3e} bound {max(16 * d, 1e-12):.3e}")
    assert e <= max(16 * d, 1e-12), (name, e, d)


def test_emulated_kernels_repeat_their_bits_and_refuse_bad_tables(built, emu):
    """on a graph of a few fronts (every run of the emulation costs seconds per hundred workgroups): two runs give the same bits; a collapsed
    pivot raises the not-positive-definite status; a child map entry outside the parent and an update-matrix array that ends inside a
    front's Sigma_BB raise kStatusInternal (64) before anything of that front is written"""
    spec = synth.small_world(5, 3, seed=1)
    g, A, lay = _analysed(spec, 0)
    assert A["n_fronts"] >= 2 and max(A["f_b"]) >= 2
    L = _device_panels(A, _random_h(A, lay, spec, seed=3))
    S, U, status = _run_emu(emu, A, L)
    assert status == 0.0 and np.any(np.isfinite(S))
    S_again, U_again, _ = _run_emu(emu, A, L)
    assert S_again.tobytes() == S.tobytes() and U_again.tobytes() == U.tobytes()
    s = int(np.argmax(A["f_p"])); p = int(A["f_p"][s]); k = int(A["f_Loff"][s]) + (p - 1) * p + (p - 1)
    Lbad = L.copy(); Lbad[k] *= 1e-8
    assert _run_emu(emu, A, Lbad)[2] == 1.0
    s = int(np.argmax(A["f_b"])); b = int(A["f_b"][s]); q = int(A["f_parent"][s])
    cm = np.array(A["cmap"]).copy(); cm[A["f_cmap_off"][s] + b // 2] = int(A["f_p"][q]) + int(A["f_b"][q]) + 2
    _, Ubad, status = _run_emu(emu, A, L, cmap=cm)
    assert status == 64.0 and np.all(np.isnan(Ubad[A["f_Uoff"][s]:A["f_Uoff"][s] + b * b]))
    end, t = max((int(A["f_Uoff"][t]) + int(A["f_b"][t]) ** 2, t) for t in range(A["n_fronts"]) if A["f_b"][t] > 0)
    _, Ubad, status = _run_emu(emu, A, L, n_U=end - 1)
    assert status == 64.0 and np.all(np.isnan(Ubad[A["f_Uoff"][t]:A["f_Uoff"][t] + int(A["f_b"][t]) ** 2]))
