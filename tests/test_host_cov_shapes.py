"""CPU: the table of tests/cov_shape_helpers.py before any of it costs GPU time, and the covariance kernels' source on the host at every
shape of that table.

  1. every contract line is claimed by an entry, and every entry meets the lines it claims (from pps_analysis_dump alone); the node set
     of the pps_cov_block queries has the roles it is chosen for; pattern_pairs finds every pair where the read calls look for it
     (cov_helpers.locate_block) and nothing else
  2. longdouble_inverse against a 40-digit mpmath inverse at n = 36 (1e-18 relative), and against np.linalg.inv at the sizes of the table
  3. the host emulations of the kernels (tests/cpp/cov_emu.cpp, cov_block_emu.cpp, cov_dense_emu.cpp, cov_wide_emu.cpp: one std::thread
     per GPU thread) over the whole table, on the panels of a dense Cholesky factor of a random positive definite H of the graph's
     sparsity, NaN wherever the device leaves memory unspecified.  The level pass and the dense-front pass: EVERY entry of every front
     -- [S_AA; S_BA] and S_BB, fill included -- against longdouble_inverse at 1e-9 relative per front, the tolerance of
     tests/test_host_cov.py.  The path walks: the joint of the role nodes and rows x cols both ways, e <= max(16 d, 1e-12) with d
     = np.linalg.inv against the reference; on band entries the wide walk writes the bits of the wave walk.
     No entry is left to the GPU alone: the largest (dense_72p_400l_8x6, fronts of 264 rows) takes about ten seconds in the dense pass.
"""
import ctypes as C
import os
import subprocess
import time

import numpy as np
import pytest

import cov_shape_helpers as H
from cov_block_helpers import elimination_positions, request_tables
from cov_helpers import locate_block, rel_err
from test_host_cov_factor import _Emu, _device_panels, _random_h
from test_host_cov_factor import emu as wide_emu            # noqa: F401  (module-scoped fixtures: the build lines of those files)
from test_host_cov_select import _run_emu, read_block
from test_host_cov_select import emu as dense_emu           # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the contracts --------------------------------------------------------------------------------------------------------
def test_every_contract_line_is_claimed_by_an_entry():
    assert H.uncovered_lines() == ([], [])
    assert H.BAND and H.DENSE and all(H.TABLE[n][2] for n in H.BAND) and all(H.TABLE[n][3] for n in H.DENSE)


@pytest.mark.parametrize("name", list(H.TABLE))
def test_entry_meets_its_contract(built, name):
    g, spec, A, lay = H.analysed(name)
    f, sel, pairs, fill = H.assert_entry(name, A, lay, spec)
    assert len(set(sel)) == len(sel) and len(sel) <= 13
    roles = H.roles_present(A, lay, sel)
    if len(f["fronts"]) > 1:
        assert len(sel) >= 7 and all(roles.values()), (name, roles)
    # the pattern: exactly the pairs the look-up of csrc/pps_cov.cpp (restated in cov_helpers.locate_block) finds
    _, epos = elimination_positions(A)
    ids = sorted(lay)
    found = {(r, c) for r in ids for c in ids if r != c and locate_block(A, epos, lay, r, c) is not None}
    assert found == set(pairs), (name, len(found), len(pairs))
    assert set(fill) <= set(pairs) and all((c, r) in set(pairs) for r, c in pairs)
    print(f"COVSHAPE contract {name}: scalars {f['n_scalars']} fronts {len(f['fronts'])} max front {f['max_front']} pairs {len(pairs)} of them no factor joins "
          f"{len(fill)} nodes of the block queries {sel} shapes {sorted(set(f['fronts']), reverse=True)}")


# ---- 2. the reference --------------------------------------------------------------------------------------------------------
def _spd(n, seed):
    rng = np.random.default_rng(seed)
    J = rng.normal(size=(2 * n, n)) * np.where(rng.random((2 * n, n)) < 0.2, 1.0, 0.0)
    return J.T @ J + 1e-3 * np.eye(n)


def test_longdouble_inverse_against_forty_digits():
    if not H.have_long_double():
        pytest.skip("np.longdouble is no wider than float64 here")
    import mpmath
    assert np.finfo(np.longdouble).nmant >= 63
    Hm = _spd(36, 1)
    S = H.longdouble_inverse(Hm)
    hi = S.astype(np.float64); lo = (S - hi.astype(np.longdouble)).astype(np.float64)      # S = hi + lo exactly
    with mpmath.workdps(40):
        R = mpmath.matrix(Hm.tolist()) ** -1
        diff = max(abs(mpmath.mpf(float(hi[i, j])) + mpmath.mpf(float(lo[i, j])) - R[i, j]) for i in range(36) for j in range(36))
        scale = max(abs(R[i, j]) for i in range(36) for j in range(36))
        rel = float(diff / scale)
    print(f"COVSHAPE longdouble_inverse n 36: {rel:.2e} of the largest entry from the 40-digit inverse, cond {np.linalg.cond(Hm):.2e}")
    assert rel <= 1e-18


@pytest.mark.parametrize("n", [180, 318])
def test_longdouble_inverse_against_numpy_at_the_sizes_of_the_table(n):
    Hm = _spd(n, n)
    t0 = time.perf_counter()
    S = H.longdouble_inverse(Hm)
    dt = time.perf_counter() - t0
    S1 = np.linalg.inv(Hm)
    rel = float(np.linalg.norm(S1 - S) / np.linalg.norm(S))
    cond = float(np.linalg.cond(Hm))
    print(f"COVSHAPE longdouble_inverse n {n}: {dt:.2f} s, np.linalg.inv at {rel:.2e} relative (Frobenius), cond {cond:.2e}")
    assert S.dtype == np.longdouble
    assert rel <= cond * np.finfo(np.float64).eps                      # float64's inverse: within cond * eps of the reference
    assert float(np.linalg.norm(Hm @ S.astype(np.float64) - np.eye(n))) <= 64 * n * cond * np.finfo(np.float64).eps


# ---- 3. the kernel source on the host ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def level_emus(tmp_path_factory):
    """cov_emu.cpp (k_cov_level) and cov_block_emu.cpp (k_cov_path, k_cov_gram) with the build line of their tests"""
    out = {}
    d = tmp_path_factory.mktemp("covshapes")
    for src in ("cov_emu", "cov_block_emu"):
        so = d / f"lib{src}.so"
        subprocess.check_call(["g++", "-std=c++20", "-O1", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-I", os.path.join(ROOT, "tests", "cpp", "block_emu"),
                               "-I", os.path.join(ROOT, "pop_up_slam_amd", "csrc"), "-x", "c++", os.path.join(ROOT, "tests", "cpp", src + ".cpp"), "-o", str(so)])
        out[src] = C.CDLL(str(so))
    return out


_SETUP = {}


def _setup(name):
    """(A, lay, spec, H, its reference inverse, np.linalg.inv, device panels, role nodes) of an entry, computed once"""
    if name not in _SETUP:
        g, spec, A, lay = H.analysed(name)
        _, sel, pairs, fill = H.assert_entry(name, A, lay, spec)
        Hm = _random_h(A, lay, spec, seed=5)
        _SETUP[name] = (A, lay, spec, Hm, H.longdouble_inverse(Hm), np.linalg.inv(Hm), _device_panels(A, Hm), sel, pairs, fill)
    return _SETUP[name]


def _front_rows(A, s):
    p, b, po = int(A["f_p"][s]), int(A["f_b"][s]), int(A["f_poff"][s])
    return p, b, np.asarray(A["pidx"][po:po + p]), np.asarray(A["bidx"][A["f_bidx_off"][s]:A["f_bidx_off"][s + 1]])


def _check_every_front(name, A, S, U, Sref):
    """every entry the pass writes: [S_AA; S_BA] in the panel, S_BB in the update-matrix slot; returns the worst relative error of a front"""
    worst = 0.0
    for s in range(A["n_fronts"]):
        p, b, ip, ib = _front_rows(A, s)
        pan = S[A["f_Loff"][s]:A["f_Loff"][s] + (p + b) * p].reshape(p + b, p)
        assert np.all(np.isfinite(pan)), (name, s, p, b)
        assert np.array_equal(pan[:p], pan[:p].T), (name, s, "S_AA not symmetric bit for bit")
        parts = [("S_AA", pan[:p], Sref[np.ix_(ip, ip)])]
        if b:
            B = U[A["f_Uoff"][s]:A["f_Uoff"][s] + b * b].reshape(b, b)
            assert np.array_equal(B, B.T), (name, s, "S_BB not symmetric bit for bit")
            parts += [("S_BA", pan[p:], Sref[np.ix_(ib, ip)]), ("S_BB", B, Sref[np.ix_(ib, ib)])]
        for what, got, ref in parts:
            e = rel_err(got, ref); worst = max(worst, e)
            assert e <= 1e-9, (name, "front", s, (p, b), what, e)
    return worst


def _check_pattern(name, A, lay, S, Sref, pairs):
    """every pair of the pattern where pps_cov_access reads it, at the same tolerance against the reference's diagonal blocks"""
    _, epos = elimination_positions(A)
    span = lambda n: slice(lay[n][0], lay[n][0] + lay[n][1])
    blocks = []
    for r, c in pairs:
        M = read_block(A, S, epos, lay, r, c)
        assert M is not None, (name, r, c)
        blocks.append((r, c, M))
    return blocks, span


@pytest.mark.parametrize("name", H.BAND)
def test_level_pass_on_the_host_every_entry_of_every_front(built, level_emus, name):
    A, lay, spec, Hm, Sref, S1, L, sel, pairs, fill = _setup(name)
    lib = level_emus["cov_emu"]
    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)
    i64 = lambda v: np.ascontiguousarray(v, dtype=np.int64)
    U = np.full(A["U_size"], np.nan); S = np.full(A["L_size"], np.nan)
    arrs = [i32(A["level_off"]), i32(A["level_fronts"]), i32(A["f_p"]), i32(A["f_b"]), i64(A["f_Loff"]), i64(A["f_Uoff"]), i32(A["f_cmap_off"]), i32(A["cmap"]),
            i32(A["f_parent"]), np.ascontiguousarray(L), U, S, np.zeros(4)]
    t0 = time.perf_counter()
    lib.emu_cov(int(A["n_fronts"]), int(A["n_levels"]), *[a.ctypes.data_as(C.c_void_p) for a in arrs])
    dt = time.perf_counter() - t0
    assert arrs[-1][2] == 0.0
    worst = _check_every_front(name, A, S, U, Sref)
    blocks, span = _check_pattern(name, A, lay, S, Sref, pairs)
    e, d = H.block_errors(blocks, Sref, S1, span) if blocks else (0.0, 0.0)
    print(f"COVSHAPE host k_cov_level {name}: fronts {A['n_fronts']} worst front {worst:.2e} pattern pairs {len(pairs)} (no factor: {len(fill)}) e {e:.2e} d {d:.2e}, {dt:.2f} s")
    assert e <= 1e-9, (name, e)


@pytest.mark.parametrize("name", list(H.TABLE))
def test_dense_front_pass_on_the_host_every_entry_of_every_front(built, dense_emu, name):
    A, lay, spec, Hm, Sref, S1, L, sel, pairs, fill = _setup(name)
    t0 = time.perf_counter()
    S, U, status = _run_emu(dense_emu, A, L)
    dt = time.perf_counter() - t0
    assert status == 0.0
    worst = _check_every_front(name, A, S, U, Sref)
    for s in range(A["n_fronts"]):                          # nothing beyond b x b of a slot is touched
        b = int(A["f_b"][s])
        assert np.all(np.isnan(U[A["f_Uoff"][s] + b * b:A["f_Uoff"][s] + (b + 1) ** 2])), (name, s)
    blocks, span = _check_pattern(name, A, lay, S, Sref, pairs)
    e, d = H.block_errors(blocks, Sref, S1, span) if blocks else (0.0, 0.0)
    print(f"COVSHAPE host dense-front pass {name}: fronts {A['n_fronts']} worst front {worst:.2e} pattern pairs {len(pairs)} (no factor: {len(fill)}) e {e:.2e} d {d:.2e}, {dt:.2f} s")
    assert e <= 1e-9, (name, e)


def _queries(sel):
    half = max(1, len(sel) // 2)
    return [(sel, None), (sel[:half], sel[half - 1:] if len(sel) > 1 else sel)]


@pytest.mark.parametrize("name", list(H.TABLE))
def test_path_walks_on_the_host_at_the_role_nodes(built, level_emus, wide_emu, name):
    A, lay, spec, Hm, Sref, S1, L, sel, pairs, fill = _setup(name)
    span = lambda n: slice(lay[n][0], lay[n][0] + lay[n][1])
    E = _Emu(wide_emu, A, lay, L)
    band = name in H.BAND
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)

    def narrow(rows, cols):                                 # k_cov_path + k_cov_gram through cov_block_emu.cpp
        walks, steps, prs, K, n_strip, shape = request_tables(A, lay, rows, cols)
        Y = np.full(n_strip, np.nan); out = np.full(1 + shape[0] * shape[1], np.nan); out[0] = 0.0
        rc = level_emus["cov_block_emu"].emu_cov_block(int(A["n_fronts"]), *[ptr(t) for t in E.tabs], ptr(walks), len(walks), ptr(steps), len(steps), K, E.max_p,
                                                       int(max(E.rows)), ptr(Y), C.c_longlong(n_strip), ptr(prs), len(prs), ptr(out), C.c_longlong(shape[0] * shape[1]))
        assert rc == 0 and out[0] == 0.0, (name, rc, out[0])
        return out[1:].reshape(shape)

    e = d = 0.0
    n_blocks = 0
    for rows, cols in _queries(sel):
        M = E.block(rows, cols)
        assert np.all(np.isfinite(M)), name
        if cols is None:
            assert np.array_equal(M, M.T), (name, "joint not symmetric bit for bit")
            blocks = H.split_block(M, rows, rows, lay)
        else:
            assert np.array_equal(E.block(cols, rows), M.T), (name, "Sigma(r, c) is not the transpose of Sigma(c, r) bit for bit")
            blocks = H.split_block(M, rows, cols, lay)
        if band:                                            # the wave walk: the same strips, the same blocks
            Yw, sw, _ = E.walks(True, rows, cols); Yn, sn, _ = E.walks(False, rows, cols)
            assert sw == (0, 0.0) and sn == (0, 0.0) and Yw.tobytes() == Yn.tobytes(), name
            assert narrow(rows, cols).tobytes() == M.tobytes(), name
        eq, dq = H.block_errors(blocks, Sref, S1, span)
        e, d = max(e, eq) if eq == eq else eq, max(d, dq); n_blocks += len(blocks)
    print(f"COVSHAPE host path walks {name}: nodes {sel} blocks {n_blocks} e {e:.3e} d {d:.3e} bound {max(16 * d, 1e-12):.3e}" + (" (wave walk: the same bits)" if band else ""))
    assert e <= max(16 * d, 1e-12), (name, e, d)
