"""CPU: what the loop gate added to the device functions the Mahalanobis gate kernels share (csrc/pps_gate_dev.h), compiled for the host
without multiply-add contraction (tests/cpp/gate_dev_m6_host.cpp), the way tests/test_host_gate_dev.py pins their siblings:
  strip_gram<6, 6, 6>   against a plain restatement of the stated operation order (numpy float64 scalars, one IEEE operation per Python
                        operation, so equality is exact) and, within max(16 d, 1e-12), the dense numpy product (d = numpy's own error
                        against an np.longdouble evaluation, as in tests/test_host_gate_dev.py)
  strip_gram<3, 3, 3>   against strip_gram3<3, 3> on the same inputs, bit for bit
  common_root_pivots    against the common suffix of the two root paths (tests/cov_block_helpers.py) on random forests: same front, one front
                        an ancestor of the other, disjoint subtrees, no common root; and its refusals of a table that points outside itself."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
NAN = float("nan")
LENS = [6, 12, 63, 64, 65, 130]


@pytest.fixture(scope="module")
def dev(tmp_path_factory):
    so = tmp_path_factory.mktemp("gate_dev_m6") / "libgatedevm6.so"
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-Wno-attributes", "-Wno-unknown-pragmas",
                           "-I", os.path.join(ROOT, "tests", "cpp", "block_emu"), "-I", os.path.join(ROOT, "pop_up_slam_amd", "csrc"), "-x", "c++",
                           os.path.join(ROOT, "tests", "cpp", "gate_dev_m6_host.cpp"), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.gate_dev_strip_gram6.restype = None
    lib.gate_dev_strip_gram6.argtypes = [_dp, _dp, _dp, C.c_int, C.c_int, C.c_int, C.c_int, _dp]
    lib.gate_dev_strip_gram33.restype = None
    lib.gate_dev_strip_gram33.argtypes = [C.c_int, _dp, _dp, _dp, _dp, C.c_int, C.c_int, C.c_int, C.c_int, _dp]
    lib.gate_dev_common_root_pivots.restype = C.c_int
    lib.gate_dev_common_root_pivots.argtypes = [_ip, _ip, C.c_int, C.c_int, C.c_int, _ip]
    return lib


def _c(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def gram6(dev, J, Ya, Yb, len_a, len_b, common, K):
    J, Ya, Yb = _c(J), _c(Ya), _c(Yb)
    s = np.full(21, 123.0)
    dev.gate_dev_strip_gram6(J.ctypes.data_as(_dp), Ya.ctypes.data_as(_dp), Yb.ctypes.data_as(_dp), len_a, len_b, common, K, s.ctypes.data_as(_dp))
    return s


def gram_lanes(M, Ja, Jb, Ya, Yb, len_a, len_b, common, K):
    """the stated order: lane `lane` takes the rows K - 1 - j, j = lane, lane + 64, ...; per row z_a = Ja y_a and z_b = Jb y_b (columns
    ascending, from 0.0), rows of common ancestors add (z_a + z_b)(z_a + z_b)' with the sum BEFORE the product, all other rows
    z_a z_a' + z_b z_b'; then the 64 partial sums of an entry in lane order from 0.0.  All Python floats."""
    Ja, Jb, Ya, Yb = (np.asarray(x).tolist() for x in (Ja, Jb, Ya, Yb))
    E = M * (M + 1) // 2
    ln = max(len_a, len_b)
    part = [[0.0] * 64 for _ in range(E)]
    for lane in range(64):
        s = [0.0] * E
        for j in range(lane, ln, 64):
            k = K - 1 - j
            za, zb = [0.0] * M, [0.0] * M
            for z, Jm, Y, n in ((za, Ja, Ya, len_a), (zb, Jb, Yb, len_b)):
                if j < n:
                    y = Y[k]
                    for i in range(M):
                        t = 0.0
                        for q in range(len(y)):
                            t += Jm[i][q] * y[q]
                        z[i] = t
            zs = [za[i] + zb[i] for i in range(M)]
            e = 0
            for i in range(M):
                for jj in range(i + 1):
                    s[e] += zs[i] * zs[jj] if j < common else za[i] * za[jj] + zb[i] * zb[jj]
                    e += 1
        for e in range(E):
            part[e][lane] = s[e]
    out = []
    for e in range(E):
        t = 0.0
        for k in range(64):
            t += part[e][k]
        out.append(t)
    return np.array(out)


def _dense(J, Ya, Yb, len_a, len_b, common, K, dtype):
    Ja, Jb = J[:, :6].astype(dtype), J[:, 6:].astype(dtype)
    A, B = Ya[K - len_a:].astype(dtype), Yb[K - len_b:].astype(dtype)      # the valid rows
    S = Ja @ (A.T @ A) @ Ja.T + Jb @ (B.T @ B) @ Jb.T
    if common:
        Sab = A[len_a - common:].T @ B[len_b - common:]                     # the common suffix
        S = S + Ja @ Sab @ Jb.T + Jb @ Sab.T @ Ja.T
    return S[np.tril_indices(6)]                                            # (row-major lower triangle: (0,0) (1,0) (1,1) (2,0) ...)


def test_strip_gram6_bits_end_alignment_and_the_dense_product(dev):
    rng = np.random.default_rng(66)
    worst, n = 0.0, 0
    for len_a in LENS:
        for len_b in LENS:
            J = rng.standard_normal((6, 12))
            ya, yb = rng.standard_normal((len_a, 6)), rng.standard_normal((len_b, 6))
            Kmax = max(len_a, len_b)
            for common in sorted({0, 6, min(len_a, len_b)}):                # none, part, all of the shorter
                got = []
                for K in (Kmax, Kmax + 7):
                    # end-aligned strips; the rows ahead of the valid ones hold NaN and must not be read into the result
                    Ya = np.full((K, 6), NAN); Ya[K - len_a:] = ya
                    Yb = np.full((K, 6), NAN); Yb[K - len_b:] = yb
                    s = gram6(dev, J, Ya, Yb, len_a, len_b, common, K)
                    assert np.all(np.isfinite(s))
                    got.append(s)
                    if K == Kmax:
                        assert np.array_equal(s, gram_lanes(6, J[:, :6], J[:, 6:], Ya, Yb, len_a, len_b, common, K)), (len_a, len_b, common)
                        ref = _dense(J, Ya, Yb, len_a, len_b, common, K, np.float64)
                        ext = _dense(J, Ya, Yb, len_a, len_b, common, K, np.longdouble)
                        d = float(np.linalg.norm(ref - ext) / np.linalg.norm(ext))
                        e = float(np.linalg.norm(s - ref) / np.linalg.norm(ref))
                        worst = max(worst, e / max(16 * d, 1e-12)); n += 1
                        assert e <= max(16 * d, 1e-12), (len_a, len_b, common, e, d)
                assert np.array_equal(got[0], got[1])                       # the sums do not depend on K
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps
    print(f"GATE_DEV strip_gram<6,6,6>: {n} cases, worst error / bound {worst:.3e}")


def test_nearly_cancelling_common_rows_are_summed_before_they_are_multiplied(dev):
    """J_b = -J_a and y_b = y_a (1 + 1e-9) on the common rows: (z_a + z_b) is 1e-9 |z_a|, its square 1e-18 |z_a|^2 -- multiplied out the
    four products would leave rounding of the size 1e-16 |z_a|^2, a hundred times the result.  Against np.longdouble."""
    rng = np.random.default_rng(5)
    n = 70
    Ja = rng.standard_normal((6, 6)); J = np.hstack([Ja, -Ja])
    ya = rng.standard_normal((n, 6)); yb = ya * (1.0 + 1e-9)
    s = gram6(dev, J, ya, yb, n, n, n, n)
    z = (Ja.astype(np.longdouble) @ ya.T.astype(np.longdouble)) - (Ja.astype(np.longdouble) @ yb.T.astype(np.longdouble))
    ext = (z @ z.T)[np.tril_indices(6)]
    e = float(np.max(np.abs(s - ext)) / np.max(np.abs(ext)))
    print(f"GATE_DEV strip_gram<6,6,6> cancelling rows: error {e:.3e} of entries of size {float(np.max(np.abs(ext))):.3e}")
    assert e <= 1e-6, e      # z_a + z_b carries the relative rounding 1e-16 / 1e-9 = 1e-7 of a difference of neighbours; its square twice that


def test_strip_gram_m3_equals_strip_gram3(dev):
    rng = np.random.default_rng(33)
    n = 0
    for len_a in (3, 6, 63, 64, 65, 130):
        for len_b in (3, 64, 65, 130):
            Ja, Jb = _c(rng.standard_normal((3, 3))), _c(rng.standard_normal((3, 3)))
            K = max(len_a, len_b) + 2
            Ya = _c(np.full((K, 3), NAN)); Ya[K - len_a:] = rng.standard_normal((len_a, 3))
            Yb = _c(np.full((K, 3), NAN)); Yb[K - len_b:] = rng.standard_normal((len_b, 3))
            for common in sorted({0, 3, min(len_a, len_b)}):
                out = []
                for generic in (1, 0):
                    s = np.full(6, 123.0)
                    dev.gate_dev_strip_gram33(generic, *[x.ctypes.data_as(_dp) for x in (Ja, Jb, Ya, Yb)], len_a, len_b, common, K, s.ctypes.data_as(_dp))
                    out.append(s)
                assert np.all(np.isfinite(out[0])) and np.array_equal(out[0], out[1]), (len_a, len_b, common)
                assert np.array_equal(out[0], gram_lanes(3, Ja, Jb, Ya, Yb, len_a, len_b, common, K))
                n += 1
    assert n == 6 * 4 * 3 - 9      # (the nine shapes with a strip of 3 rows: common 3 IS the shorter strip)


def _forest(rng, n_fronts, n_roots):
    """fronts numbered children first (a parent has the larger index), the last n_roots fronts are roots; 1 .. 7 pivots each"""
    parent = np.array([int(rng.integers(s + 1, n_fronts)) if s < n_fronts - n_roots else -1 for s in range(n_fronts)], dtype=np.int32)
    p = rng.integers(1, 8, n_fronts)
    rootlen = np.zeros(n_fronts, dtype=np.int32)
    for s in range(n_fronts - 1, -1, -1):
        rootlen[s] = p[s] + (rootlen[parent[s]] if parent[s] >= 0 else 0)
    return parent, p, rootlen


def _path(parent, s):
    out = []
    while s >= 0:
        out.append(int(s)); s = int(parent[s])
    return out


def test_common_root_pivots_on_random_forests(dev):
    rng = np.random.default_rng(12)
    seen = {"same": 0, "nested": 0, "apart": 0, "no_root": 0}
    for n_fronts, n_roots in ((1, 1), (2, 2), (9, 1), (40, 1), (40, 3)):
        parent, p, rootlen = _forest(rng, n_fronts, n_roots)
        for fa in range(n_fronts):
            for fb in range(n_fronts):
                pa, pb = _path(parent, fa), _path(parent, fb)
                want = 0
                for x, y in zip(reversed(pa), reversed(pb)):
                    if x != y:
                        break
                    want += int(p[x])
                got = C.c_int(-7)
                assert dev.gate_dev_common_root_pivots(parent.ctypes.data_as(_ip), rootlen.ctypes.data_as(_ip), n_fronts, fa, fb, C.byref(got)) == 1
                assert got.value == want, (n_fronts, fa, fb)
                seen["same" if fa == fb else "nested" if (fa in pb or fb in pa) else "apart" if want else "no_root"] += 1
    assert all(seen.values()), seen


def test_common_root_pivots_refuses_a_table_that_leaves_the_tree(dev):
    rootlen = np.array([5, 4, 2], dtype=np.int32)
    got = C.c_int(-7)
    for parent in ([2, 7, -1], [2, -3, -1], [1, 0, -1]):                    # past the table, below -1, a cycle (ended by the hop count)
        par = np.array(parent, dtype=np.int32)
        rl = np.array([3, 3, 2], dtype=np.int32) if parent == [1, 0, -1] else rootlen
        assert dev.gate_dev_common_root_pivots(par.ctypes.data_as(_ip), rl.ctypes.data_as(_ip), 3, 0, 1, C.byref(got)) == 0 and got.value == 0
