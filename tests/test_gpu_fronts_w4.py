"""The 4-column form of the register-tile elimination (pps_debug_front_factor_w, width 4: what the register-only band kernels run, the
tile column a compile-time constant) on the hardware, one front at a time: the smallest shapes at which the hand-over from one tile
column's loop to the next can go wrong -- a step that ends its column exactly, with and without boundary rows behind it, a last step
that stops short, pivots in two, three and all four tile columns.  Each front is compared with numpy's Cholesky at the tolerances of
tests/test_gpu_fronts.py and, bit for bit, with the 8-column form on the same device: per entry the two forms perform the same
operations in the same order, and the 8-column kernels are the code that did not change.  tests/test_front_emu_columns.py runs the
same source on the CPU for every pivot count."""
import numpy as np
import pytest

import pop_up_slam_amd as P

pytestmark = pytest.mark.gpu

# (p, b, tile rows the band kernels pick for the front)
SHAPES = [(1, 2, 2), (4, 8, 2), (5, 8, 2), (16, 16, 2), (17, 15, 2), (13, 19, 2),
          (15, 33, 3), (12, 36, 3), (16, 32, 3), (27, 21, 3), (32, 16, 3), (33, 15, 3),
          (27, 24, 4), (47, 16, 4), (48, 15, 4), (49, 14, 4), (63, 0, 4),
          (18, 0, 2)]


def _front(p, b, seed):
    rng = np.random.default_rng(seed)
    f = p + b
    M = rng.standard_normal((f, f + 20))
    H = M @ M.T + f * np.eye(f)
    rhs = rng.standard_normal(f)
    full = np.zeros((f + 1, f + 1)); full[:f, :f] = H; full[f, :f] = rhs; full[f, f] = 7.0
    tri = np.concatenate([full[i, :i + 1] for i in range(f + 1)])
    return H, rhs, tri


@pytest.mark.parametrize("p,b,nt", SHAPES)
def test_width_4_against_numpy_and_bit_for_bit_against_width_8(built, p, b, nt):
    H, rhs, tri = _front(p, b, 100 * p + b)
    f = p + b
    L, U, bad = P.debug_front_factor(tri, p, b, tiles=nt, width=4)
    L0, U0, bad0 = P.debug_front_factor(tri, p, b, width=4)          # tiles = 0: the band kernels' choice is the tile count of the table
    assert bad == 0.0 and bad0 == 0.0
    ok = np.tril(np.ones((f + 1, p), dtype=bool))                   # (above the diagonal of L_A: unspecified)
    assert np.array_equal(L[ok], L0[ok]) and np.array_equal(U, U0)
    LA = np.linalg.cholesky(H[:p, :p])
    LB = np.linalg.solve(LA, H[p:, :p].T).T
    y = np.linalg.solve(LA, rhs[:p])
    scale = np.abs(LA).max()
    assert np.abs(np.tril(L[:p]) - LA).max() <= 1e-12 * scale
    if b:
        assert np.abs(L[p:f] - LB).max() <= 1e-12 * scale
    assert np.abs(L[f] - y).max() <= 1e-12 * max(1.0, np.abs(y).max())
    S = H[p:, p:] - LB @ LB.T
    r = rhs[p:] - LB @ y
    Ut = np.zeros((b + 1, b + 1)); Ut[np.tril_indices(b + 1)] = U
    if b:
        assert np.abs(np.tril(Ut[:b, :b]) - np.tril(S)).max() <= 1e-11 * np.abs(S).max()
        assert np.abs(Ut[b, :b] - r).max() <= 1e-11 * max(1.0, np.abs(r).max())
    L8, U8, bad8 = P.debug_front_factor(tri, p, b, tiles=nt, width=8)
    assert bad8 == 0.0
    assert np.array_equal(L[ok], L8[ok]), np.abs(L[ok] - L8[ok]).max()
    assert np.array_equal(U, U8), np.abs(U - U8).max()


def test_not_positive_definite_in_the_second_tile_column(built):
    _, _, tri = _front(20, 10, 3)
    assert P.debug_front_factor(tri, 20, 10, width=4)[2] == 0.0
    t = tri.copy(); t[17 * 18 // 2 + 17] = -1.0                      # H[17][17]: the first step of tile column 1
    assert P.debug_front_factor(t, 20, 10, width=4)[2] == 1.0


def test_width_4_arguments_no_path_takes(built):
    """the 4-column form holds neither the LDS strip nor a fifth tile row; there is no other width"""
    _, _, tri = _front(20, 50, 1)
    for kw in (dict(tiles=5), dict(tiles=4, strip=True), dict()):
        with pytest.raises(P.PpsError):
            P.debug_front_factor(tri, 20, 50, width=4, **kw)
    _, _, tri = _front(6, 10, 1)
    with pytest.raises(P.PpsError):
        P.debug_front_factor(tri, 6, 10, width=6)
