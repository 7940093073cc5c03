"""The 4-column form of the register-tile elimination with its first panel read straight from the assembled triangle, on the hardware.

One front at a time (pps_debug_front_factor_w): width 4 -- the K = 0 step takes columns 0 .. 3 of row `lane` from the LDS triangle, ahead
of the tile reads, with no extraction and no read-back -- against width 8, the general loop, on the same device, bit for bit (-0.0 and
+0.0 differ), at the shapes where the new step can go wrong: fronts that end inside the first panel, at its end, one pivot into the next
panel and into the next tile column; no boundary rows, one, eighteen; fronts at the edges of the tile counts; a boundary row whose entries
are signed zeros.  Compared: every entry of the stored factor panel that a form computes (the entries above the diagonal of a column's own
diagonal tile included -- in the first panel they are what the tile load finds in the next rows of the triangle; rows of the tile rows above
a column's tile column hold what an earlier panel left in the panel buffer, in either form), the update matrix with its rhs row, the flag.

Then two small trees through the whole-tree factor launch (k_band_factor_all) against the launch-per-stage schedule, bit for bit: the
smallest corridor with a group crossing and a graph with leaves of more than sixteen pivots (tests/test_gpu_assembly_batches.py builds
both).  tests/test_front_emu_first_panel.py runs the same source on the CPU at every pivot count."""
import numpy as np
import pytest

import pop_up_slam_amd as P
from pop_up_slam_amd import synth

pytestmark = pytest.mark.gpu

PS = (1, 2, 3, 4, 5, 6, 7, 9, 15, 17, 18)
BS = (0, 1, 18)
# p + b + 1 = 33 / 34 (two tile rows / three), 49 / 50 (three / four), 63: (p, b)
EDGES = [(15, 17), (15, 18), (6, 26), (6, 27), (18, 14), (18, 15), (15, 33), (15, 34), (27, 21), (27, 22), (9, 39), (9, 40), (18, 44), (3, 59), (17, 45)]


def _front(p, b, seed):
    rng = np.random.default_rng(seed)
    f = p + b
    M = rng.standard_normal((f, f + 20))
    H = M @ M.T + f * np.eye(f)
    rhs = rng.standard_normal(f)
    full = np.zeros((f + 1, f + 1)); full[:f, :f] = H; full[f, :f] = rhs; full[f, f] = 7.0
    tri = np.concatenate([full[i, :i + 1] for i in range(f + 1)])
    return H, rhs, tri


def _tile_counts(p, b):
    fa = p + b + 1
    return range(2 if fa <= 33 else 3 if fa <= 49 else 4, 5)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _computed(p, b):
    rows, cols = np.indices((p + b + 1, p))
    return rows >= 16 * (cols // 16)


def _same_in_both_widths(tri, p, b, tiles):
    L4, U4, bad4 = P.debug_front_factor(tri, p, b, tiles=tiles, width=4)
    L8, U8, bad8 = P.debug_front_factor(tri, p, b, tiles=tiles, width=8)
    ok = _computed(p, b)
    assert bad4 == bad8, (p, b, tiles)
    assert np.array_equal(_bits(L4)[ok], _bits(L8)[ok]), (p, b, tiles, np.argwhere((_bits(L4) != _bits(L8)) & ok)[:4])
    assert np.array_equal(_bits(U4), _bits(U8)), (p, b, tiles, np.flatnonzero(_bits(U4) != _bits(U8))[:4])
    return L4, U4, bad4


def _against_numpy(H, rhs, p, b, L, U):
    f = p + b
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


@pytest.mark.parametrize("p", PS)
def test_fronts_that_end_in_or_just_behind_the_first_panel(built, p):
    for b in BS:
        H, rhs, tri = _front(p, b, 1000 + 100 * p + b)
        for tiles in _tile_counts(p, b):
            L, U, bad = _same_in_both_widths(tri, p, b, tiles)
            assert bad == 0.0
            _against_numpy(H, rhs, p, b, L, U)


@pytest.mark.parametrize("p,b", EDGES)
def test_fronts_at_the_tile_count_edges(built, p, b):
    assert p + b + 1 in (33, 34, 49, 50, 63)
    H, rhs, tri = _front(p, b, 2000 + 100 * p + b)
    for tiles in _tile_counts(p, b):
        L, U, bad = _same_in_both_widths(tri, p, b, tiles)
        assert bad == 0.0
        _against_numpy(H, rhs, p, b, L, U)


@pytest.mark.parametrize("zero", [-0.0, 0.0])
def test_signed_zeros_in_the_boundary_block(built, zero):
    """a boundary row that no pivot touches: its entries against the other boundary rows and its rhs entry only ever meet zero products,
    whose signs decide theirs"""
    for p, b in [(2, 3), (3, 18), (6, 18), (9, 18), (15, 18), (18, 18)]:
        _, _, tri = _front(p, b, 31 * p + b)
        f = p + b
        j = p + 1
        t = tri.copy()
        t[j * (j + 1) // 2:j * (j + 1) // 2 + j] = zero
        for i in range(j + 1, f):
            t[i * (i + 1) // 2 + j] = zero
        t[f * (f + 1) // 2 + j] = zero
        for tiles in _tile_counts(p, b):
            _, U, bad = _same_in_both_widths(t, p, b, tiles)
            assert bad == 0.0
            Ut = np.zeros((b + 1, b + 1)); Ut[np.tril_indices(b + 1)] = U
            assert Ut[1, 0] == 0.0 and Ut[b, 1] == 0.0 and (Ut[2:b, 1] == 0.0).all()


def test_not_positive_definite_flag_for_the_pivots_that_exist(built):
    for p, b in [(1, 4), (2, 4), (3, 4), (4, 4), (6, 18), (9, 18), (15, 18), (18, 18)]:
        _, _, tri = _front(p, b, 5 * p + b)
        diag = lambda i: i * (i + 1) // 2 + i
        for i, want in ((0, 1.0), (p - 1, 1.0), (p, 0.0)):          # first, last existing, first masked pivot
            t = tri.copy(); t[diag(i)] = -1e6
            assert P.debug_front_factor(t, p, b, width=4)[2] == want, (p, b, i)
        t = tri.copy(); t[diag(p)] = -1e6
        _same_in_both_widths(t, p, b, 0)


TREES = {
    "corridor_24_6": lambda: synth.corridor(24, 6, seed=1),              # the smallest tree with a group crossing
    "small_world_20_6_8": lambda: synth.small_world(20, 6, 8, seed=1),   # leaves of p = 24
}


def _steps(make):
    g = P.Graph()
    make().replay(g)
    out = []
    for lam in (0.0, 1e-3):
        d, _, form, bad = g.debug_solve(lam)
        assert bad == 0.0
        out.append((d.copy(), form))
    d, d2, form, bad = g.debug_solve(1e-3, 1e-2)
    assert bad == 0.0
    out.append((np.concatenate([d, d2]), form))
    g.analyze()
    A = g.analysis_dump()
    g.close()
    return out, A


@pytest.mark.parametrize("name", list(TREES))
def test_whole_tree_launch_has_the_bits_of_the_launch_per_stage_schedule(built, monkeypatch, name):
    """(a handle reads PPS_PLAIN_SCHEDULE once, when it is created: 4 = one launch per band stage, the plain walk)"""
    whole, A = _steps(TREES[name])
    monkeypatch.setenv("PPS_PLAIN_SCHEDULE", "4")
    plain, _ = _steps(TREES[name])
    assert A["max_front"] <= 64 and A["n_stages"] >= 2
    if name == "small_world_20_6_8":
        leaves = np.setdiff1d(np.arange(A["n_fronts"]), A["f_parent"][A["f_parent"] >= 0])
        assert (A["f_p"][leaves] > 16).any()
    for (dw, fw), (dp, fp) in zip(whole, plain):
        assert fw == 1 and fp == 0, (fw, fp)
        assert np.isfinite(dw).all() and np.abs(dw).max() > 0
        assert np.array_equal(_bits(dw), _bits(dp))
