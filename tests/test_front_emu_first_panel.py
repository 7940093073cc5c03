"""csrc/pps_front_reg.h, the 4-column form with its first panel read straight from the assembled triangle (the K = 0 step takes columns
0 .. 3 of row `lane` from F at the tile load's own addresses: no tile, no extraction, no read-back in front of the first pivot block), on
the CPU through the wave emulation of tests/cpp/wave_emu.h.  Every p = 1 .. 63 -- a front that ends inside the first panel, at its end, in
any later panel and tile column -- with b in {0, 1, one in between, 63 - p}, in the tile count the kernels pick and in every larger one.

The 8-column general form neither reads the triangle that way nor changed: the fused build must leave the same BITS in both -- the
factor panel as it is stored (the entries above the diagonal, which nothing reads, included wherever a form computes them -- _computed
below; in the first panel they are what the tile load finds in the next rows of the triangle, and tile column 0 is compared whole), the
update matrix and the rhs row.  Bits, not values: -0.0 and +0.0 differ here.
The hardware run is tests/test_gpu_first_panel.py."""
import numpy as np
import pytest

from test_front_emu import _check, _emu_lib, _front, _runner, emu, emu_fused  # noqa: F401  (the fixtures)


def _shapes():
    """p = 1 .. 63 with b in {0, 1, 63 - p} and one b in between"""
    rng = np.random.default_rng(23)
    out = []
    for p in range(1, 64):
        mid = int(rng.integers(2, 63 - p)) if 63 - p > 2 else 0
        for b in sorted({0, 1, mid, 63 - p}):
            if b >= 0 and p + b + 1 <= 64:
                out.append((p, b))
    return out


def _tile_counts(p, b):
    """the tile count the kernels pick for the front (rhs row as a vector: p + b rows in the tiles) and every larger one up to 4"""
    fa = p + b + 1
    t0 = 2 if fa <= 33 else 3 if fa <= 49 else 4
    return range(t0, 5)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _computed(p, b):
    """the entries of the stored factor panel that a form computes from the front: everything but rows of the tile rows ABOVE a column's
    tile column (row < 16 (col // 16)).  No tile exists there; a step of tile column 1 and up never extracts those rows, so what their lanes
    solve and store is what an earlier panel left in the panel buffer -- eight columns of it in one form, four in the other, in the code
    before the first panel came from the triangle as well.  Inside the column's own diagonal tile the entries above the diagonal ARE
    computed (from the next rows of the triangle, then updated like any entry) and are compared."""
    rows, cols = np.indices((p + b + 1, p))
    return rows >= 16 * (cols // 16)


SHAPES = _shapes()


def test_shapes_cover_every_pivot_count():
    assert {p for p, _ in SHAPES} == set(range(1, 64))
    for p in range(1, 64):
        bs = {b for q, b in SHAPES if q == p}
        assert {0, 63 - p} <= bs and (1 in bs or 63 - p < 1)
        assert p > 60 or any(1 < b < 63 - p for b in bs)


def test_against_numpy_every_pivot_count(emu):
    for p, b in SHAPES:
        for tiles in _tile_counts(p, b):
            _check(emu, p, b, tiles, False, seed=7 + 100 * p + b, w=4)


def test_same_bits_as_the_eight_column_form_every_pivot_count(emu_fused):
    """all of L as stored (rows 0 .. f, the rhs row f among them, and the entries above the diagonal that a form computes), all of U"""
    for p, b in SHAPES:
        _, _, tri = _front(p, b, 7 + 100 * p + b)
        for tiles in _tile_counts(p, b):
            L4, U4, bad4, _ = emu_fused(tri, p, b, tiles, False, 4)
            L8, U8, bad8, _ = emu_fused(tri, p, b, tiles, False, 8)
            assert bad4 == bad8 == 0.0, (p, b, tiles)
            ok = _computed(p, b)
            assert _same_bits(L4[ok], L8[ok]), (p, b, tiles, np.argwhere((_bits(L4) != _bits(L8)) & ok)[:4])
            assert _same_bits(L4[:, :min(p, 16)], L8[:, :min(p, 16)]), (p, b, tiles)       # (tile column 0: every row, whole)
            assert _same_bits(U4, U8), (p, b, tiles)


def test_signed_zeros_in_the_boundary_block_keep_their_bits(emu_fused):
    """a boundary row that no pivot touches: its entries against the other boundary rows and its rhs entry are zeros that only ever meet
    zero products, so their sign is decided by the signs of those products -- once with -0.0 and once with +0.0 in the triangle"""
    for p, b in [(1, 3), (2, 3), (3, 4), (5, 6), (6, 18), (7, 3), (9, 18), (15, 18), (18, 18)]:
        for zero in (-0.0, 0.0):
            H, rhs, tri = _front(p, b, 31 * p + b)
            f = p + b
            j = p + 1                                                   # the second boundary row
            t = tri.copy()
            t[j * (j + 1) // 2:j * (j + 1) // 2 + j] = zero             # row j left of its diagonal: pivot columns and boundary column p
            for i in range(j + 1, f):
                t[i * (i + 1) // 2 + j] = zero                          # column j below its diagonal
            t[f * (f + 1) // 2 + j] = zero                              # rhs entry of row j
            for tiles in _tile_counts(p, b):
                L4, U4, bad4, _ = emu_fused(t, p, b, tiles, False, 4)
                L8, U8, bad8, _ = emu_fused(t, p, b, tiles, False, 8)
                assert bad4 == bad8 == 0.0
                ok = _computed(p, b)
                assert _same_bits(L4[ok], L8[ok]) and _same_bits(U4, U8), (p, b, zero, tiles)
                Ut = np.zeros((b + 1, b + 1)); Ut[np.tril_indices(b + 1)] = U4
                assert Ut[1, 0] == 0.0 and Ut[b, 1] == 0.0 and (Ut[2:b, 1] == 0.0).all()


@pytest.mark.parametrize("w", [4, 8])
def test_not_positive_definite_flag_first_last_and_first_masked_pivot(emu, w):
    """the flag is raised for the pivots that exist -- the first, the last one of a partial or full last panel -- and not for the first masked
    one: column p of the last panel, the diagonal of the first boundary row, belongs to the update matrix"""
    for p, b in [(1, 4), (2, 4), (3, 4), (4, 4), (5, 4), (6, 20), (7, 4), (8, 4), (9, 18), (15, 18), (16, 10), (17, 10), (18, 18), (27, 21)]:
        _, _, tri = _front(p, b, 5 * p + b)
        diag = lambda i: i * (i + 1) // 2 + i
        assert emu(tri, p, b, 0, False, w)[2] == 0.0
        t = tri.copy(); t[diag(0)] = -1.0
        assert emu(t, p, b, 0, False, w)[2] == 1.0, ("first", p, b)
        t = tri.copy(); t[diag(p - 1)] = -1e6
        assert emu(t, p, b, 0, False, w)[2] == 1.0, ("last existing", p, b)
        t = tri.copy(); t[diag(p)] = -1e6
        assert emu(t, p, b, 0, False, w)[2] == 0.0, ("first masked", p, b)


def test_first_masked_pivot_not_positive_leaves_the_same_bits(emu_fused):
    for p, b in [(1, 4), (2, 4), (3, 4), (5, 4), (6, 20), (9, 18), (15, 18), (18, 18)]:
        _, _, tri = _front(p, b, 5 * p + b)
        t = tri.copy(); t[p * (p + 1) // 2 + p] = -1e6
        L4, U4, bad4, _ = emu_fused(t, p, b, 0, False, 4)
        L8, U8, bad8, _ = emu_fused(t, p, b, 0, False, 8)
        ok = _computed(p, b)
        assert bad4 == bad8 == 0.0 and _same_bits(L4[ok], L8[ok]) and _same_bits(U4, U8), (p, b)
        assert np.isfinite(L4[np.tril_indices(p + b + 1, 0, p)]).all() and np.isfinite(U4).all()
