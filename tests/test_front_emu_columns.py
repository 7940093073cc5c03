"""csrc/pps_front_reg.h, the 4-column form (W == 4, no strip, NT <= 4: what the register-only band kernels run: compile-time tile columns), on the CPU through the wave emulation of tests/cpp/wave_emu.h -- the library and the checks of tests/test_front_emu.py, at every
pivot count: a step that ends its tile column, a last step that stops short of it, hand-overs into every tile column, in the tile count
the kernels pick and in every larger one.  The 8-column form is the code that did not change: the fused build must leave the same bits
in both.  The hardware run of the hand-over shapes is tests/test_gpu_fronts_w4.py."""
import numpy as np
import pytest

from test_front_emu import _check, _emu_lib, _front, _runner, emu, emu_fused  # noqa: F401  (the fixtures)


def _shapes():
    """p = 1 .. 63 with b in {0, 1, 63 - p} and one b in between"""
    rng = np.random.default_rng(11)
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


SHAPES = _shapes()


def test_shapes_cover_what_the_issue_asks():
    ps = {p for p, _ in SHAPES}
    assert ps == set(range(1, 64))
    for p in range(1, 64):
        bs = {b for q, b in SHAPES if q == p}
        assert {0, 63 - p} <= bs and (1 in bs or 63 - p < 1)
        assert p > 60 or any(1 < b < 63 - p for b in bs)


def test_width_4_against_numpy_every_pivot_count(emu):
    for p, b in SHAPES:
        for tiles in _tile_counts(p, b):
            _check(emu, p, b, tiles, False, seed=100 * p + b, w=4)


def test_width_4_and_width_8_agree_bit_for_bit_every_pivot_count(emu_fused):
    for p, b in SHAPES:
        _, _, tri = _front(p, b, 100 * p + b)
        ok = np.tril(np.ones((p + b + 1, p), dtype=bool))          # (above the diagonal of L_A: unspecified in both)
        for tiles in _tile_counts(p, b):
            L4, U4, bad4, _ = emu_fused(tri, p, b, tiles, False, 4)
            L8, U8, bad8, _ = emu_fused(tri, p, b, tiles, False, 8)
            assert np.array_equal(L4[ok], L8[ok]) and np.array_equal(U4, U8) and bad4 == bad8 == 0.0, (p, b, tiles)


def test_one_mfma_per_tile_of_the_live_columns(emu):
    """a step in tile column TJ issues one MFMA for every tile (ti >= tj >= TJ), whatever the step: p = 15 / b = 33 in three tile rows is
    four steps in column 0 (6 tiles each); p = 18 / b = 0 in two tile rows is four steps in column 0 (3 tiles) and one in column 1 (1)"""
    assert _check(emu, 15, 33, 3, False, w=4)[1] == 4 * 6
    assert _check(emu, 18, 0, 2, False, w=4)[1] == 4 * 3 + 1
    assert _check(emu, 63, 0, 4, False, w=4)[1] == 4 * (10 + 6 + 3 + 1)


def test_not_positive_definite_in_the_second_tile_column(emu):
    _, _, tri = _front(20, 10, 3)
    assert emu(tri, 20, 10, 0, False, 4)[2] == 0.0
    t = tri.copy(); t[17 * 18 // 2 + 17] = -1.0                  # H[17][17]: first step of tile column 1
    assert emu(t, 20, 10, 0, False, 4)[2] == 1.0
    assert emu(t, 20, 10, 0, False, 8)[2] == 1.0
