"""Piecewise detrending, the written definition (the piecewise part of
iterative_cleaner_amd/detrend.py) on the CPU: one piece is the whole-line
statement, pieces are independent fits on their own abscissa and chains, a
sawtooth is recovered against numpy's least squares, retired pieces stay
retired, the IC_DETREND_PIECES switch, and the interface's declarations.

The coefficient bound is test_detrend_host.py's: the Gram matrix of the
monomials up to order 3 on [-1, 1] has a condition number of 1e3..1e4, so the
normal equations in f64 lose about 1e-12 of the largest coefficient; 1e-9
leaves three decades.
"""
import os
import re

import numpy as np
import pytest

import detrend_pieces_ref
import detrend_ref
from helpers import bits_equal, bits_equal_nan
from iterative_cleaner_amd import detrend as dt

COEF_RTOL = 1e-9
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_line(n, seed, dtype=np.float64):
    rng = np.random.default_rng(seed)
    d = (1.0 + 0.5 * np.linspace(-1.0, 1.0, n) ** 2 + 0.05 * rng.standard_normal(n)).astype(dtype)
    if n >= 20:
        d[rng.choice(n, size=max(1, n // 15), replace=False)] += dtype(4.0)
    valid = rng.random(n) < 0.85
    return d, valid


# ------------------------------------------------------------------ one piece

@pytest.mark.parametrize("rounds", (1, 4))
@pytest.mark.parametrize("k", (1, 2, 3))
@pytest.mark.parametrize("n", (1, 2, 3, 63, 64, 65, 130))
def test_one_piece_is_the_whole_line_statement(n, k, rounds):
    """[0]: line_fit's coefficients and d' bit for bit: ordinary lines, n <= k and
    n = 1, a NaN and an Inf member, a dead line, f32 values."""
    for variant in ("plain", "nan", "inf", "dead", "f32"):
        d, valid = _random_line(n, 100 * n + 10 * k + rounds, np.float32 if variant == "f32" else np.float64)
        if variant == "dead":
            valid[:] = False
        elif variant in ("nan", "inf"):
            valid[n // 2] = True
            d[n // 2] = np.nan if variant == "nan" else np.inf
        want, _, _ = dt.line_fit(d, valid, k, rounds)
        got, _, _ = dt.line_fit_pieces(d, valid, k, [0], rounds)
        assert got.shape == (1, 4)
        assert bits_equal(got[0], want), (variant, got, want)
        assert bits_equal_nan(dt.detrended_pieces(d, valid, got, k, [0]), dt.detrended(d, valid, want, k)), variant
        if variant in ("nan", "inf", "dead") or n <= k:
            assert not want.any()


def test_one_piece_cube_and_combine():
    """detrend_cube_pieces and the GPU tests' piecewise yardstick with one piece
    each: the whole-line ones (detrend_cube, detrend_ref.combine)."""
    data, w = detrend_ref.hard_cube(9, 70, 64, 3)
    valid = w != 0
    with np.errstate(invalid="ignore"):
        D = data.std(axis=2).astype(np.float64)
    a = dt.detrend_cube(D, valid, 2, 3)
    b = dt.detrend_cube_pieces(D, valid, 2, 3, [0], None)
    assert bits_equal_nan(a[0], b[0]) and bits_equal_nan(a[1], b[1])
    assert bits_equal_nan(a[2], b[2][:, 0]) and bits_equal_nan(a[3], b[3][:, 0])
    diags = (D, data.mean(axis=2).astype(np.float64), np.ptp(data, axis=2), np.abs(data).max(axis=2).astype(np.float64))
    t0, c0, s0, _ = detrend_ref.combine(diags, valid, 5.0, 4.0, (2, 3))
    t1, c1, s1 = detrend_pieces_ref.combine(diags, valid, 5.0, 4.0, (2, 3), [0], [0])
    assert bits_equal_nan(t0, t1) and bits_equal_nan(c0, c1[:, :, 0]) and bits_equal_nan(s0, s1[:, :, 0])
    assert np.isnan(t0).any() and not np.isnan(t0).all()


# ------------------------------------------------------------------ pieces

@pytest.mark.parametrize("k", (1, 2, 3))
def test_pieces_are_independent_at_one_round(k):
    """rounds = 1: a line in pieces is line_trend of every slice: the local
    abscissa and the local chains (pieces that start off the 64 grid, pieces of
    1, 2, 64, 65 and 130 entries)."""
    starts = [0, 1, 3, 67, 132, 262, 270]
    n = 300
    d, valid = _random_line(n, 7 + k)
    coef, used = dt.line_trend_pieces(d, valid, k, starts, rounds=1)
    assert used == 1 and coef.shape == (len(starts), 4)
    dp = dt.detrended_pieces(d, valid, coef, k, starts)
    for q, (b, e) in enumerate(zip(starts, starts[1:] + [n])):
        want, _ = dt.line_trend(d[b:e], valid[b:e], k, rounds=1)
        assert bits_equal(coef[q], want), (q, b, e)
        assert bits_equal(dp[b:e], dt.detrended(d[b:e], valid[b:e], want, k)), (q, b, e)
    assert coef[3].any() and not coef[0].any()


def test_sawtooth_is_recovered():
    """Quadratic teeth with noise: every piece's coefficients against
    numpy.linalg.lstsq on the piece's final members."""
    rng = np.random.default_rng(21)
    width, npieces = 16, 10
    n = width * npieces
    starts = dt.pieces_every(n, width)
    assert starts == list(range(0, n, width)) == dt.pieces_from_count(n, npieces)
    x = dt.piece_abscissa(starts, n)
    assert bits_equal(x[:width], dt.abscissa(width)) and bits_equal(x[-width:], dt.abscissa(width))
    tooth = rng.uniform(0.5, 2.0, size=(npieces, 3))
    y = np.concatenate([t[0] + t[1] * dt.abscissa(width) - t[2] * dt.abscissa(width) ** 2 for t in tooth])
    y += 1e-3 * rng.standard_normal(n)
    valid = np.ones(n, bool)
    coef, used, use = dt.line_fit_pieces(y, valid, 2, starts)
    assert used >= 1 and use.sum() >= 0.8 * n
    for q, b in enumerate(starts):
        sl = slice(b, b + width)
        u = use[sl]
        ref = np.linalg.lstsq(np.vander(x[sl][u], 3, increasing=True), y[sl][u], rcond=None)[0]
        assert np.abs(coef[q, :3] - ref).max() <= COEF_RTOL * np.abs(coef[q]).max(), q
        assert coef[q, 3] == 0.0
    # one cubic over the whole line cannot follow the teeth
    whole, _ = dt.line_trend(y, valid, 3)
    flat = dt.detrended_pieces(y, valid, coef, 2, starts)
    assert np.abs(flat).max() < 1e-2 < 0.1 < np.abs(dt.detrended(y, valid, whole, 3)).max()


def test_a_retired_piece_stays_retired():
    """A piece with <= k members keeps +0.0 in every round while its neighbours
    are fitted and the line goes on clipping; a piece that loses its members to
    the clip is retired from that round on."""
    rng = np.random.default_rng(2)
    n, starts, k = 48, [0, 16, 32], 2
    x = dt.piece_abscissa(starts, n)
    y = 1.0 + 0.5 * x + 0.01 * rng.standard_normal(n)
    y[40] += 30.0                                # an outlier: rounds go on
    valid = np.ones(n, bool)
    valid[16:32] = False
    valid[[18, 25]] = True                       # the middle piece: 2 members <= k
    for rounds in (1, 2, 4):
        coef, used, use = dt.line_fit_pieces(y, valid, k, starts, rounds)
        assert used == rounds or rounds == 4
        assert not coef[1].any() and not np.signbit(coef[1]).any()
        assert coef[0].any() and coef[2].any()
    assert not use[40] and used > 1
    # its entries come back undetrended
    dp = dt.detrended_pieces(y, valid, coef, k, starts)
    assert bits_equal(dp[[18, 25]], y[[18, 25]]) and np.abs(dp[:16]).max() < 0.1
    # the last piece: 4 members, one the outlier: fitted in round 1 (badly: the
    # residuals of all four stand far outside the line's clip), so the clip
    # leaves it <= k members and it is retired from round 2 on
    v2 = np.ones(n, bool)
    v2[32:] = False
    v2[[33, 36, 40, 45]] = True
    c1, _ = dt.line_trend_pieces(y, v2, k, starts, rounds=1)
    c2, used2, use2 = dt.line_fit_pieces(y, v2, k, starts, rounds=3)
    assert c1[2].any() and use2[32:].sum() <= k and used2 >= 2
    assert not c2[2].any() and not np.signbit(c2[2]).any() and c2[0].any()
    # with one piece "retire and go on" reaches no output (the statement's note): line_fit stops, the coefficients agree
    few = np.zeros(n, bool)
    few[[3, 9]] = True
    assert bits_equal(dt.line_fit_pieces(y, few, k, [0])[0][0], dt.line_fit(y, few, k)[0])


# ------------------------------------------------------------------ the switch

def test_helpers_and_their_refusals():
    assert dt.check_pieces((0, 3, 9), 10) == [0, 3, 9]
    assert dt.pieces_from_count(600, 512)[:4] == [0, 1, 2, 3] and len(dt.pieces_from_count(600, 512)) == 512
    assert dt.pieces_from_count(10, 3) == [0, 3, 6]
    assert dt.pieces_every(65, 16) == [0, 16, 32, 48, 64]
    assert dt.pieces_every(5, 9) == [0]
    for bad, n in (((1, 2), 10), ((0, 3, 3), 10), ((0, 5, 4), 10), ((0, 10), 10), ((0, 3, 11), 10), ((), 10),
                   (tuple(range(513)), 1000), ((0, 1.5), 10), ("ab", 10)):
        with pytest.raises(ValueError):
            dt.check_pieces(bad, n)
    for n, m in ((10, 11), (600, 513), (10, 0), (3, 4)):
        with pytest.raises(ValueError):
            dt.pieces_from_count(n, m)
    with pytest.raises(ValueError):
        dt.pieces_every(10, 0)
    with pytest.raises(ValueError):
        dt.pieces_every(1000, 1)                 # 1000 pieces


def test_switch_parsing(monkeypatch):
    assert dt.parse_pieces("") is None and dt.parse_pieces(" ; ") is None and dt.parse_pieces(None) is None
    assert dt.parse_pieces(";w16") == (None, "w16")
    assert dt.parse_pieces("3;") == (3, None)
    assert dt.parse_pieces("0,6; 0,16,40") == ((0, 6), (0, 16, 40))
    for junk in ("w16", "1;2;3", "x;", ";w", ";w0", ";-3", "0;", "513;", "1,2;", "0,3,2;", "0,3,3;", "0,;", ";1.5",
                 ";0 6"):
        with pytest.raises(ValueError):
            dt.parse_pieces(junk)
    monkeypatch.delenv("IC_DETREND_PIECES", raising=False)
    assert dt.env_pieces() is None and dt.normalise_pieces(None, 8, 160) is None
    monkeypatch.setenv("IC_DETREND_PIECES", "2;w16")
    assert dt.env_pieces() == (2, "w16")
    assert dt.normalise_pieces(None, 8, 160) == ([0, 4], list(range(0, 160, 16)))
    # an argument goes before the switch; every form of a side
    assert dt.normalise_pieces((None, 4), 8, 160) == (None, [0, 40, 80, 120])
    assert dt.normalise_pieces(([0, 3], "w100"), 8, 160) == ([0, 3], [0, 100])
    assert dt.normalise_pieces((None, None), 8, 160) is None
    # resolved with the shape: a start past n, coinciding starts from a count, too many pieces
    for bad in (([0, 8], None), (9, None), (None, "w1"), (None, [0, 160]), (None, 513), ("junk", None), (1, 2, 3)):
        with pytest.raises(ValueError):
            dt.normalise_pieces(bad, 8, 1000 if bad == (None, "w1") else 160)
    # detrending off: no pieces; a direction without an order: its pieces are ignored, unresolved
    assert dt.normalise_pieces((2, "w16"), 8, 160, None) is None
    assert dt.normalise_pieces((99, "w16"), 8, 160, (0, 2, 4, 5.0)) == (None, list(range(0, 160, 16)))
    assert dt.normalise_pieces((2, "w16"), 8, 160, (1, 0, 4, 5.0)) == ([0, 4], None)
    assert dt.normalise_pieces((None, "w16"), 8, 160, (1, 0, 4, 5.0)) is None


# ------------------------------------------------------------------ the interface

def test_interface_is_declared():
    from iterative_cleaner_amd import _native
    header = open(os.path.join(REPO, "include", "iterative_cleaner.h")).read()
    for sym in ("ic_set_detrend_pieces", "ic_get_trends_pieces", "ic_comprehensive_stats_detrend_pieces"):
        assert re.search(r"\bint %s\(" % sym, header), sym
        assert sym in _native.EXPORTS, sym
    assert re.search(r"#define\s+IC_ABI_VERSION\s+9\b", header) and _native.ABI_VERSION == 9
    assert "UNPINNED" in header.split("ic_set_detrend_pieces")[0].split("Piecewise detrending")[1]
    assert "breakpoints / numpieces" in header
    assert "UNPINNED" in dt.__doc__.split("Piecewise detrending")[1]
