"""Detrended scaling, the written definition (iterative_cleaner_amd/detrend.py)
on the CPU: recovery of a known trend against numpy's least squares, the
statement's rules, the IC_DETREND switch, and the control of the GPU tests'
yardstick (tests/detrend_ref.combine with zero trends is
oracle/restated.comprehensive_stats bit for bit).

The coefficient bound: the Gram matrix of the monomials up to order 3 on
[-1, 1] has a condition number of 1e3..1e4, so the normal equations in f64 lose
about 1e-12 of the largest coefficient; 1e-9 leaves three decades.
"""
import os
import re

import numpy as np
import pytest

import detrend_ref
from helpers import bits_equal, bits_equal_nan
from iterative_cleaner_amd import detrend as dt

COEF_RTOL = 1e-9
LENGTHS = (1, 2, "k", "k+1", 63, 64, 65, 130, 1000)


def _line(n, k, seed):
    """y = polynomial(order k) + small noise with up to 10 % gross outliers."""
    rng = np.random.default_rng(seed)
    x = dt.abscissa(n)
    c = rng.uniform(0.5, 2.0, size=k + 1) * rng.choice([-1.0, 1.0], size=k + 1)
    y = sum(c[i] * x ** i for i in range(k + 1)) + 1e-3 * rng.standard_normal(n)
    out = np.zeros(n, bool)
    if n >= 20:
        out[rng.choice(n, size=rng.integers(1, n // 10 + 1), replace=False)] = True
        y[out] += rng.choice([-1.0, 1.0], size=int(out.sum())) * rng.uniform(5.0, 50.0, size=int(out.sum()))
    return x, y, out, c


@pytest.mark.parametrize("k", (1, 2, 3))
@pytest.mark.parametrize("length", LENGTHS)
def test_recovers_a_known_trend(length, k):
    n = k if length == "k" else k + 1 if length == "k+1" else length
    x, y, out, _ = _line(n, k, 1000 * k + n)
    valid = np.ones(n, bool)
    coef, used, use = dt.line_fit(y, valid, k)
    c2, u2 = dt.line_trend(y, valid, k)
    assert bits_equal(coef, c2) and used == u2
    if n <= k:                                   # |valid| <= k: zero trend
        assert not coef.any() and not np.signbit(coef).any()
        return
    assert used >= 1 and not (use & out).any(), "outliers left in the final membership"
    assert use[~out].sum() >= 0.8 * (~out).sum()
    ref = np.linalg.lstsq(np.vander(x[use], k + 1, increasing=True), y[use], rcond=None)[0]
    assert np.abs(coef[:k + 1] - ref).max() <= COEF_RTOL * np.abs(coef).max()
    assert not coef[k + 1:].any()


def test_sums_follow_the_written_order():
    rng = np.random.default_rng(5)
    for n in (1, 63, 64, 65, 130, 1000):
        t = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, size=n)
        chains = []
        for lane in range(64):
            acc = np.float64(0.0)
            for j in range(lane, n, 64):
                acc = acc + t[j]
            chains.append(acc)
        h = 32
        while h:
            chains = [chains[q] + chains[q + h] for q in range(h)]
            h //= 2
        assert bits_equal(np.float64(chains[0]), np.float64(dt.chain_sum(t)))


def test_rules():
    rng = np.random.default_rng(11)
    n = 80
    x = dt.abscissa(n)
    y = 2.0 + 3.0 * x + 1e-2 * rng.standard_normal(n)
    valid = rng.random(n) < 0.8
    zero = np.zeros(4)
    # a NaN or Inf valid entry: zero trend; an invalid one does not matter
    for bad in (np.nan, np.inf, -np.inf):
        yb = y.copy()
        yb[np.nonzero(valid)[0][3]] = bad
        coef, used = dt.line_trend(yb, valid, 2)
        assert bits_equal(coef, zero) and used == 0
        yi = y.copy()
        yi[np.nonzero(~valid)[0][0]] = bad
        assert bits_equal(dt.line_trend(yi, valid, 2)[0], dt.line_trend(y, valid, 2)[0])
    # all-invalid line, |valid| <= k
    assert bits_equal(dt.line_trend(y, np.zeros(n, bool), 1)[0], zero)
    for k in (1, 2, 3):
        few = np.zeros(n, bool)
        few[[5, 40, 70][:k]] = True
        coef, used = dt.line_trend(y, few, k)
        assert bits_equal(coef, zero) and used == 0
        few[77] = True                            # k + 1 members: a fit
        assert dt.line_trend(y, few, k)[1] >= 1
    # a constant line (mad == 0) stops after one fit; rounds = 1 fits once
    coef, used = dt.line_trend(np.full(n, 1.25), valid, 2)
    assert used == 1 and abs(coef[0] - 1.25) < 1e-12
    yo = y.copy()
    yo[np.nonzero(valid)[0][::9]] += 40.0
    assert dt.line_trend(yo, valid, 1, rounds=1)[1] == 1
    assert dt.line_trend(yo, valid, 1, rounds=4)[1] > 1
    # invalid entries come back unchanged; valid ones lose the trend
    coef, _ = dt.line_trend(yo, valid, 1)
    d1 = dt.detrended(yo, valid, coef, 1)
    assert bits_equal(d1[~valid], yo[~valid])
    assert np.abs(d1[valid] - (yo[valid] - (coef[0] + coef[1] * x[valid]))).max() < 1e-12
    # f32 lines stay f32
    y32 = yo.astype(np.float32)
    c32, _ = dt.line_trend(y32, valid, 1)
    d32 = dt.detrended(y32, valid, c32, 1)
    assert d32.dtype == np.float32 and bits_equal(d32[~valid], y32[~valid])
    want = (y32.astype(np.float64) - dt.poly_eval(x, c32, 1)).astype(np.float32)
    assert bits_equal(d32[valid], want[valid])
    # order 0: the input's bits; a zero trend of any order too (-0.0 and NaN included)
    odd = y.copy()
    odd[:3] = (-0.0, np.nan, np.inf)
    c0, u0 = dt.line_trend(odd, valid, 0)
    assert bits_equal(c0, zero) and u0 == 0
    assert dt.detrended(odd, valid, c0) is odd
    for k in (1, 2, 3):
        assert bits_equal_nan(dt.detrended(odd, np.ones(n, bool), zero, k), odd)
    # a pivot that is not > 0: n == 1 has x = 0, S_2 = 0 at order 1 (|use| <= k comes first), and a
    # two-point line at order 1 is solvable
    assert bits_equal(dt.line_trend(np.array([3.0]), np.ones(1, bool), 1)[0], zero)
    c2, _ = dt.line_trend(np.array([1.0, 3.0]), np.ones(2, bool), 1)
    assert c2[0] == 2.0 and c2[1] == 1.0


def test_switch_parsing_and_refusals(monkeypatch):
    monkeypatch.delenv("IC_DETREND", raising=False)
    assert dt.env_detrend() is None
    for text in ("", "0", " 0 ", "0,0", "0,0,3,2.5"):
        monkeypatch.setenv("IC_DETREND", text)
        assert dt.env_detrend() is None
    monkeypatch.setenv("IC_DETREND", "1,2")
    assert dt.env_detrend() == (1, 2, 4, 5.0)
    monkeypatch.setenv("IC_DETREND", " 3, 0 ,8, 2.5")
    assert dt.env_detrend() == (3, 0, 8, 2.5)
    for bad in ("1", "4,1", "1,-1", "1,2,0", "1,2,9", "1,2,4,0", "1,2,4,-1", "1,2,4,inf", "1,2,4,nan",
                "a,b", "1.5,1", "1,2,3,4,5"):
        monkeypatch.setenv("IC_DETREND", bad)
        with pytest.raises(ValueError):
            dt.env_detrend()
    monkeypatch.setenv("IC_DETREND", "2,1")
    assert dt.normalise(None) == (2, 1, 4, 5.0)
    assert dt.normalise((0, 0)) is None and dt.normalise((1, 0, 2)) == (1, 0, 2, 5.0)
    for bad in ((4, 0), (0, -1), (1, 1, 0), (1, 1, 9), (1, 1, 4, 0.0), (1, 1, 4, float("inf")), (1,), (1.5, 1)):
        with pytest.raises(ValueError):
            dt.normalise(bad)


def test_run_loop_refuses_detrend_under_channel_sharding(monkeypatch):
    """Before any session is made (no GPU, no library needed)."""
    import argparse

    from iterative_cleaner_amd import _native, cleaner, dist
    monkeypatch.setattr(dist, "channel_sharding", lambda: True)   # (the real one joins a process group)

    def no_session(*a, **k):
        raise AssertionError("a session was made")
    monkeypatch.setattr(_native, "GpuSession", no_session)
    monkeypatch.setattr(_native, "shard_layout", no_session)
    args = argparse.Namespace(max_iter=1, chanthresh=5.0, subintthresh=5.0, pulse_region=[0, 0, 1])
    cube = np.zeros((2, 512, 64), np.float32)
    with pytest.raises(ValueError, match="channel sharding"):
        cleaner.run_loop(cube, np.ones((2, 512), np.float32), np.zeros(512, np.int64), args, detrend=(1, 2))
    monkeypatch.setenv("IC_DETREND", "1,1")
    with pytest.raises(ValueError, match="channel sharding"):
        cleaner.run_loop(cube, np.ones((2, 512), np.float32), np.zeros(512, np.int64), args)


def test_interface_is_declared():
    from iterative_cleaner_amd import _native
    here = os.path.dirname(os.path.abspath(__file__))
    text = open(os.path.join(here, "..", "include", "iterative_cleaner.h")).read()
    for name in ("ic_set_detrend", "ic_get_trends", "ic_comprehensive_stats_detrend"):
        assert re.search(r"\bint %s\(" % name, text) and name in _native.EXPORTS
    assert re.search(r"^#define IC_ABI_VERSION 9$", text, re.M) and _native.ABI_VERSION == 9
    assert "UNPINNED" in text and "UNPINNED" in dt.__doc__
    assert "oracle" not in "".join(line for line in open(dt.__file__) if "import" in line)


def test_control_combine_is_restated():
    """The yardstick's combine with zero trends equals restated.comprehensive_stats
    bit for bit (a NaN matches a NaN), NaN rule included."""
    from iterative_cleaner_amd import synth
    from oracle import restated
    data, w0, _ = synth.make_cube(6, 40, 64, 21, 0.1)
    raw = data[:, 0].copy()
    w0 = synth.fractional_weights(w0)
    raw[2, 7, 3] = np.nan                       # a NaN diagnostic: its channel and subint go NaN
    raw[4, 9, 1] = np.inf
    X = restated.weighted_cube(raw, w0)
    valid = w0 != 0
    want = restated.comprehensive_stats(X, w0, 5, 4.0)
    got, cc, sc, used = detrend_ref.combine(restated.diagnostics(X, valid), valid, 5, 4.0, None)
    assert np.isnan(want).any() and not np.isnan(want).all()
    assert bits_equal_nan(got, want)
    assert not cc.any() and not sc.any() and not any(used)
    # detrending changes it (the yardstick is not blind to the trend)
    got2, cc2, _, _ = detrend_ref.combine(restated.diagnostics(X, valid), valid, 5, 4.0, (1, 2))
    assert cc2.any() and not bits_equal_nan(got2, want)
