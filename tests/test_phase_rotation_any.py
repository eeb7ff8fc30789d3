"""The opt-in chirp-z statement of the rotation (phase_rotation.rotate_czt): any
profile length in 16..4096 that the default rotation kernels do not serve.

Accuracy against numpy's f64 rotation (oracle/restated.fft_phase_shift) on the
inputs of tests/test_phase_rotation_mr.py ``_max_error``, in f32 epsilons of the
profile's largest |sample|.  Measured maxima: 16: 4.08, 17: 2.73, 33: 3.30,
48: 2.92, 100: 3.09, 125: 2.47, 129: 3.25, 448: 3.16, 500: 3.08, 997: 3.54,
2047: 3.23, 2049: 3.05, 2500: 3.78, 4095: 2.93.  Bound: the largest (4.08)
plus 25 % for other seeds and delays, rounded up to half an epsilon = 5.5 (the
condition: no more than 8, twice the default rotation's 4).

Every test here fails where the host layer has no ``any_length`` / IC_ANY_NBIN.
"""
import os

import numpy as np
import pytest

from iterative_cleaner_amd import synth

EPS = float(np.finfo(np.float32).eps)
LENGTHS = [16, 17, 33, 48, 100, 125, 129, 448, 500, 997, 2047, 2049, 2500, 4095]
BOUND = 5.5      # f32 epsilons of the largest |sample| (module docstring)
REFUSED = [100, 500, 48, 56, 4104, 4200, 448]     # test_phase_rotation_mr.py REFUSED
SWITCH = "IC_ANY_NBIN"
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "iterative_cleaner.h")


def _max_error(n):
    """test_phase_rotation_mr._max_error with the opt-in."""
    from iterative_cleaner_amd import phase_rotation as pr
    from oracle.restated import fft_phase_shift
    rng = np.random.default_rng(n)
    d = rng.uniform(-3 * n, 3 * n, 16)
    x = (rng.standard_normal((8, 16, n)) * 10 + 3).astype(np.float32)
    ph = pr.phasors(n, d)
    scale = np.max(np.abs(x), axis=-1, keepdims=True).astype(np.float64)
    worst = 0.0
    for sign in (1, -1):
        got = pr.rotate(x, ph, sign, any_length=True)
        assert got.dtype == np.float32
        want = fft_phase_shift(x, d, sign)
        worst = max(worst, float(np.max(np.abs(got.astype(np.float64) - want) / (EPS * scale))))
    return worst


@pytest.mark.parametrize("n", LENGTHS)
def test_rotation_within_bound_of_numpy_fft(n):
    """Measured maxima, in f32 epsilons of the largest |sample|: 16: 4.08,
    17: 2.73, 33: 3.30, 48: 2.92, 100: 3.09, 125: 2.47, 129: 3.25, 448: 3.16,
    500: 3.08, 997: 3.54, 2047: 3.23, 2049: 3.05, 2500: 3.78, 4095: 2.93.
    Bound 5.5 = 4.08 x 1.25 rounded up to half an epsilon, below the 8 allowed."""
    from iterative_cleaner_amd import phase_rotation as pr
    assert pr.czt_selected(n, True) and not pr.czt_selected(n, False)
    worst = _max_error(n)
    print("nbin %d: %.2f eps" % (n, worst))
    assert BOUND <= 8.0 and worst <= BOUND


@pytest.mark.parametrize("n", [100, 125])
def test_integer_and_zero_delays(n):
    """A zero delay is the identity and an integer delay numpy's roll, within
    the accuracy bound."""
    from iterative_cleaner_amd import phase_rotation as pr
    rng = np.random.default_rng(7 + n)
    x = (rng.standard_normal((3, 4, n)) * 5).astype(np.float32)
    d = np.array([0.0, 5.0, n - 1.0, 2.0 * n + 9])
    y = pr.rotate(x, pr.phasors(n, d), 1, any_length=True)
    back = pr.rotate(x, pr.phasors(n, d), -1, any_length=True)
    for c, s in enumerate([0, 5, n - 1, 9]):
        scale = np.max(np.abs(x[:, c]), axis=-1, keepdims=True)
        assert np.all(np.abs(y[:, c] - np.roll(x[:, c], -s, axis=-1)) <= BOUND * np.float32(EPS) * scale)
        assert np.all(np.abs(back[:, c] - np.roll(x[:, c], s, axis=-1)) <= BOUND * np.float32(EPS) * scale)


@pytest.mark.parametrize("n", [100, 125])
def test_edge_values_run_and_propagate(n):
    """test_phase_rotation_mr.test_edge_values_run_and_propagate at chirp-z
    lengths: subnormals, overflow, signed zeros and a spike, per channel and per
    profile, both signs."""
    from iterative_cleaner_amd import phase_rotation as pr
    from test_phase_rotation import _edge_cube
    x = _edge_cube(n)
    rng = np.random.default_rng(n)
    d = rng.uniform(-2 * n, 2 * n, 6)
    d[1], d[2] = 0.0, 0.5
    d2 = rng.uniform(-2 * n, 2 * n, (4, 6))
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for delay in (d, d2):
            ph = pr.phasors(n, delay)
            for sign in (1, -1):
                a = pr.rotate(x, ph, sign, any_length=True)
                assert a.dtype == np.float32 and a.shape == x.shape
                assert not np.isfinite(a[1, 0]).all()           # the overflow case does overflow
                assert np.all(a[1, 1] == 0) and np.all(a[1, 2] == 0)
                assert np.isfinite(a[2, 3]).all() and np.isfinite(a[0]).all()
        y = x.copy()
        y[3, 1, n - 1] = np.nan
        y[3, 2, 2] = np.inf
        b = pr.rotate(y, pr.phasors(n, d), 1, any_length=True)
        clean = pr.rotate(x, pr.phasors(n, d), 1, any_length=True)
    assert np.isnan(b[3, 1]).all() and not np.isfinite(b[3, 2]).any()
    keep = np.ones(x.shape[:2], bool)
    keep[3, 1] = keep[3, 2] = False
    assert np.array_equal(b[keep], clean[keep], equal_nan=True)


@pytest.mark.parametrize("n", [17, 125, 997, 2047, 4095, 100, 2500])
def test_phasors_within_1e15_of_exact(n):
    """phasors() at odd n (harmonics 0 .. (n - 1)/2; its formula never used
    that n is even) against x87 long double, the construction and bound of
    test_phase_rotation_mr.test_phasors_within_1e15_of_exact."""
    from iterative_cleaner_amd import phase_rotation as pr
    rng = np.random.default_rng(n)
    d = np.concatenate([rng.uniform(-3 * n, 3 * n, 40), [0.0, 0.5, -1.25, 7.0, n * 0.37]])
    ph = pr.phasors(n, d)
    assert ph.shape == (2, d.size, n // 2 + 1)
    k = np.arange(n // 2 + 1, dtype=np.longdouble)
    r = np.fmod(k[None, :] * d.astype(np.longdouble)[:, None], np.longdouble(n))
    ang = 2 * np.longdouble("3.141592653589793238462643383279502884") * r / np.longdouble(n)
    err = float(np.maximum(np.abs(ph[0] - np.cos(ang)), np.abs(ph[1] - np.sin(ang))).max())
    print("nbin %d: phasor error %.2e" % (n, err))
    assert err < 1e-15


@pytest.mark.parametrize("n", [16, 17, 100, 125, 997, 2049, 4095])
def test_filter_table_is_the_exactly_rounded_one(n):
    """B (the written-order f64 Stockham, rounded to f32) against numpy's f64
    fft of the same b rounded to f32: within 1 f32 ulp, the ulp taken at the
    entry's modulus (a part near zero of an entry of modulus ~sqrt(n) carries
    the f64 transforms' absolute error, ~1e-14, not a relative one)."""
    from iterative_cleaner_amd import phase_rotation as pr
    L = pr.czt_length(n)
    assert L >= 2 * n - 1 and L // 2 < 2 * n - 1 and L & (L - 1) == 0
    w = pr.czt_chirp(n)
    j = np.arange(n)
    assert np.array_equal(w, pr.twiddles(2 * n)[:, (j * j) % (2 * n)])
    b = np.zeros(L, np.complex128)
    b[j] = w[0] - 1j * w[1]
    b[(L - j) % L] = w[0] - 1j * w[1]
    want = np.fft.fft(b)
    got = pr.czt_filter(n)
    assert got.dtype == np.float32 and got.shape == (2, L)
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(got[0].astype(np.float64) - want.real.astype(np.float32)) <= ulp)
    assert np.all(np.abs(got[1].astype(np.float64) - want.imag.astype(np.float32)) <= ulp)


def _foreign_file(tmp_path, nbin):
    """test_psrfits.test_fractional_delays_at_unsupported_nbin_fail_loudly's file."""
    from iterative_cleaner_amd import psrfits
    ar = synth.make_archive(2, 8, nbin, seed=4)
    ar._dm, ar._period = 30.0, 0.05
    ar._chan_freqs = 1400.0 + np.arange(8) * 10.0 - 35.0
    p = str(tmp_path / ("u%d.fits" % nbin))
    psrfits.save(ar, p, stand_in_meta=False)
    return p


@pytest.mark.parametrize("env", [None, "", "0"])
def test_switch_off_every_refusal_stays(tmp_path, monkeypatch, env):
    from iterative_cleaner_amd import archive as ica
    from iterative_cleaner_amd import dedispersion, psrfits
    from iterative_cleaner_amd import phase_rotation as pr
    if env is None:
        monkeypatch.delenv(SWITCH, raising=False)
    else:
        monkeypatch.setenv(SWITCH, env)
    assert not pr.any_length_enabled()
    for n in REFUSED:
        assert not pr.mr_supported(n) and not pr.is_supported(n) and not dedispersion.fft_supported(n), n
        with pytest.raises(ValueError, match="power-of-two nbin"):
            ica.Archive(np.zeros((2, 1, 3, n), np.float32), dm_delay=np.array([0.5, 1.25, -3.0]))
        with pytest.raises(ValueError, match="power-of-two nbin"):
            dedispersion.plan(np.array([0.5, 1.25, -3.0]), n)
        with pytest.raises(ValueError, match="power-of-two nbin"):
            pr.rotate(np.zeros((1, 3, n), np.float32), np.zeros((2, 3, n // 2 + 1)), 1)
    with pytest.raises(ValueError, match="power-of-two nbin.*IC_ANY_NBIN"):   # the hint names the switch
        dedispersion.plan(np.array([0.5]), 100)
    with pytest.raises(ValueError, match="power-of-two nbin"):
        psrfits.load(_foreign_file(tmp_path, 100))


@pytest.mark.parametrize("how", ["env", "keyword"])
def test_opted_in(tmp_path, monkeypatch, how):
    """plan, Archive, rotate and psrfits.load succeed at 100 / 125 / 448 bins,
    the delays stay unrounded; 8, 4104 and 16384 bins stay refused."""
    from iterative_cleaner_amd import archive as ica
    from iterative_cleaner_amd import dedispersion, psrfits
    from iterative_cleaner_amd import phase_rotation as pr
    if how == "env":
        monkeypatch.setenv(SWITCH, "1")
        kw = {}
        assert pr.any_length_enabled()
    else:
        monkeypatch.delenv(SWITCH, raising=False)
        kw = {"any_length": True}
    d = np.array([0.5, 1.25, -3.0])
    for n in (100, 125, 448):
        shift, delay = dedispersion.plan(d, n, **kw)
        assert np.array_equal(shift, np.zeros(3, np.int64)) and np.array_equal(delay, d)
        d2 = d[None, :] * (1.0 + 1e-6 * np.arange(2))[:, None]
        assert np.array_equal(dedispersion.plan(d2, n, **kw)[1], d2)
        rng = np.random.default_rng(n)
        data = rng.standard_normal((2, 1, 3, n)).astype(np.float32)
        ar = ica.Archive(data, dm_delay=d, **kw)
        assert np.array_equal(ar.get_dm_delay(), d)
        want = pr.rotate_czt(data, pr.phasors(n, d), 1)
        assert np.array_equal(pr.rotate(data, pr.phasors(n, d), 1, **kw), want)
        cl = ar.clone()
        cl.dedisperse()
        assert np.array_equal(cl._data, want)
        cl.dededisperse()
        assert np.array_equal(cl._data, pr.rotate_czt(want, pr.phasors(n, d), -1))
    br = psrfits.load(_foreign_file(tmp_path, 100), **kw)
    dl = br.get_dm_delay()
    assert dl is not None and np.any(dl != np.rint(dl))
    f = 1400.0 + np.arange(8) * 10.0 - 35.0
    fr = br.get_centre_frequency()
    t = (30.0 * (1.0 / 2.41e-4)) * (1.0 / (f * f) - 1.0 / (fr * fr))
    assert np.array_equal(dl, t / 0.05 * 100.0)
    for n in (8, 4104, 16384):
        assert not pr.czt_selected(n, True)
        with pytest.raises(ValueError, match="power-of-two nbin"):
            dedispersion.plan(d, n, **kw)
    # (8 and 16384 are powers of two: the numpy statement itself, and with it the stand-in, is defined there;
    # the loader and the library refuse them)
    with pytest.raises(ValueError, match="power-of-two nbin"):
        ica.Archive(np.zeros((2, 1, 3, 4104), np.float32), dm_delay=d, **kw)
    with pytest.raises(ValueError, match="power-of-two nbin"):
        pr.rotate(np.zeros((1, 3, 4104), np.float32), np.zeros((2, 3, 2053)), 1, **kw)


@pytest.mark.parametrize("n", [64, 128, 200, 1000])
def test_served_lengths_keep_their_bits(n):
    from iterative_cleaner_amd import phase_rotation as pr
    rng = np.random.default_rng(n)
    x = (rng.standard_normal((2, 3, n)) * 9).astype(np.float32)
    ph = pr.phasors(n, rng.uniform(-n, n, 3))
    assert not pr.czt_selected(n, True)
    for sign in (1, -1):
        assert pr.rotate(x, ph, sign, any_length=True).tobytes() == pr.rotate(x, ph, sign).tobytes()


def test_header_declares_the_mode_and_symbol():
    import re
    text = open(HEADER).read()
    assert re.search(r"^#define IC_ABI_VERSION 9$", text, re.M)
    assert re.search(r"^#define IC_DEDISP_FFT_ANY 2$", text, re.M)
    assert re.search(r"^int ic_rotate_profiles_any\(int device, int nsub, int nchan, int nbin, const float \*in, "
                     r"const double \*delay_bins,\s+int per_profile, int sign, float \*out\);", text, re.M)
    from iterative_cleaner_amd import _native
    assert "ic_rotate_profiles_any" in _native.EXPORTS and _native.DEDISP_FFT_ANY == 2
