"""The written-order f32 phase rotation at mixed-radix profile lengths (N = 2M,
M = 2^a 3^b 5^c, N a multiple of 8 in 64..4096; phase_rotation.py mr_supported,
stage_radices, DFT_3 and DFT_5).  CPU tests of the numpy definition: its error
against numpy's f64 rotation (oracle/restated.py fft_phase_shift) under the
project's bound of 4 f32 epsilons of the profile's largest |sample|, integer
and zero delays, edge values, the phasors against x87 long double, and the
predicate every host layer shares.  The power-of-two lengths keep their own
tests (tests/test_phase_rotation.py: bit-equal to the C oracle)."""
import numpy as np
import pytest

from test_phase_rotation import _edge_cube

LENGTHS = [72, 96, 120, 200, 1000, 1536, 4000]
MR_EXAMPLES = [72, 80, 96, 120, 200, 240, 400, 1000, 1200, 1536, 2000, 3000, 3840, 4000]
REFUSED = [100, 500, 48, 56, 4104, 4200, 448]   # 448 = 64 * 7: a multiple of 8 with a factor 7

EPS = float(np.finfo(np.float32).eps)


def _max_error(n):
    """Largest |pr.rotate - fft_phase_shift| in f32 epsilons of the profile's
    largest |sample|, both signs, on test_rotation_within_f32_error_of_numpy_fft's inputs."""
    from iterative_cleaner_amd import phase_rotation as pr
    from oracle.restated import fft_phase_shift
    rng = np.random.default_rng(n)
    d = rng.uniform(-3 * n, 3 * n, 16)
    x = (rng.standard_normal((8, 16, n)) * 10 + 3).astype(np.float32)
    ph = pr.phasors(n, d)
    scale = np.max(np.abs(x), axis=-1, keepdims=True).astype(np.float64)
    worst = 0.0
    for sign in (1, -1):
        got = pr.rotate(x, ph, sign)
        want = fft_phase_shift(x, d, sign)
        worst = max(worst, float(np.max(np.abs(got.astype(np.float64) - want) / (EPS * scale))))
    return worst


@pytest.mark.parametrize("n", LENGTHS)
def test_rotation_within_4_eps_of_numpy_fft(n):
    """Measured maxima, in f32 epsilons of the largest |sample| (stage order:
    power-of-two levels, then the 3s, then the 5s): 72: 2.26, 96: 2.41,
    120: 2.43, 200: 2.48, 1000: 3.19, 1536: 2.32, 4000: 2.74 (the powers of
    two measure 2.2-2.7 on the same inputs).  Bound: the header's 4."""
    worst = _max_error(n)
    print("nbin %d: %.2f f32 epsilons" % (n, worst))
    assert worst <= 4.0


@pytest.mark.parametrize("n", [200, 1536])
def test_integer_and_zero_delays(n):
    """A zero delay is the identity and an integer delay numpy's roll, within
    the f32 transforms' error (4 epsilons of the largest |sample|)."""
    from iterative_cleaner_amd import phase_rotation as pr
    rng = np.random.default_rng(7 + n)
    x = (rng.standard_normal((3, 4, n)) * 5).astype(np.float32)
    d = np.array([0.0, 5.0, n - 1.0, 2.0 * n + 9])
    y = pr.rotate(x, pr.phasors(n, d), 1)
    back = pr.rotate(x, pr.phasors(n, d), -1)
    for c, s in enumerate([0, 5, n - 1, 9]):
        scale = np.max(np.abs(x[:, c]), axis=-1, keepdims=True)
        assert np.all(np.abs(y[:, c] - np.roll(x[:, c], -s, axis=-1)) <= 4 * np.float32(EPS) * scale)
        assert np.all(np.abs(back[:, c] - np.roll(x[:, c], s, axis=-1)) <= 4 * np.float32(EPS) * scale)


@pytest.mark.parametrize("n", [120, 1000])
def test_edge_values_run_and_propagate(n):
    """Subnormals, overflow, signed zeros and a spike, per channel and per
    profile, both signs: no error, every output f32; an overflowing profile
    ends non-finite, a NaN or Inf sample makes its own profile non-finite and
    leaves the others alone, and a zero profile stays zero."""
    from iterative_cleaner_amd import phase_rotation as pr
    x = _edge_cube(n)
    rng = np.random.default_rng(n)
    d = rng.uniform(-2 * n, 2 * n, 6)
    d[1], d[2] = 0.0, 0.5
    d2 = rng.uniform(-2 * n, 2 * n, (4, 6))
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for delay in (d, d2):
            ph = pr.phasors(n, delay)
            for sign in (1, -1):
                a = pr.rotate(x, ph, sign)
                assert a.dtype == np.float32 and a.shape == x.shape
                assert not np.isfinite(a[1, 0]).all()           # the overflow case does overflow
                assert np.all(a[1, 1] == 0) and np.all(a[1, 2] == 0)
                assert np.isfinite(a[2, 3]).all() and np.isfinite(a[0]).all()
        y = x.copy()
        y[3, 1, n - 1] = np.nan
        y[3, 2, 2] = np.inf
        b = pr.rotate(y, pr.phasors(n, d), 1)
        clean = pr.rotate(x, pr.phasors(n, d), 1)
    assert np.isnan(b[3, 1]).all() and not np.isfinite(b[3, 2]).any()
    keep = np.ones(x.shape[:2], bool)
    keep[3, 1] = keep[3, 2] = False
    assert np.array_equal(b[keep], clean[keep], equal_nan=True)


@pytest.mark.parametrize("n", LENGTHS)
def test_phasors_within_1e15_of_exact(n):
    """ic_phasor's product form against exp(2 pi i k d / n) in x87 long double,
    the construction of test_phasors_within_7e16_of_exact.  Measured: 72:
    3.19e-16, 96: 2.93e-16, 120: 2.76e-16, 200: 4.38e-16, 1000: 5.50e-16,
    1536: 7.04e-16, 4000: 5.70e-16 (4/n is a rounded factor; a power of two
    stays under 7e-16).  Bound 1e-15: eight orders below the f32 epsilon the phasors are
    rounded to."""
    from iterative_cleaner_amd import phase_rotation as pr
    rng = np.random.default_rng(n)
    d = np.concatenate([rng.uniform(-3 * n, 3 * n, 40), [0.0, 0.5, -1.25, 7.0, n * 0.37]])
    ph = pr.phasors(n, d)
    k = np.arange(n // 2 + 1, dtype=np.longdouble)
    r = np.fmod(k[None, :] * d.astype(np.longdouble)[:, None], np.longdouble(n))
    ang = 2 * np.longdouble("3.141592653589793238462643383279502884") * r / np.longdouble(n)
    err = float(np.maximum(np.abs(ph[0] - np.cos(ang)), np.abs(ph[1] - np.sin(ang))).max())
    print("nbin %d: phasor error %.2e" % (n, err))
    assert err < 1e-15


def test_power_of_two_stage_order_is_unchanged():
    from iterative_cleaner_amd import phase_rotation as pr
    assert pr.stage_radices(2) == [2] and pr.stage_radices(4) == [4] and pr.stage_radices(32) == [8, 4]
    assert pr.stage_radices(512) == [8, 8, 8] and pr.stage_radices(4096) == [8, 8, 8, 8]
    assert pr.stage_radices(36) == [4, 3, 3] and pr.stage_radices(48) == [8, 2, 3]
    assert pr.stage_radices(1920) == [8, 8, 2, 3, 5] and pr.stage_radices(500) == [4, 5, 5, 5]
    assert max(len(pr.stage_radices(n // 2)) for n in range(64, 4097, 8) if pr.mr_supported(n)) <= 12


def test_predicate_and_messages():
    """fft_supported, is_supported and the Archive constructor share one set."""
    from iterative_cleaner_amd import archive as ica
    from iterative_cleaner_amd import dedispersion
    from iterative_cleaner_amd import phase_rotation as pr
    for n in MR_EXAMPLES:
        assert pr.mr_supported(n) and pr.is_supported(n) and dedispersion.fft_supported(n), n
        ar = ica.Archive(np.zeros((2, 1, 3, n), np.float32), dm_delay=np.array([0.5, 1.25, -3.0]))
        assert ar.get_dm_delay().shape == (3,)
    for n in (64, 128, 1024, 4096, 8192):
        assert not pr.mr_supported(n) and dedispersion.fft_supported(n)
    for n in REFUSED:
        assert not pr.mr_supported(n) and not pr.is_supported(n) and not dedispersion.fft_supported(n), n
        with pytest.raises(ValueError, match="power-of-two nbin"):
            ica.Archive(np.zeros((2, 1, 3, n), np.float32), dm_delay=np.array([0.5, 1.25, -3.0]))
        with pytest.raises(ValueError, match="power-of-two nbin"):
            dedispersion.plan(np.array([0.5, 1.25, -3.0]), n)
        with pytest.raises(ValueError, match="power-of-two nbin"):
            pr.rotate(np.zeros((1, 3, n), np.float32), np.zeros((2, 3, n // 2 + 1)), 1)


def test_plan_returns_fractional_delays_at_1000():
    from iterative_cleaner_amd import dedispersion
    d = np.array([0.0, 0.5, 999.25, -3.75])
    shift, delay = dedispersion.plan(d, 1000)
    assert np.array_equal(shift, np.zeros(4, np.int64)) and np.array_equal(delay, d)
    d2 = d[None, :] * (1.0 + 1e-6 * np.arange(3))[:, None]
    shift, delay = dedispersion.plan(d2, 1000)
    assert delay.shape == (3, 4) and np.array_equal(delay, d2)
    shift, delay = dedispersion.plan(np.array([0.0, 5.0, 1003.0]), 1000)
    assert delay is None and np.array_equal(shift, [0, 5, 3])


def test_foreign_psrfits_file_at_1000_bins_loads_with_dm_delays(tmp_path):
    """A PSRFITS file without the stand-in's columns (built as test_psrfits.py
    builds its unsupported case): psrchive's fractional delays from DM."""
    from iterative_cleaner_amd import dedispersion, psrfits, synth
    ar = synth.make_archive(2, 8, 1000, seed=4)
    ar._dm, ar._period = 30.0, 0.05
    ar._chan_freqs = 1400.0 + np.arange(8) * 10.0 - 35.0
    p = str(tmp_path / "mr.fits")
    psrfits.save(ar, p, stand_in_meta=False)
    br = psrfits.load(p)
    d = br.get_dm_delay()
    assert d is not None and np.any(d != np.rint(d))
    want = dedispersion.delays_from_dm(30.0, ar._chan_freqs, br.get_centre_frequency(), [0.05, 0.05], 1000)[0]
    assert np.array_equal(d, want)
    assert np.array_equal(br.get_dm_shift(), np.zeros(8, np.int64))
