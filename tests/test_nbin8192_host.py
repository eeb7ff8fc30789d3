"""8192-bin profiles on the host side: the dedispersion plan, the PSRFITS reader
and the psrchive-like path accept fractional delays at nbin 8192 (and still
refuse 16384 and the non-powers of two), and the stand-in's written-order
rotation equals the C oracle's at that length, bit for bit, within 4 f32
epsilons of numpy's f64 rotation (the bound of tests/test_phase_rotation.py).
The reference's own clean() at 8192 bins is pinned by the clean_s4x16x8192*
fixtures, which tests/test_oracle_golden.py takes as further cases."""
import numpy as np
import pytest

from helpers import nan_equal

NBIN = 8192


def test_plan_accepts_fractional_delays_at_8192():
    from iterative_cleaner_amd import dedispersion
    assert dedispersion.fft_supported(NBIN)
    rng = np.random.default_rng(1)
    d = rng.uniform(-3 * NBIN, 3 * NBIN, 12)
    shift, delay = dedispersion.plan(d, NBIN)
    assert np.array_equal(shift, np.zeros(12, np.int64)) and np.array_equal(delay, d) and delay.shape == (12,)
    shift, delay = dedispersion.plan(np.broadcast_to(d, (5, 12)), NBIN)     # equal rows: one delay per channel
    assert delay.shape == (12,) and np.array_equal(delay, d)
    d2 = d[None, :] * (1.0 + 1e-6 * np.arange(5))[:, None]
    shift, delay = dedispersion.plan(d2, NBIN)
    assert np.array_equal(shift, np.zeros(12, np.int64)) and delay.shape == (5, 12) and np.array_equal(delay, d2)
    # integral delays stay integer shifts
    shift, delay = dedispersion.plan(np.array([0.0, 5.0, NBIN + 3.0]), NBIN)
    assert delay is None and np.array_equal(shift, [0, 5, 3])


@pytest.mark.parametrize("nbin", [100, 32, 16384])
def test_plan_still_refuses_other_lengths(nbin):
    from iterative_cleaner_amd import dedispersion
    assert not dedispersion.fft_supported(nbin)
    with pytest.raises(ValueError, match="power-of-two nbin"):
        dedispersion.plan(np.array([0.25, 1.5, 7.0]), nbin)


def test_foreign_psrfits_file_loads_at_8192(tmp_path):
    """A PSRFITS file without the stand-in's columns (DM 30, period 0.05, eight
    channels near 1400 MHz, as tests/test_psrfits.py builds its unsupported-nbin
    case): its fractional delays come from the DM and are kept."""
    from iterative_cleaner_amd import dedispersion, psrfits, synth
    ar = synth.make_archive(2, 8, NBIN, seed=4)
    ar._dm, ar._period = 30.0, 0.05
    ar._chan_freqs = 1400.0 + np.arange(8) * 10.0 - 35.0
    p = str(tmp_path / "u.fits")
    psrfits.save(ar, p, stand_in_meta=False)
    br = psrfits.load(p)
    assert br.get_nbin() == NBIN
    d = br.get_dm_delay()
    assert d is not None and d.shape == (8,) and np.any(d != np.rint(d))
    assert np.array_equal(d, dedispersion.delays_from_dm(30.0, ar._chan_freqs, 1400.0, [0.05, 0.05], NBIN)[0])
    assert np.array_equal(br.get_dm_shift(), np.zeros(8, np.int64))


def test_dedispersion_of_a_psrchive_like_archive_at_8192():
    from psrchive_like import PsrchiveLike

    from iterative_cleaner_amd import cleaner, dedispersion
    data = np.zeros((4, 1, 6, NBIN), np.float32)
    w = np.ones((4, 6), np.float32)
    freqs = 150.0 + np.arange(6) * 0.5
    per = np.array([0.1, 0.1000001, 0.0999999, 0.1])
    shift, delay = cleaner._dedispersion(PsrchiveLike(data, w, 12.0, freqs, per, 151.0))
    assert np.array_equal(shift, np.zeros(6)) and delay.shape == (4, 6)
    assert np.array_equal(delay, dedispersion.delays_from_dm(12.0, freqs, 151.0, per, NBIN))
    shift, delay = cleaner._dedispersion(PsrchiveLike(data, w, 12.0, freqs, np.full(4, 0.1), 151.0))
    assert delay.shape == (6,)
    with pytest.raises(ValueError, match="power-of-two nbin"):
        cleaner._dedispersion(PsrchiveLike(np.zeros((4, 1, 6, 16384), np.float32), w, 12.0, freqs, per, 151.0))


def _signs_equal(a, c):
    # NaN payloads/signs are not part of the definition (tests/test_phase_rotation.py)
    return nan_equal(a, c) and np.array_equal(np.signbit(a) | np.isnan(a), np.signbit(c) | np.isnan(c))


def test_rotation_matches_c_oracle_at_8192(oracle_lib):
    """Tables and rotation, per channel (with and without the level
    subtraction, a NaN, an Inf and an all-zero profile) and per profile."""
    from test_phase_rotation import _case

    from iterative_cleaner_amd import phase_rotation as pr
    x, d, b = _case(NBIN)
    assert np.array_equal(pr.twiddles(NBIN), oracle_lib.twiddles(NBIN))
    ph = pr.phasors(NBIN, d)
    assert np.array_equal(ph, oracle_lib.phasors(NBIN, d))
    d2 = np.random.default_rng(NBIN).uniform(-2 * NBIN, 2 * NBIN, x.shape[:2])
    d2[0, 0], d2[1, 1] = 0.0, 0.25
    for sign in (1, -1):
        for base in (None, b):
            assert _signs_equal(pr.rotate(x, ph, sign, base=base), oracle_lib.rotate(x, d, sign, base=base))
        assert _signs_equal(pr.rotate(x, pr.phasors(NBIN, d2), sign), oracle_lib.rotate(x, d2, sign))


def test_rotation_within_f32_error_of_numpy_fft_at_8192(oracle_lib):
    """The bound of tests/test_phase_rotation.py (4 f32 epsilons of the
    profile's largest |sample|) against numpy's f64 irfft(rfft(x) * phasor)."""
    from oracle.restated import fft_phase_shift
    rng = np.random.default_rng(NBIN)
    d = rng.uniform(-3 * NBIN, 3 * NBIN, 16)
    x = (rng.standard_normal((4, 16, NBIN)) * 10 + 3).astype(np.float32)
    eps = float(np.finfo(np.float32).eps)
    scale = np.max(np.abs(x), axis=-1, keepdims=True).astype(np.float64)
    for sign in (1, -1):
        got = oracle_lib.rotate(x, d, sign)
        want = fft_phase_shift(x, d, sign)
        assert np.all(np.abs(got.astype(np.float64) - want) <= 4 * eps * scale)
