"""8192-bin profiles on the GPU: k_diag_p2<8192> (8 waves per profile, four
radix-8 stages) and k_rotate<8192> (two radix-8 groups per lane, twiddles
through L1/L2) against the C oracle, under the rules of the shorter lengths:
std / mean / ptp, templates, amplitudes, status, weights and residuals bit for
bit (a NaN matches any NaN), fftmax and test values within 1e-9 relative.
The reference's own clean() at 8192 bins: the clean_s4x16x8192* fixtures, which
tests/test_gpu_parity.py takes as further cases.  nbin 16384 stays refused."""
import functools

import numpy as np
import pytest

from helpers import bits_equal, bits_equal_nan

pytestmark = pytest.mark.gpu

NBIN = 8192


def _same(a, b):
    """Bit-equal, except that NaNs only need to be NaN."""
    a = np.asarray(a)
    b = np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    nan = np.isnan(a) & np.isnan(b)
    ut = np.uint32 if a.dtype == np.float32 else np.uint64
    return bool(np.all((a.view(ut) == b.view(ut)) | nan))


def _close(a, b, tol=1e-9):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    fin = np.isfinite(a) & np.isfinite(b)
    return bool(np.all(same | (fin & (np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b))))))


# ------------------------------------------------------------------ rotation
def test_rotate_profiles_matches_oracle(oracle_lib):
    from iterative_cleaner_amd import _native
    rng = np.random.default_rng(NBIN)
    nsub, nchan = 3, 11
    d = rng.uniform(-5 * NBIN, 5 * NBIN, nchan)
    d[0], d[1], d[2] = 0.0, 7.0, 0.25
    d2 = rng.uniform(-5 * NBIN, 5 * NBIN, (nsub, nchan))
    d2[0, 0], d2[1, 1], d2[2, 2], d2[0, 3] = 0.0, 7.0, 0.25, -0.25
    x = (rng.standard_normal((nsub, nchan, NBIN)) * 50).astype(np.float32)
    x[0, 3, NBIN - 1] = np.nan
    x[1, 4, :] = 0.0
    x[2, 5, 2] = np.inf
    for delay in (d, d2):
        for sign in (1, -1):
            got = _native.rotate_profiles(x, delay, sign)
            assert _same(got, oracle_lib.rotate(x, delay, sign)), "sign %d, per-profile %s" % (sign, delay.ndim == 2)


def test_rotate_profiles_f32_edge_values(oracle_lib):
    """Subnormal, overflowing, signed-zero and spike profiles (the cube of
    tests/test_phase_rotation.py), per channel and per profile, both signs."""
    from test_phase_rotation import _edge_cube

    from iterative_cleaner_amd import _native
    x = _edge_cube(NBIN)
    rng = np.random.default_rng(NBIN + 1)
    d = rng.uniform(-2 * NBIN, 2 * NBIN, 6)
    d[1], d[2] = 0.0, 0.5
    d2 = rng.uniform(-2 * NBIN, 2 * NBIN, (4, 6))
    for delay in (d, d2):
        for sign in (1, -1):
            got = _native.rotate_profiles(x, delay, sign)
            assert _same(got, oracle_lib.rotate(x, delay, sign)), "sign %d, per-profile %s" % (sign, delay.ndim == 2)


# ---------------------------------------------------------------- statistics
def _check_stats(test, diags, ref_test, valid, ref_diags):
    """tests/test_stats_gpu.py's _check, with NaN diagnostics as NaN."""
    fin = np.isfinite(ref_test)
    assert np.array_equal(np.isnan(test), np.isnan(ref_test))
    assert np.array_equal(np.isinf(test), np.isinf(ref_test))
    assert np.all(np.abs(test[fin] - ref_test[fin]) <= 1e-9 * np.maximum(1, np.abs(ref_test[fin])))
    assert np.array_equal(test >= 1, ref_test >= 1)
    sd, mn, pt, ff = diags
    for name, got, want in (("std", sd, ref_diags[0]), ("mean", mn, ref_diags[1]), ("ptp", pt, ref_diags[2])):
        assert bits_equal_nan(np.where(valid, got, 0), np.where(valid, want, 0).astype(got.dtype)), name
    assert _close(ff, ref_diags[3])


@functools.lru_cache(maxsize=None)
def _stats_case(small):
    from oracle import lib as oracle_lib
    from oracle import restated as R
    oracle_lib.build()
    rng = np.random.default_rng(NBIN + (1 if small else 0))
    nsub, nchan = (5, 9) if small else (24, 70)
    X = rng.standard_normal((nsub, nchan, NBIN)).astype(np.float32)
    w = np.ones((nsub, nchan), np.float32)
    if small:       # non-finite rows, and one whose samples are all zero
        X[1, 2, 100] = np.nan
        X[3, 4, 5] = np.inf
        X[2, 6, NBIN - 1] = -np.inf
        X[4, 1, :] = 0.0
        w[0, 3] = 0.0
        w[1, 2] = 0.5
    else:           # lines with real medians (tests/test_stats_gpu.py's larger case)
        X[3, :, rng.integers(0, NBIN, 7)] += 60
        X[:, 11, :] += (20 * np.sin(np.arange(NBIN) * 0.3)).astype(np.float32)
        w[:, 5] = 0
        w[7, 9] = 0.5
    with np.errstate(invalid="ignore"):
        Xw = R.weighted_cube(X, w)
    diags = oracle_lib.diagnostics(Xw, w != 0)
    ref = oracle_lib.test_values(w != 0, *diags, 5, 5)
    return X, w, diags, ref


@pytest.mark.parametrize("waves", [0, 8])
@pytest.mark.parametrize("small", [False, True], ids=["24x70", "5x9_nonfinite"])
def test_stats_match_c_oracle(small, waves):
    from iterative_cleaner_amd import _native
    X, w, ref_diags, ref = _stats_case(small)
    test, diags = _native.comprehensive_stats(X, w, 5, 5, diagnostics=True, rowstat_waves=waves, rowstat_minlen=1)
    _check_stats(test, diags, ref, w != 0, ref_diags)


# ----------------------------------------------------------------------- fit
def test_fit_profiles_match_c_oracle(oracle_lib):
    """40 profiles against one template, exact (lmdif) and closed form: zero
    profiles, scaled templates plus noise, tiny and huge scales, a NaN sample;
    then a zero template."""
    from iterative_cleaner_amd import _native, synth
    data, w0, shift = synth.make_cube(4, 10, NBIN, 21, 0.3)
    D = oracle_lib.fit_cube(data[:, 0], w0, shift).reshape(-1, NBIN)
    T = oracle_lib.template(data[:, 0], w0, shift)
    rng = np.random.default_rng(5)
    D[3] = 0.0
    D[7] *= np.float32(1e-30)
    D[9] = (T * np.float32(1e12)).astype(np.float32)
    D[12] = (T * np.float32(-2.5) + rng.standard_normal(NBIN).astype(np.float32) * np.float32(0.1)).astype(np.float32)
    D[13] = T
    D[17, 4000] = np.nan
    for Tt, Dd in ((T, D), (np.zeros(NBIN, np.float32), D[:6])):
        amp, info, Rg = _native.fit_profiles(Dd, Tt)
        a_o, i_o, R_o = oracle_lib.fit_residual(Dd, Tt)
        assert bits_equal_nan(amp, a_o) and bits_equal(info, i_o) and _same(Rg, R_o)
        amp, info, Rg = _native.fit_profiles(Dd, Tt, fit_mode=_native.FIT_CLOSED)
        a_c, i_c, R_c = oracle_lib.fit_closed(Dd, Tt)
        assert bits_equal_nan(amp, a_c) and bits_equal(info, i_c) and _same(Rg, R_c)


# ------------------------------------------------------------ the whole loop
ARGS = dict(max_iter=5, chanthresh=5.0, subintthresh=5.0)
PULSE = [0.25, 2000, 3000]
# name -> (delays, closed form, f64 data, pulse region)
MODES = {
    "shift": (None, False, False, False),
    "fft": ("chan", False, False, False),
    "fft_pp": ("prof", False, False, False),
    "closed_shift": (None, True, False, False),
    "closed_fft": ("chan", True, False, False),
    "f64_shift": (None, False, True, False),
    "f64_fft": ("chan", False, True, False),
    "pulse_shift": (None, False, False, True),
    "pulse_fft_pp": ("prof", False, False, True),
}


@functools.lru_cache(maxsize=None)
def _cube():
    from iterative_cleaner_amd import synth
    data, w0, shift = synth.make_cube(5, 24, NBIN, 31, 0.2)
    return np.ascontiguousarray(data[:, 0]), w0, shift


def _delay(kind):
    from iterative_cleaner_amd import synth
    raw, w0, shift = _cube()
    if kind is None:
        return None
    return synth.fractional_delays(shift, NBIN) if kind == "chan" else synth.per_profile_delays(shift, NBIN, 5)


def _run(mode, options=None, fit_tail=None):
    from iterative_cleaner_amd import _native
    kind, closed, f64, pulse = MODES[mode]
    raw, w0, shift = _cube()
    delay = _delay(kind)
    with _native.GpuSession(5, 24, NBIN, ARGS["max_iter"], ARGS["chanthresh"], ARGS["subintthresh"],
                            PULSE if pulse else [0, 0, 1], device=0, delay=delay, data_f64=f64,
                            fit_mode=_native.FIT_CLOSED if closed else _native.FIT_EXACT, options=options) as s:
        if fit_tail is not None:
            s.set_fit_tail(fit_tail)
        s.upload(raw, w0, shift if delay is None else np.zeros(24, np.int32))
        out = s.run()
        out["T"] = s.template()
        out["amp"], out["info"] = s.fit()
        out["diag"] = s.diagnostics()
        out["R"] = s.residual()
    return out


@functools.lru_cache(maxsize=None)
def _default(mode):
    return _run(mode)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_loop_matches_c_oracle(mode, oracle_lib):
    """What tests/test_fft_dedisp_gpu.py::test_fft_loop_matches_c_oracle
    compares, in every mode of the session."""
    from iterative_cleaner_amd import _native
    kind, closed, f64, pulse = MODES[mode]
    raw, w0, shift = _cube()
    pr = None
    if pulse:
        _, fac, a, b = _native.normalise_pulse_region(PULSE, NBIN)
        pr = (fac, a, b)
    ref = oracle_lib.clean_loop(raw, w0, shift, ARGS["chanthresh"], ARGS["subintthresh"], ARGS["max_iter"], pr,
                                want_residual=True, want_details=True, fit_mode=1 if closed else 0, data_f64=f64,
                                delay=_delay(kind))
    assert ref["loops"] > 1 and np.any(ref["weights"] != w0)      # the case does clean something
    out = _default(mode)
    sd, mn, pt, ff = out["diag"]
    assert out["loops"] == ref["loops"]
    assert np.array_equal(out["changed"], ref["changed"][:out["n_iter"]])
    assert bits_equal(out["T"], ref["T"][out["n_iter"] - 1])
    assert bits_equal(out["amp"], ref["amp"]) and bits_equal(out["info"], ref["info"])
    assert bits_equal(out["weights"], ref["weights"])
    assert bits_equal(sd, ref["std"]) and bits_equal(mn, ref["mean"]) and bits_equal(pt, ref["ptp"])
    assert _close(ff, ref["fft"]) and _close(out["test"], ref["test"])
    assert _same(out["R"], ref["residual"])


SETTINGS = [
    # (options, fit_tail)
    ({}, 0),
    ({}, 16),
    ({"diag_fork": 0}, None),
    ({"diag_fork": 1}, None),
    ({"diag_fork": 3}, None),
    ({"template_incr": 0}, None),
    ({"fit_tiled": 0}, None),
    ({"grid_cap": 2}, None),
]


@pytest.mark.parametrize("mode", ["shift", "fft_pp"])
def test_schedules_are_bit_identical(mode):
    """Every schedule setting gives the default's bits (which
    test_loop_matches_c_oracle compares with the oracle): the tail at once and
    late, the diagnostics fork off / early / at round 3 (the kernels then take
    profile lists), full template passes, the row-major fit cube, and a grid of
    two blocks, under which every grid-stride loop runs several trips."""
    base = _default(mode)
    for opts, tail in SETTINGS:
        got = _run(mode, opts, tail)
        what = (mode, opts, tail)
        assert got["loops"] == base["loops"] and np.array_equal(got["changed"], base["changed"]), what
        for key in ("weights", "test", "T", "amp", "info"):
            assert bits_equal(got[key], base[key]), (what, key)
        for x0, x1 in zip(base["diag"], got["diag"]):
            assert bits_equal(x1, x0), what
        assert _same(got["R"], base["R"]), what


def test_two_local_shards_match_one_session():
    """A two-super-block archive (300 channels) in the FFT mode as two
    in-process channel shards: the merged weights are one session's."""
    from iterative_cleaner_amd import _native, sharded, synth
    nsub, nchan = 3, 300
    data, w0, shift = synth.make_cube(nsub, nchan, NBIN, 77, 0.2)
    delay = synth.fractional_delays(shift, NBIN)
    raw = np.ascontiguousarray(data[:, 0])
    zero = np.zeros(nchan, np.int32)
    with _native.GpuSession(nsub, nchan, NBIN, device=0, delay=delay) as s:
        s.upload(raw, w0, zero)
        one = s.run()
    out = sharded.clean_cube_local(raw, w0, zero, 2, delay=delay)
    assert out["loops"] == one["loops"] and np.array_equal(out["changed"], one["changed"])
    assert bits_equal(out["weights"], one["weights"]) and bits_equal(out["test"], one["test"])


def test_cli_foreign_psrfits_fractional_dedispersion(tmp_path, monkeypatch, capsys, oracle_lib):
    """The CLI on a PSRFITS file of 8192-bin profiles without the stand-in's
    columns: fractional delays from the DM, the quantised samples uploaded as
    stored; the zap mask equals the C oracle's loop on the decoded samples
    (as tests/test_psrfits_gpu.py at 256 bins)."""
    from iterative_cleaner_amd import archive as ica
    from iterative_cleaner_amd import cleaner, dedispersion, psrfits, synth
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("IC_DEDISPERSION", raising=False)
    nsub, nchan = 6, 16
    data, w, shift = synth.make_cube(nsub, nchan, NBIN, 61, 0.2, npol=2)
    ar = ica.Archive(data, w, np.zeros(nchan, np.int64), filename="dm.sf")
    ar._chan_freqs = 1300.0 + np.arange(nchan) * 3.0
    ar._period = 0.0125
    ar._dm = 20.0
    psrfits.save(ar, "dm.sf", stand_in_meta=False)
    src = psrfits.load("dm.sf")
    delay = src.get_dm_delay()
    assert delay is not None and delay.shape == (nchan,) and np.any(delay != np.rint(delay))
    assert np.array_equal(delay, dedispersion.delays_from_dm(20.0, ar._chan_freqs, 1400.0, [0.0125] * nsub, NBIN)[0])
    dec = src.get_data()
    cube = (dec[:, 0] + dec[:, 1]).astype(np.float32)
    ref = oracle_lib.clean_loop(cube, src.get_weights(), src.get_dm_shift(), delay=delay)
    cleaner.main(cleaner.parse_arguments(["-l", "-q", "dm.sf"]))
    res = ica.Archive_load("dm_cleaned.ar")
    assert bits_equal(res.get_weights(), ref["weights"])
    assert np.any(ref["weights"] != src.get_weights())


def test_longer_profiles_stay_refused():
    from iterative_cleaner_amd import _native
    with pytest.raises(_native.NativeError, match="power-of-two"):
        _native.GpuSession(2, 4, 16384, device=0, delay=np.full(4, 0.5))
    with pytest.raises(_native.NativeError, match="LDS"):
        _native.GpuSession(2, 4, 16384, device=0)
    with pytest.raises(_native.NativeError, match="power-of-two"):
        _native.rotate_profiles(np.zeros((2, 3, 16384), np.float32), np.full(3, 0.5))
