"""The diagnostics at the profile lengths that are neither a power of two nor
mixed-radix, on the GPU (k_diag_czt: 129..4096, odd and prime lengths up to
2048 included; the lengths below its measured lower bound, 16..125 here, keep
the generic k_diag and pass the same checks, as the odd lengths above 2048 do).

std / mean / ptp, the closed-form amplitude and its status are pinned bit for
bit (a NaN matches a NaN) to the C oracle, whose sums are numpy's pairwise sums,
and for rows of finite samples to oracle/restated.py's numpy statement itself.
fftmax is pinned within 1e-9 relative to numpy's rfft; the test values follow
from the four diagnostics, so they carry its 1e-9 (tests/test_stats_gpu.py).

The fork test is the one that fails without the kernel: the generic k_diag
takes no profile list, so diag_fork resolves to the unforked schedule at these
lengths and launches k_diag once per iteration whatever the option says.

The recipes are tests/test_diag_mr_gpu.py's."""
import numpy as np
import pytest

from helpers import bits_equal, bits_equal_nan, nan_equal
from test_diag_mr_gpu import PULSE, _same_run
from test_fast_mode_gpu import _close
from test_stats_gpu import _check

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- 1. one-shot statistics

# k_diag_czt from 250 on: one wave per profile (250, 448, 500, 510: L <= 512),
# 2, 4 and 8 waves around one work array (514; 997; 2047, 2050, 2500, 4094), an
# odd half length (250), odd and prime lengths (997, 2047), 33 pairwise leaves
# (4094); 16..125 are the generic kernel's
@pytest.mark.parametrize("nbin", [16, 17, 18, 50, 100, 125, 250, 448, 500, 510, 514, 997, 2047, 2050, 2500, 4094])
def test_one_shot_statistics(nbin, oracle_lib):
    """5 x 7 profiles (a partial last block at every block size) of N(0, 50^2)
    with a zero-weight profile, an all-zero row, a constant row, a row with a
    NaN at its last sample, a row with +Inf and a fractional weight."""
    from oracle import restated as R

    from iterative_cleaner_amd import _native
    rng = np.random.default_rng(nbin)
    nsub, nchan = 5, 7
    X = (rng.standard_normal((nsub, nchan, nbin)) * 50).astype(np.float32)
    w = np.ones((nsub, nchan), np.float32)
    w[1, 2] = 0.0
    X[0, 3, :] = 0.0
    X[2, 4, :] = 3.5
    X[3, 1, nbin - 1] = np.nan
    X[4, 5, 2] = np.inf
    w[2, 6] = 0.5
    valid = w != 0
    test, (sd, mn, pt, ff) = _native.comprehensive_stats(X, w, 5, 5, diagnostics=True)
    Xw = R.weighted_cube(X, w)
    with np.errstate(all="ignore"):
        osd, omn, opt, off = oracle_lib.diagnostics(Xw, valid)
        nsd, nmn, npt, _ = R.diagnostics(Xw, valid)
    for name, got, want in (("std", sd, osd), ("mean", mn, omn), ("ptp", pt, opt)):
        assert bits_equal_nan(got, want), name
    finite = np.isfinite(Xw).all(axis=-1)
    assert finite.sum() == nsub * nchan - 2
    for name, got, want in (("std", sd, nsd), ("mean", mn, nmn), ("ptp", pt, npt)):
        assert bits_equal(got[finite], want[finite].astype(got.dtype)), name
    # fftmax: max |rfft(v)|, v = f64(X) - mean (valid) or f64(X) (zero weight)
    with np.errstate(all="ignore"):
        v = Xw.astype(np.float64) - np.where(valid, mn, 0.0)[..., None]
        want = np.abs(np.fft.rfft(v, axis=-1)).max(axis=-1)
    assert np.array_equal(np.isnan(ff), ~finite)
    floor = nbin * 2.0 ** -52 * np.abs(Xw).max(axis=-1)
    flat = np.zeros((nsub, nchan), bool)
    flat[0, 3] = flat[2, 4] = flat[1, 2] = True
    err = np.abs(ff - want)
    print("nbin", nbin, "max rel fftmax error", np.nanmax(err[finite & ~flat] / want[finite & ~flat]))
    assert ff[0, 3] == 0.0 and ff[1, 2] == 0.0
    assert np.all(err[finite & ~flat] <= 1e-9 * want[finite & ~flat])
    assert np.all(err[flat] <= 1e-9 * want[flat] + floor[flat])
    ref = oracle_lib.test_values(valid, osd, omn, opt, off, 5, 5)
    _check(test, (sd, mn, pt, ff), ref, valid)


# ---------------------------------------------------------------- 2. the loop against the C oracle

def _loop(oracle_lib, shape, seed, pulse=False, fit_mode=0, data_f64=False):
    from iterative_cleaner_amd import _native, synth
    nsub, nchan, nbin = shape
    data, w0, shift = synth.make_cube(nsub, nchan, nbin, seed, 0.2)
    raw = np.ascontiguousarray(data[:, 0])
    pr = None
    if pulse:
        _, fac, a, b = _native.normalise_pulse_region(PULSE, nbin)
        pr = (fac, a, b)
    ref = oracle_lib.clean_loop(raw, w0, shift, 5.0, 5.0, 5, pr, want_residual=True, want_details=True,
                                fit_mode=fit_mode, data_f64=data_f64)
    with _native.GpuSession(nsub, nchan, nbin, 5, 5.0, 5.0, PULSE if pulse else [0, 0, 1], device=0,
                            fit_mode=_native.FIT_CLOSED if fit_mode else _native.FIT_EXACT,
                            data_f64=data_f64) as s:
        s.upload(raw, w0, shift)
        out = s.run()
        out["T"] = s.template()
        out["amp"], out["info"] = s.fit()
        out["diag"] = s.diagnostics()
        out["R"] = s.residual()
    return out, ref


@pytest.mark.parametrize("pulse", [False, True], ids=["plain", "pulse"])
@pytest.mark.parametrize("shape", [(6, 40, 100), (5, 20, 125), (4, 16, 500), (3, 12, 2500)],
                         ids=lambda s: "%dx%dx%d" % s)
def test_exact_loop_matches_c_oracle(shape, pulse, oracle_lib):
    """Integer shifts, the default (forked) schedule; the tiled fit cube."""
    out, ref = _loop(oracle_lib, shape, 9, pulse)
    diag = out["diag"]
    assert out["loops"] == ref["loops"]
    assert bits_equal(out["weights"], ref["weights"])
    assert bits_equal(out["amp"], ref["amp"]) and bits_equal(out["info"], ref["info"])
    for name, x in zip(("std", "mean", "ptp"), diag[:3]):
        assert nan_equal(x, ref[name]) and x.dtype == ref[name].dtype, name
    assert bits_equal(out["R"], ref["residual"])
    ff = ref["fft"]
    nz = ff != 0   # zero-weight profiles: 0 on both sides
    print(shape, pulse, "max rel fftmax error", np.max(np.abs(diag[3] - ff)[nz] / np.abs(ff)[nz]))
    assert np.all(np.abs(diag[3] - ff) <= 1e-9 * np.abs(ff)), "fftmax"
    assert _close(out["test"], ref["test"], 1e-9)


def test_closed_form_loop_matches_c_oracle_500(oracle_lib):
    """fit_mode 1 with integer shifts (DIAG_CLOSED), tests/test_fast_mode_gpu.py's comparisons."""
    out, ref = _loop(oracle_lib, (5, 33, 500), 12, fit_mode=1)
    sd, mn, pt, ff = out["diag"]
    assert out["loops"] == ref["loops"]
    assert bits_equal(out["T"], ref["T"][out["n_iter"] - 1])
    assert bits_equal(out["amp"], ref["amp"]) and bits_equal(out["info"], ref["info"])
    assert bits_equal(out["weights"], ref["weights"])
    assert np.array_equal(out["changed"], ref["changed"][:out["n_iter"]])
    assert bits_equal(sd, ref["std"]) and bits_equal(mn, ref["mean"]) and bits_equal(pt, ref["ptp"])
    assert _close(ff, ref["fft"], 1e-9)
    assert _close(out["test"], ref["test"], 1e-9)
    assert bits_equal(out["R"], ref["residual"])


@pytest.mark.parametrize("shape", [(6, 40, 56), (6, 40, 250), (4, 20, 500), (3, 16, 514)],
                         ids=lambda s: "%dx%dx%d" % s)
def test_f64_data_loop_matches_c_oracle(shape, oracle_lib):
    """data_f64: X = f64(R) * f64(w), f64 pairwise mean and f64 ptp.  56 bins
    are the generic kernel's; 250, 500 and 514 are k_diag_czt's three f64
    instantiations (4 and 8 points per thread, several waves)."""
    out, ref = _loop(oracle_lib, shape, 5, data_f64=True)
    diag = out["diag"]
    assert out["loops"] == ref["loops"]
    assert bits_equal(out["weights"], ref["weights"])
    assert bits_equal(out["amp"], ref["amp"]) and bits_equal(out["info"], ref["info"])
    for name, x in zip(("std", "mean", "ptp"), diag[:3]):
        assert nan_equal(x, ref[name]) and x.dtype == ref[name].dtype == np.float64, name
    ff = ref["fft"]
    assert np.all(np.abs(diag[3] - ff) <= 1e-9 * np.abs(ff)), "fftmax"
    assert _close(out["test"], ref["test"], 1e-9)


# ---------------------------------------------------------------- 3. the fork

_FORK = {}


def _fork_run(shape, mode, options, tail):
    """mode: 'int' (integer shifts), 'fft' (per-channel delays), 'fft_pp'
    (per-profile delays); the two FFT modes are the opt-in any-length mode."""
    from iterative_cleaner_amd import _native, synth
    key = (shape, mode, tuple(sorted(options.items())), tail)
    if key in _FORK:
        return _FORK[key]
    nsub, nchan, nbin = shape
    data, w0, shift = synth.make_cube(nsub, nchan, nbin, 5, 0.1)
    raw = np.ascontiguousarray(data[:, 0])
    delay = None
    if mode == "fft":
        delay = synth.fractional_delays(shift, nbin)
    elif mode == "fft_pp":
        delay = synth.per_profile_delays(shift, nbin, nsub)
    with _native.GpuSession(nsub, nchan, nbin, max_iter=5, device=0, delay=delay, options=options,
                            any_length=delay is not None) as s:
        s.set_fit_tail(tail)
        s.set_timing(True)
        s.upload(raw, w0, np.zeros_like(shift) if delay is not None else shift)
        out = s.run()
        out["amp"], out["info"] = s.fit()
        out["diag"] = s.diagnostics()
        out["launches"] = s.kernel_times()["k_diag"]["launches"]
    _FORK[key] = out
    return out


@pytest.mark.parametrize("mode", ["int", "fft", "fft_pp"])
@pytest.mark.parametrize("shape", [(16, 256, 500), (8, 256, 250)], ids=lambda s: "%dx%dx%d" % s)
def test_fork_engages_and_changes_no_bit(shape, mode):
    """Rounds only (fit tail 0): the forked schedule launches the diagnostics
    kernel more often than the unforked one (pass A on the second stream, pass
    B from the round list) and every output keeps its bits, fftmax included; so
    do a fit tail of 512 with tail_split 0 and 1, and a grid of one block."""
    ref = _fork_run(shape, mode, {"diag_fork": 0}, 0)
    one = _fork_run(shape, mode, {"diag_fork": 1}, 0)
    print(shape, mode, "k_diag launches: unforked", ref["launches"], "diag_fork=1", one["launches"])
    assert one["launches"] > ref["launches"]
    for fork in (1, 3, 5):
        _same_run(_fork_run(shape, mode, {"diag_fork": fork}, 0), ref, ("fork", fork))
        for split in (0, 1):
            got = _fork_run(shape, mode, {"diag_fork": fork, "tail_split": split}, 512)
            _same_run(got, ref, ("fork", fork, "tail 512, split", split))
    _same_run(_fork_run(shape, mode, {"grid_cap": 1}, 0), ref, "grid_cap 1")
    _same_run(_fork_run(shape, mode, {"grid_cap": 1, "diag_fork": 0}, 0), ref, "grid_cap 1 unforked")


# ---------------------------------------------------------------- 4. shards

def test_two_local_shards_equal_one_session_integer_mode():
    """Integer shifts at 100 bins; 600 channels are three 256-channel
    super-blocks, split 2 + 1.  The run zaps something."""
    from iterative_cleaner_amd import _native, sharded, synth
    nsub, nchan, nbin = 6, 600, 100
    data, w0, shift = synth.make_cube(nsub, nchan, nbin, 91, 0.2)
    raw = np.ascontiguousarray(data[:, 0])
    with _native.GpuSession(nsub, nchan, nbin, device=0) as s:
        s.upload(raw, w0, shift)
        one = s.run()
        one["amp"], one["info"] = s.fit()
        one["std"], one["mean"], one["ptp"], one["fft"] = s.diagnostics()
    assert int((one["weights"] == 0).sum()) > int((w0 == 0).sum())
    out = sharded.clean_cube_local(raw, w0, shift, 2, want_details=True)
    assert out["loops"] == one["loops"] and np.array_equal(out["changed"], one["changed"])
    for key in ("weights", "test", "amp", "info", "std", "mean", "ptp", "fft"):
        assert bits_equal(out[key], one[key]), key
