"""The opt-in chirp-z rotation on the GPU (k_rotate_czt, IC_DEDISP_FFT_ANY,
ic_rotate_profiles_any): fractional dedispersion at any profile length in
16..4096 that the default kernels do not serve.

The yardsticks are the numpy statement (phase_rotation.rotate_czt: the one-shot
rotation must carry its bits) and the reference's own clean() on stand-in
archives of these lengths (tests/golden/any_clean_*.npz, made by
tests/golden/make_golden_any.py), compared with the rules of
tests/test_gpu_parity.py: template, amplitudes, status, std / mean / ptp and
weights bit for bit, fftmax within 1e-9 relative.  Every test here fails where
the library has no IC_DEDISP_FFT_ANY / ic_rotate_profiles_any."""
import os

import numpy as np
import pytest

from helpers import GOLDEN, bits_equal, bits_equal_nan, load_clean_case
from test_fft_dedisp_gpu import _same
from test_fft_mr_gpu import SCHEDULES

pytestmark = pytest.mark.gpu

SWITCH = "IC_ANY_NBIN"
ANY_FIXTURES = ["s6x24x100_fft", "s5x20x125_fft_pp_u", "s4x16x500_fft_pr", "s4x12x448_fft_ded", "s6x20x56_fft_f64"]


def _fixture(name):
    return os.path.join(GOLDEN, "any_clean_%s.npz" % name)


def _inputs(nbin):
    """The inputs of test_fft_mr_gpu.test_rotate_profiles_carries_the_definitions_bits."""
    rng = np.random.default_rng(nbin)
    nsub, nchan = 5, 7
    d = rng.uniform(-5 * nbin, 5 * nbin, nchan)
    d[0], d[1], d[2] = 0.0, 7.0, 0.25
    d2 = rng.uniform(-5 * nbin, 5 * nbin, (nsub, nchan))
    d2[0, 0], d2[1, 1] = 0.0, 64.0
    x = (rng.standard_normal((nsub, nchan, nbin)) * 50).astype(np.float32)
    x[0, 3, nbin - 1] = np.nan
    x[1, 4, :] = 0.0
    x[2, 5, 2] = np.inf
    b = rng.standard_normal((nsub, nchan)).astype(np.float32)
    return x, b, d, d2


# ---------------------------------------------------------------- 1. one-shot rotation

@pytest.mark.parametrize("nbin", [16, 33, 100, 125, 129, 448, 997, 1002, 2047])
def test_rotate_profiles_carries_the_definitions_bits(nbin):
    """5 x 7 profiles, per channel and per profile, both signs, with and
    without a baseline level (subtracted in f32 first: the statement's step 1).
    The smallest n of each L and just above a power of two (16, 33, 129), the
    fullest buffer (2047: 4093 of 4096 points), rows that are odd or no
    multiple of 4 (33, 125, 129, 997, 1002, 2047), a prime (997)."""
    from iterative_cleaner_amd import _native
    from iterative_cleaner_amd import phase_rotation as pr
    x, b, d, d2 = _inputs(nbin)
    xb = (x - b[..., None]).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for delay in (d, d2):
            ph = pr.phasors(nbin, delay)
            for sign in (1, -1):
                want = pr.rotate_czt(x, ph, sign)
                assert _same(_native.rotate_profiles(x, delay, sign, any_length=True), want), (delay.ndim, sign)
                assert _same(_native.rotate_profiles(xb, delay, sign, any_length=True),
                             pr.rotate_czt(x, ph, sign, base=b)), (delay.ndim, sign)
        assert _same(pr.rotate(x, pr.phasors(nbin, d), 1, any_length=True), pr.rotate_czt(x, pr.phasors(nbin, d), 1))


@pytest.mark.parametrize("nbin,per_profile,sign", [(2049, False, 1), (4095, True, -1)])
def test_rotate_profiles_at_the_longest_convolution(nbin, per_profile, sign):
    """L = 8192: the twiddle table is read from global memory."""
    from iterative_cleaner_amd import _native
    from iterative_cleaner_amd import phase_rotation as pr
    x, b, d, d2 = _inputs(nbin)
    delay = d2 if per_profile else d
    with np.errstate(invalid="ignore", over="ignore"):
        want = pr.rotate_czt(x, pr.phasors(nbin, delay), sign)
    assert _same(_native.rotate_profiles(x, delay, sign, any_length=True), want)


def test_rotate_profiles_f32_edge_values():
    """Subnormal, overflowing, signed-zero and spike profiles at 125 bins."""
    from iterative_cleaner_amd import _native
    from iterative_cleaner_amd import phase_rotation as pr
    from test_phase_rotation import _edge_cube
    nbin = 125
    x = _edge_cube(nbin)
    rng = np.random.default_rng(nbin + 1)
    d = rng.uniform(-2 * nbin, 2 * nbin, 6)
    d[1], d[2] = 0.0, 0.5
    d2 = rng.uniform(-2 * nbin, 2 * nbin, (4, 6))
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for delay in (d, d2):
            ph = pr.phasors(nbin, delay)
            for sign in (1, -1):
                assert _same(_native.rotate_profiles(x, delay, sign, any_length=True),
                             pr.rotate_czt(x, ph, sign)), (delay.ndim, sign)


@pytest.mark.parametrize("nbin", [128, 200])
def test_served_lengths_keep_their_kernels_bits(nbin):
    from iterative_cleaner_amd import _native
    x, b, d, d2 = _inputs(nbin)
    for delay in (d, d2):
        for sign in (1, -1):
            assert _same(_native.rotate_profiles(x, delay, sign, any_length=True),
                         _native.rotate_profiles(x, delay, sign)), (delay.ndim, sign)


# ---------------------------------------------------------------- 2. the reference's loop

@pytest.mark.parametrize("name", ANY_FIXTURES)
def test_loop_matches_reference_fixture(name, monkeypatch):
    import test_gpu_parity as parity
    monkeypatch.setenv(SWITCH, "1")
    parity.test_loop_matches_reference(_fixture(name), "default")
    parity.test_every_iteration_matches_reference(_fixture(name))


@pytest.mark.parametrize("name", ["s6x24x100_fft", "s4x16x500_fft_pr"])
def test_loop_matches_reference_fixture_rounds_and_tail(name, monkeypatch):
    import test_gpu_parity as parity
    monkeypatch.setenv(SWITCH, "1")
    for fit_mode in ("rounds", "tail"):
        parity.test_loop_matches_reference(_fixture(name), fit_mode)


@pytest.mark.parametrize("name", ANY_FIXTURES)
def test_clean_stdout_final_weights_and_residual_archive(name, tmp_path, monkeypatch, capsys):
    import test_gpu_parity as parity
    monkeypatch.setenv(SWITCH, "1")
    parity.test_clean_stdout_matches_reference(_fixture(name), tmp_path, monkeypatch, capsys)


# ---------------------------------------------------------------- 3. schedules

def _run_500(options, fit_tail=None):
    from iterative_cleaner_amd import _native
    z, meta, raw, w0, shift, args = load_clean_case(_fixture("s4x16x500_fft_pr"))
    nsub, nchan, nbin = raw.shape
    with _native.GpuSession(nsub, nchan, nbin, args["max_iter"], args["chanthresh"], args["subintthresh"],
                            args["pulse_region"], device=0, delay=z["dm_delay"], options=options,
                            any_length=True) as s:
        if fit_tail is not None:
            s.set_fit_tail(fit_tail)
        s.upload(raw, w0, shift)
        out = s.run()
        out["T"] = s.template()
        out["amp"], out["info"] = s.fit()
        out["diag"] = s.diagnostics()
        out["R"] = s.residual()
    return out


def test_schedules_are_bit_identical():
    """The SCHEDULES of test_fft_mr_gpu.py at the 500-bin fixture; grid_cap = 1
    drives k_rotate_czt's grid-stride loop through 64 profiles on one block."""
    base = _run_500({})
    for options, tail in SCHEDULES:
        got = _run_500(options, tail)
        assert got["loops"] == base["loops"] and np.array_equal(got["changed"], base["changed"]), options
        for key in ("weights", "test", "T", "amp", "info"):
            assert bits_equal(got[key], base[key]), (options, key)
        for x0, x1 in zip(base["diag"], got["diag"]):
            assert bits_equal(x1, x0), options
        assert _same(got["R"], base["R"]), options


def test_grid_cap_one_rotation_at_129():
    """The one-shot entry point takes no grid cap, so the repeat at 129 bins is
    a session's: grid_cap = 1 (35 profiles on one block of three waves: twelve
    trips of k_rotate_czt's grid-stride loop, in every rotation of the loop)
    gives the bits of the uncapped grid."""
    from iterative_cleaner_amd import _native, synth
    nsub, nchan, nbin = 5, 7, 129
    data, w0, shift = synth.make_cube(nsub, nchan, nbin, 17, 0.2)
    raw = np.ascontiguousarray(data[:, 0])
    delay = synth.fractional_delays(shift, nbin)
    outs = []
    for options in ({}, {"grid_cap": 1}):
        with _native.GpuSession(nsub, nchan, nbin, device=0, delay=delay, options=options, any_length=True) as s:
            s.upload(raw, w0, np.zeros(nchan, np.int32))
            out = s.run()
            out["R"] = s.residual()
            out["T"] = s.template()
            outs.append(out)
    assert bits_equal(outs[0]["weights"], outs[1]["weights"]) and bits_equal_nan(outs[0]["test"], outs[1]["test"])
    assert bits_equal(outs[0]["T"], outs[1]["T"]) and _same(outs[0]["R"], outs[1]["R"])


# ---------------------------------------------------------------- 4. shards and batch

def test_two_local_shards_equal_one_session():
    """Per-profile delays at 100 bins; 600 channels: three super-blocks, split 2 + 1."""
    from iterative_cleaner_amd import _native, sharded, synth
    nsub, nchan, nbin = 6, 600, 100
    data, w0, shift = synth.make_cube(nsub, nchan, nbin, 91, 0.2)
    delay = synth.per_profile_delays(shift, nbin, nsub)
    raw = np.ascontiguousarray(data[:, 0])
    zero = np.zeros(nchan, np.int32)
    with _native.GpuSession(nsub, nchan, nbin, device=0, delay=delay, any_length=True) as s:
        s.upload(raw, w0, zero)
        one = s.run()
        one["amp"], one["info"] = s.fit()
        one["std"], one["mean"], one["ptp"], one["fft"] = s.diagnostics()
    assert int((one["weights"] == 0).sum()) > 0
    out = sharded.clean_cube_local(raw, w0, zero, 2, want_details=True, delay=delay, any_length=True)
    assert out["loops"] == one["loops"] and np.array_equal(out["changed"], one["changed"])
    for key in ("weights", "test", "amp", "info", "std", "mean", "ptp", "fft"):
        assert bits_equal(out[key], one[key]), key


@pytest.mark.parametrize("lanes", [1, 2])
def test_clean_batch_fft_equals_single_sessions(lanes):
    """Three archives of 4 x 16 x 100 with their own delays (two per channel,
    one per profile) through clean_batch(dedisp="fft", any_length=True)."""
    from iterative_cleaner_amd import _native, batch, synth
    shape = (4, 16, 100)
    arcs = []
    for k in range(3):
        data, w0, shift = synth.make_cube(*shape, 800 + k, 0.2)
        d = synth.fractional_delays(shift, shape[2]) + 0.13 * k
        if k == 2:
            d = np.ascontiguousarray(d[None, :] * (1.0 + 3e-4 * np.arange(shape[0]))[:, None])
        arcs.append((np.ascontiguousarray(data[:, 0]), w0, np.zeros(shape[1], np.int32), d))
    refs = []
    for cube, w0, shift, d in arcs:
        with _native.GpuSession(*shape, device=0, delay=d, any_length=True) as s:
            s.upload(cube, w0, shift)
            refs.append(s.run())
    got = list(batch.clean_batch(iter(arcs), shape, device=0, lanes=lanes, dedisp="fft", any_length=True))
    assert len(got) == 3
    for a, b in zip(got, refs):
        assert a["loops"] == b["loops"] and a["n_iter"] == b["n_iter"]
        assert np.array_equal(a["changed"], b["changed"]) and np.array_equal(a["nzero"], b["nzero"])
        assert bits_equal(a["weights"], b["weights"]) and bits_equal_nan(a["test"], b["test"])


# ---------------------------------------------------------------- 5. refusals

def test_refusals(monkeypatch):
    from iterative_cleaner_amd import _native
    monkeypatch.delenv(SWITCH, raising=False)
    for nbin in (100, 448):   # IC_DEDISP_FFT refuses what it refused
        with pytest.raises(_native.NativeError, match="power-of-two"):
            _native.GpuSession(4, 8, nbin, device=0, delay=np.zeros(8))
        with pytest.raises(_native.NativeError, match="power-of-two"):
            _native.rotate_profiles(np.zeros((2, 3, nbin), np.float32), np.zeros(3))
    for nbin in (8, 4104, 16384):
        with pytest.raises(_native.NativeError, match="power-of-two"):
            _native.GpuSession(4, 8, nbin, device=0, delay=np.zeros(8), any_length=True)
        with pytest.raises(_native.NativeError, match="power-of-two"):
            _native.rotate_profiles(np.zeros((2, 3, nbin), np.float32), np.zeros(3), any_length=True)
    with pytest.raises(_native.NativeError, match="IC_FIT_CLOSED with fractional dedispersion"):
        _native.GpuSession(4, 8, 100, device=0, delay=np.zeros(8), fit_mode=_native.FIT_CLOSED, any_length=True)
    # the integer mode keeps the fast mode at this length
    with _native.GpuSession(4, 8, 100, device=0, fit_mode=_native.FIT_CLOSED, any_length=True):
        pass
