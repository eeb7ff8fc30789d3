"""Fractional dedispersion at mixed-radix profile lengths on the GPU
(k_rotate_mr: nbin = 2M, M = 2^a 3^b 5^c, a multiple of 8 in 64..4096).

The C oracle's rotation is written for powers of two, so the yardsticks here
are the numpy definition (phase_rotation.rotate: the one-shot rotation must
carry its bits) and the reference's own clean() on stand-in archives of these
lengths (tests/golden/mr_clean_*.npz, made by tests/golden/make_golden_mr.py),
compared with the rules of tests/test_gpu_parity.py: template, amplitudes,
status, std / mean / ptp and weights bit for bit, fftmax within 1e-9 relative.
Every test here fails where the session and ic_rotate_profiles refuse these
lengths."""
import os

import numpy as np
import pytest

from helpers import GOLDEN, bits_equal, bits_equal_nan, load_clean_case
from test_fft_dedisp_gpu import _same
from test_phase_rotation import _edge_cube

pytestmark = pytest.mark.gpu

MR_FIXTURES = ["s6x24x96_fft", "s5x20x200_fft_pp_u", "s6x20x120_fft_f64", "s4x16x1000_fft_pr",
               "s4x12x1536_fft_ded"]


def _fixture(name):
    return os.path.join(GOLDEN, "mr_clean_%s.npz" % name)


# ---------------------------------------------------------------- 1. one-shot rotation

@pytest.mark.parametrize("nbin", [72, 80, 96, 120, 200, 1000, 1536, 4000])
def test_rotate_profiles_carries_the_definitions_bits(nbin):
    """5 x 7 profiles (35: a partial last block at every block size), per
    channel and per profile, both signs, with and without a baseline level (the
    one-shot entry point has no base argument: the level is subtracted in f32
    first, which is the definition's step 1; the kernel's own base argument is
    covered by the loop tests below, whose templates come from rot(raw - base))."""
    from iterative_cleaner_amd import _native
    from iterative_cleaner_amd import phase_rotation as pr
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
    xb = (x - b[..., None]).astype(np.float32)
    for delay in (d, d2):
        ph = pr.phasors(nbin, delay)
        for sign in (1, -1):
            assert _same(_native.rotate_profiles(x, delay, sign), pr.rotate(x, ph, sign)), (delay.ndim, sign)
            assert _same(_native.rotate_profiles(xb, delay, sign), pr.rotate(x, ph, sign, base=b)), (delay.ndim, sign)


@pytest.mark.parametrize("nbin", [120, 1000])
def test_rotate_profiles_f32_edge_values(nbin):
    """Subnormal, overflowing, signed-zero and spike profiles (f32 denormals
    kept), per channel and per profile: the definition's bits, NaNs as NaNs."""
    from iterative_cleaner_amd import _native
    from iterative_cleaner_amd import phase_rotation as pr
    x = _edge_cube(nbin)
    rng = np.random.default_rng(nbin + 1)
    d = rng.uniform(-2 * nbin, 2 * nbin, 6)
    d[1], d[2] = 0.0, 0.5
    d2 = rng.uniform(-2 * nbin, 2 * nbin, (4, 6))
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for delay in (d, d2):
            ph = pr.phasors(nbin, delay)
            for sign in (1, -1):
                assert _same(_native.rotate_profiles(x, delay, sign), pr.rotate(x, ph, sign)), (delay.ndim, sign)


# ---------------------------------------------------------------- 2. the reference's loop

@pytest.mark.parametrize("name", MR_FIXTURES)
def test_loop_matches_reference_fixture(name):
    """The last iteration (template, amp, info, std / mean / ptp, fftmax, test,
    weights, loops, per-iteration counters) and every earlier one, by the
    comparisons of tests/test_gpu_parity.py."""
    import test_gpu_parity as parity
    parity.test_loop_matches_reference(_fixture(name), "default")
    parity.test_every_iteration_matches_reference(_fixture(name))


@pytest.mark.parametrize("name", ["s6x24x96_fft", "s4x16x1000_fft_pr"])
def test_loop_matches_reference_fixture_rounds_and_tail(name):
    import test_gpu_parity as parity
    for fit_mode in ("rounds", "tail"):
        parity.test_loop_matches_reference(_fixture(name), fit_mode)


@pytest.mark.parametrize("name", MR_FIXTURES)
def test_clean_stdout_final_weights_and_residual_archive(name, tmp_path, monkeypatch, capsys):
    """cleaner.clean() on the archive file: the reference's stdout lines, final
    weights and (-u) residual archive."""
    import test_gpu_parity as parity
    parity.test_clean_stdout_matches_reference(_fixture(name), tmp_path, monkeypatch, capsys)


def test_residual_cube_is_the_fixtures():
    """ic_get_residual and the quantised residual's decoded cube at 200 bins."""
    from iterative_cleaner_amd import _native, psrfits
    z, meta, raw, w0, shift, args = load_clean_case(_fixture("s5x20x200_fft_pp_u"))
    nsub, nchan, nbin = raw.shape
    with _native.GpuSession(nsub, nchan, nbin, args["max_iter"], args["chanthresh"], args["subintthresh"],
                            args["pulse_region"], device=0, delay=z["dm_delay"]) as s:
        s.upload(raw, w0, shift)
        s.run()
        R = s.residual()
        q, scl, offs = s.residual_quantised()
    want = z["residual_data"][:, 0]
    assert bits_equal_nan(R, want)
    Rq, sclq, offq = psrfits.quantise(R[:, None])
    assert bits_equal(q, np.ascontiguousarray(Rq[:, 0])) and bits_equal(scl, sclq[:, 0])
    assert bits_equal(offs, offq[:, 0])


# ---------------------------------------------------------------- 3. schedules

def _run_1000(options, fit_tail=None):
    from iterative_cleaner_amd import _native
    z, meta, raw, w0, shift, args = load_clean_case(_fixture("s4x16x1000_fft_pr"))
    nsub, nchan, nbin = raw.shape
    with _native.GpuSession(nsub, nchan, nbin, args["max_iter"], args["chanthresh"], args["subintthresh"],
                            args["pulse_region"], device=0, delay=z["dm_delay"], options=options) as s:
        if fit_tail is not None:
            s.set_fit_tail(fit_tail)
        s.upload(raw, w0, shift)
        out = s.run()
        out["T"] = s.template()
        out["amp"], out["info"] = s.fit()
        out["diag"] = s.diagnostics()
        out["R"] = s.residual()
    return out


SCHEDULES = [({}, 0), ({"grid_cap": 1}, None), ({"diag_fork": 0}, None), ({"diag_fork": 1}, None),
             ({"diag_fork": 5, "fork_delay": 2}, None), ({"diag_fork": 64}, None), ({"diag_chain": 0}, None),
             ({"tail_split": 1, "diag_fork": 3}, 1 << 40), ({"fit_tiled": 0, "template_incr": 0}, None),
             ({"rot_stats": 0}, None)]


def test_schedules_are_bit_identical():
    """fit_tail = 0, grid_cap = 1 (every grid-stride loop past its first trip:
    64 profiles on one block) and every diagnostics-fork, chain-layout and
    fit-cube setting the session accepts at 1000 bins: the options the generic
    diagnostics kernel cannot serve resolve to the unforked schedule."""
    base = _run_1000({})
    for options, tail in SCHEDULES:
        got = _run_1000(options, tail)
        assert got["loops"] == base["loops"] and np.array_equal(got["changed"], base["changed"]), options
        for key in ("weights", "test", "T", "amp", "info"):
            assert bits_equal(got[key], base[key]), (options, key)
        for x0, x1 in zip(base["diag"], got["diag"]):
            assert bits_equal(x1, x0), options
        assert _same(got["R"], base["R"]), options


# ---------------------------------------------------------------- 4. shards and batch

def test_two_local_shards_equal_one_session():
    """Per-profile delays at 200 bins.  A shard owns whole 256-channel
    super-blocks (ic_shard_layout refuses 40 channels over two shards), so the
    archive has 600 channels: three super-blocks, split 2 + 1."""
    from iterative_cleaner_amd import _native, sharded, synth
    nsub, nchan, nbin = 6, 600, 200
    data, w0, shift = synth.make_cube(nsub, nchan, nbin, 91, 0.2)
    delay = synth.per_profile_delays(shift, nbin, nsub)
    raw = np.ascontiguousarray(data[:, 0])
    zero = np.zeros(nchan, np.int32)
    with _native.GpuSession(nsub, nchan, nbin, device=0, delay=delay) as s:
        s.upload(raw, w0, zero)
        one = s.run()
        one["amp"], one["info"] = s.fit()
        one["std"], one["mean"], one["ptp"], one["fft"] = s.diagnostics()
    assert int((one["weights"] == 0).sum()) > 0
    out = sharded.clean_cube_local(raw, w0, zero, 2, want_details=True, delay=delay)
    assert out["loops"] == one["loops"] and np.array_equal(out["changed"], one["changed"])
    for key in ("weights", "test", "amp", "info", "std", "mean", "ptp", "fft"):
        assert bits_equal(out[key], one[key]), key


@pytest.mark.parametrize("lanes", [1, 2])
def test_clean_batch_fft_equals_single_sessions(lanes):
    """Three archives of 4 x 16 x 240 with their own delays (two per channel,
    one per profile) through clean_batch(dedisp="fft")."""
    from iterative_cleaner_amd import _native, batch, synth
    shape = (4, 16, 240)
    arcs = []
    for k in range(3):
        data, w0, shift = synth.make_cube(*shape, 800 + k, 0.2)
        d = synth.fractional_delays(shift, shape[2]) + 0.13 * k
        if k == 2:
            d = np.ascontiguousarray(d[None, :] * (1.0 + 3e-4 * np.arange(shape[0]))[:, None])
        arcs.append((np.ascontiguousarray(data[:, 0]), w0, np.zeros(shape[1], np.int32), d))
    refs = []
    for cube, w0, shift, d in arcs:
        with _native.GpuSession(*shape, device=0, delay=d) as s:
            s.upload(cube, w0, shift)
            refs.append(s.run())
    got = list(batch.clean_batch(iter(arcs), shape, device=0, lanes=lanes, dedisp="fft"))
    assert len(got) == 3
    for a, b in zip(got, refs):
        assert a["loops"] == b["loops"] and a["n_iter"] == b["n_iter"]
        assert np.array_equal(a["changed"], b["changed"]) and np.array_equal(a["nzero"], b["nzero"])
        assert bits_equal(a["weights"], b["weights"]) and bits_equal_nan(a["test"], b["test"])


def test_foreign_psrfits_files_through_the_batch_loader(tmp_path):
    """Three foreign PSRFITS files of 4 x 16 x 240 (DM, channel frequencies,
    folding periods; two polarisations, int16 samples) through psrfits_loader
    and clean_batch: the results of single sessions on the decoded, pscrunched
    cubes with the files' DM-derived delays (per profile: the periods differ)."""
    from iterative_cleaner_amd import _native, batch, psrfits, synth
    from iterative_cleaner_amd import archive as ica
    shape = (4, 16, 240)
    paths, want = [], []
    for k in range(3):
        data, w, _ = synth.make_cube(*shape, 61 + k, 0.2, npol=2)
        path = str(tmp_path / ("dm%d.sf" % k))
        ar = ica.Archive(data, w, np.zeros(16, np.int64), filename=os.path.basename(path))
        ar._chan_freqs = 1300.0 + np.arange(16) * 3.0
        ar._period = 0.0125 * (1.0 + 3e-4 * np.cos(np.arange(4) + k))
        ar._dm = 20.0
        psrfits.save(ar, path, stand_in_meta=False)
        src = psrfits.load(path)
        delay = src.get_dm_delay()
        assert delay.shape == (4, 16) and np.any(delay != np.rint(delay))
        dec = src.get_data()
        cube = (dec[:, 0] + dec[:, 1]).astype(np.float32)
        with _native.GpuSession(*shape, device=0, delay=delay) as s:
            s.upload(cube, src.get_weights(), src.get_dm_shift())
            want.append(s.run())
        paths.append(path)
    got = list(batch.clean_batch(batch.psrfits_loader(paths, "fft"), shape, device=0, quantised=True, nsum=2,
                                 dedisp="fft"))
    assert len(got) == 3
    for out, ref in zip(got, want):
        assert out["loops"] == ref["loops"] and np.array_equal(out["changed"], ref["changed"])
        assert bits_equal(out["weights"], ref["weights"]) and bits_equal_nan(out["test"], ref["test"])


# ---------------------------------------------------------------- 5. refusals

def test_refusals():
    from iterative_cleaner_amd import _native
    for nbin in (448, 4104):
        with pytest.raises(_native.NativeError, match="power-of-two"):
            _native.GpuSession(4, 8, nbin, device=0, delay=np.zeros(8))
        with pytest.raises(_native.NativeError, match="power-of-two"):
            _native.rotate_profiles(np.zeros((2, 3, nbin), np.float32), np.zeros(3))
    with pytest.raises(_native.NativeError, match="IC_FIT_CLOSED with fractional dedispersion"):
        _native.GpuSession(4, 8, 1000, device=0, delay=np.zeros(8), fit_mode=_native.FIT_CLOSED)
    # the integer mode keeps the fast mode at this length
    with _native.GpuSession(4, 8, 1000, device=0, fit_mode=_native.FIT_CLOSED):
        pass
