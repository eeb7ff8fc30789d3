"""GPU tests of the quantised downloads (ic_encode_profiles,
ic_get_residual_quantised): the residual is encoded on the device to the int16
samples, scales and offsets a PSRFITS file stores, bit for bit what
psrfits.quantise - host code that predates the kernel - gives the same f32
samples (a NaN equals any NaN), so 2 bytes per sample leave the GPU and the CLI
writes the residual of a PSRFITS input as PSRFITS without ever holding the f32
cube.  Through every layer: kernel, session, binding, CLI."""
import numpy as np
import pytest

import encode_cases as ec
from helpers import bits_equal, bits_equal_nan

pytestmark = pytest.mark.gpu


def _same(got, want, big_endian=False):
    q, scl, offs = got
    assert q.dtype == np.dtype(">i2" if big_endian else np.int16) and q.flags.c_contiguous
    if big_endian:
        assert q.tobytes() == want[0].astype(">i2").tobytes()         # the bytes of the DATA column
    bad = int((q.astype(np.int16) != want[0]).sum())
    assert bad == 0, "%d of %d samples differ" % (bad, q.size)
    assert q.shape == want[0].shape
    assert bits_equal_nan(scl, want[1]), "scales"
    assert bits_equal_nan(offs, want[2]), "offsets"


# nbin % 8 == 0: 16-byte loads and stores; 100: 16-byte loads, samples stored one
# by one; 50: neither.  64 and 128 leave lanes (and whole waves) without a
# sample, 8192 gives every lane 32.
@pytest.mark.parametrize("big_endian", [False, True], ids=["native", "big-endian"])
@pytest.mark.parametrize("nbin", ec.NBINS + (50,))
def test_encode_equals_host_quantise(nbin, big_endian):
    """3 x 5 profiles, one per kind (encode_cases.edge_cube): noise at magnitudes
    1e-3 .. 1e6, a constant, all +0, one NaN, one +inf, both infinities, +-3e38,
    the round-half-even ties between -32767 and 32767, subnormals."""
    from iterative_cleaner_amd import _native
    cube = ec.edge_cube(nbin)
    want = ec.host_quantise(cube)
    got = _native.encode_profiles(cube, big_endian=big_endian)
    assert tuple(got[0].astype(np.int16)[2, 2, 2:6]) == ec.TIE_Q
    assert got[0].astype(np.int16).min() >= -32767
    _same(got, want, big_endian)


def test_encode_random_profiles():
    """16 x 64 profiles of 1024 bins, amplitudes 0.1 .. 1e4: the cube on which
    test_encode_host shows that an all-f32 encode differs in samples and scales."""
    from iterative_cleaner_amd import _native
    cube = ec.random_cube()
    _same(_native.encode_profiles(cube), ec.host_quantise(cube))


def _case(name):
    """(shape, session keywords) of a residual case; the delays from the
    shifts of the synthetic archive, as the FFT dedispersion tests make them."""
    from iterative_cleaner_amd import _native, synth
    shapes = {"exact": (6, 40, 128), "closed": (6, 40, 128), "generic": (5, 33, 100),
              "fft-channel": (6, 48, 256), "fft-profile": (6, 48, 256)}
    nsub, nchan, nbin = shapes[name]
    kw = {}
    if name == "closed":
        kw["fit_mode"] = _native.FIT_CLOSED
    if name.startswith("fft"):
        shift = synth.make_cube(1, nchan, nbin, 0, 0.0)[2]
        kw["delay"] = synth.fractional_delays(shift, nbin) if name == "fft-channel" \
            else synth.per_profile_delays(shift, nbin, nsub)
    return (nsub, nchan, nbin), kw


@pytest.mark.parametrize("cap", [0, 1, 3])
@pytest.mark.parametrize("name", ["exact", "closed", "generic", "fft-channel", "fft-profile"])
def test_residual_quantised_equals_host_quantise_of_residual(name, cap):
    """residual_quantised() == psrfits.quantise(residual()) on one session:
    residual() is held to the reference by the parity tests and quantise is the
    host's, neither is under test.  grid_cap 1 and 3 take the profile loop of
    k_encode_q (and of the residual kernels before it) through many trips per
    block.  Twice, and once more in the FITS byte order: the staging is reused."""
    from iterative_cleaner_amd import _native, psrfits, synth
    shape, kw = _case(name)
    data, w0, shift = synth.make_cube(*shape, 70 + shape[2], 0.2)
    raw = np.ascontiguousarray(data[:, 0])
    with _native.GpuSession(*shape, device=0, options={"grid_cap": cap} if cap else None, **kw) as s:
        s.upload(raw, w0, shift)
        with pytest.raises(_native.NativeError, match=r"rc=-4"):
            s.residual_quantised()
        out = s.run()
        assert out["n_iter"] >= 1
        res = s.residual()
        assert np.count_nonzero(res) > res.size // 2
        q, scl, offs = psrfits.quantise(res[:, None])
        want = (np.ascontiguousarray(q[:, 0]), scl[:, 0], offs[:, 0])
        first = s.residual_quantised()
        _same(first, want)
        _same(s.residual_quantised(big_endian=True), want, True)
        again = s.residual_quantised()
        assert all(bits_equal(a, b) for a, b in zip(first, again))
        assert bits_equal(s.residual(), res)                       # and the f32 download still serves


def test_cli_writes_the_residual_from_the_quantised_download(tmp_path, monkeypatch, capsys, oracle_lib):
    """-u on a 2-polarisation PSRFITS archive: the residual file is PSRFITS, made
    from residual_quantised (GpuSession.residual raises), with the samples,
    scales and offsets psrfits.quantise gives the residual of a separate session
    on the same input, the input's weights and metadata; the cleaned archive is
    what it was."""
    from iterative_cleaner_amd import _native, cleaner, psrfits, synth
    from iterative_cleaner_amd import archive as ica
    monkeypatch.chdir(tmp_path)
    synth.make_archive(16, 64, 128, seed=41, rfi_frac=0.2, npol=2, filename="obs.sf").unload("obs.sf")
    src = ica.Archive_load("obs.sf")
    dec = src.get_data()
    cube = (dec[:, 0] + dec[:, 1]).astype(np.float32)          # archive.py pscrunch
    ref = oracle_lib.clean_loop(cube, src.get_weights(), src.get_dm_shift())
    with _native.GpuSession(16, 64, 128, device=0) as s:
        s.upload(cube, src.get_weights(), src.get_dm_shift())
        s.run()
        want = psrfits.quantise(s.residual()[:, None])

    def refuse(self):
        raise AssertionError("the f32 residual was downloaded")

    monkeypatch.setattr(_native.GpuSession, "residual", refuse)
    cleaner.main(cleaner.parse_arguments(["-l", "-q", "-u", "obs.sf"]))
    names = [p.name for p in tmp_path.iterdir() if "_residual_" in p.name]
    assert len(names) == 1 and names[0].endswith("_residual_%d.ar" % ref["loops"])
    assert psrfits.is_psrfits(names[0])
    q, scl, offs, weights, shift, meta = psrfits.load_quantised(names[0])
    assert q.shape == (16, 1, 64, 128) and meta["state"] == "Intensity" and meta["source"] == src.get_source()
    assert bits_equal(q.astype(np.int16), want[0]) and bits_equal(scl, want[1]) and bits_equal(offs, want[2])
    assert bits_equal(weights, src.get_weights()) and bits_equal(shift, src.get_dm_shift())
    back = ica.Archive_load(names[0])
    assert back.get_npol() == 1 and not back.get_dedispersed()
    assert bits_equal(back.get_data(), psrfits.decode(*want))
    res = ica.Archive_load("obs_cleaned.ar")
    assert bits_equal(res.get_weights(), ref["weights"])
    assert np.array_equal(res.get_data(), dec)
