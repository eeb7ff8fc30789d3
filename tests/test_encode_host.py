"""Host side of the quantised downloads (no GPU): the C-ABI surface of
ic_encode_profiles / ic_get_residual_quantised, the arithmetic the GPU encode is
held to (psrfits.quantise) on the inputs the GPU tests use, the PSRFITS writer
fed int16 samples, and clean(-u) writing the residual of a PSRFITS input as
PSRFITS from the samples the loop hands back."""
import ctypes
import os
import re

import numpy as np

import encode_cases as ec
from helpers import bits_equal

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_entry_points():
    from iterative_cleaner_amd import _native
    with open(os.path.join(REPO, "include", "iterative_cleaner.h")) as fh:
        text = fh.read()
    for name in ("ic_encode_profiles", "ic_get_residual_quantised"):
        assert re.search(r"\bint %s\(" % name, text) and name in _native.EXPORTS
    assert re.search(r"#define IC_ABI_VERSION 9\b", text) and _native.ABI_VERSION == 9
    lib = ctypes.CDLL(_native.LIB_PATH)
    assert hasattr(lib, "ic_encode_profiles") and hasattr(lib, "ic_get_residual_quantised")
    assert callable(_native.encode_profiles) and callable(_native.GpuSession.residual_quantised)


def test_argument_errors_need_no_gpu():
    from iterative_cleaner_amd import _native
    lib = _native.load_library()
    p = _native._ptr
    cube = np.zeros((2, 3, 8), np.float32)
    q = np.zeros((2, 3, 8), np.int16)
    scl, offs = np.zeros((2, 3), np.float32), np.zeros((2, 3), np.float32)

    def encode(shape=(2, 3, 8), flags=0, ptrs=(p(cube), p(q), p(scl), p(offs))):
        return lib.ic_encode_profiles(0, *shape, ptrs[0], flags, *ptrs[1:])

    for k in range(4):                                    # a null pointer, each in turn
        ptrs = [p(cube), p(q), p(scl), p(offs)]
        ptrs[k] = None
        assert encode(ptrs=ptrs) == -1, k
        assert _native._err(lib)
    for shape in ((0, 3, 8), (2, 0, 8), (2, 3, 0), (-1, 3, 8)):
        assert encode(shape=shape) == -1, shape
        assert "shape" in _native._err(lib)
    for flags in (2, 3, -1):
        assert encode(flags=flags) == -1, flags
        assert "flag" in _native._err(lib)
    for args in ((None, 0, p(q), p(scl), p(offs)), (None, 2, p(q), p(scl), p(offs))):
        assert lib.ic_get_residual_quantised(*args) == -1


def test_tie_fixture_pins_round_half_even():
    """scl == 1 and offs == 0 exactly, so x is the sample itself: 0.5, 1.5, 2.5,
    -1.5 -> 0, 2, 2, -2 (floor(x + 0.5) would give 1, 2, 3, -1)."""
    for nbin in ec.NBINS:
        q, scl, offs = ec.host_quantise(ec.edge_cube(nbin))
        assert scl[2, 2] == 1.0 and offs[2, 2] == 0.0
        assert tuple(q[2, 2, 2:6]) == ec.TIE_Q
        assert q[2, 2, 0] == -32767 and q[2, 2, 1] == 32767
        assert np.array_equal(ec.edge_cube(nbin)[2, 2, 2:6], np.float32(ec.TIE_SAMPLES))


def test_edge_rows_are_what_they_claim():
    """The reference on the edge rows: NaN and both infinities give a NaN offs
    and all-zero samples, one +inf an infinite offs and -32767 everywhere else,
    subnormal ranges a subnormal scale or 1, and -32768 appears nowhere."""
    for nbin in ec.NBINS + (50,):
        cube = ec.edge_cube(nbin)
        q, scl, offs = ec.host_quantise(cube)
        assert q.min() >= -32767
        assert scl[1, 1] == 1.0 and offs[1, 1] == 3.25 and not q[1, 1].any()          # constant
        assert scl[1, 2] == 1.0 and bits_equal(offs[1, 2], np.float32(0.0)) and not q[1, 2].any()
        for row in ((1, 3), (2, 0)):                                                   # NaN, both infinities
            assert np.isnan(offs[row]) and scl[row] == 1.0 and not q[row].any()
        assert np.isposinf(offs[1, 4]) and scl[1, 4] == 1.0
        assert q[1, 4, -1] == 0 and np.all(q[1, 4, :-1] == -32767)
        assert np.isfinite(scl[2, 1]) and scl[2, 1] > 1e33 and abs(q[2, 1]).max() == 32767
        assert 0 < scl[2, 3] < np.finfo(np.float32).tiny and abs(q[2, 3]).max() > 30000
        assert scl[2, 4] == 1.0 and not q[2, 4].any()


def test_bit_comparison_can_see_an_all_f32_encode():
    """On the GPU test's random cube an encode with every step in f32 differs
    from psrfits.quantise in samples and in scales, so the GPU test's bit
    comparison does pin the f64 steps.  (A reciprocal multiply and
    floor(x + 0.5) do not show on random data: the tie fixture is for them.)"""
    cube = ec.random_cube()
    q, scl, offs = ec.host_quantise(cube)
    q32, scl32, offs32 = ec.quantise_all_f32(cube)
    nq, ns = int((q32 != q).sum()), int((scl32 != scl).sum())
    print("all-f32 encode: %d of %d samples and %d of %d scales differ" % (nq, q.size, ns, scl.size))
    assert nq >= 1 and ns >= 1


def _archive(tmp_path, name="obs.sf", npol=2, **kw):
    from iterative_cleaner_amd import synth
    path = str(tmp_path / name)
    synth.make_archive(5, 12, 32, seed=11, rfi_frac=0.2, npol=npol, filename=path, **kw).unload(path)
    return path


def test_save_quantised_writes_the_bytes_of_save(tmp_path):
    """save(ar) == save_quantised(quantise(ar's samples), ar's metadata), for an
    archive with integer shifts and for one with fractional delays, with native
    and with big-endian samples, and without the stand-in's own columns."""
    from iterative_cleaner_amd import archive as ica
    from iterative_cleaner_amd import psrfits, synth
    data, w, shift = synth.make_cube(4, 6, 64, 5, 0.2, npol=2)
    w[1, 2] = 0.0
    plain = ica.Archive(data, w, shift, source="J1234+5678", centre_frequency=1284.5, mjd_start=59000.25,
                        mjd_end=59000.5, baseline_duty=0.2)
    frac = ica.Archive(data, w, np.zeros(6, np.int64), dedispersed=True,
                       dm_delay=synth.fractional_delays(shift, 64))
    frac._chan_freqs = 1300.0 + np.arange(6) * 3.0
    frac._period = 0.0125 * (1.0 + 3e-4 * np.cos(np.arange(4)))
    frac._dm = 20.0
    for k, ar in enumerate((plain, frac)):
        for stand_in in (True, False):
            a, b = str(tmp_path / ("a%d" % k)), str(tmp_path / ("b%d" % k))
            psrfits.save(ar, a, stand_in_meta=stand_in)
            q, scl, offs = psrfits.quantise(ar._data)
            for samples in (q, q.astype(">i2")):
                psrfits.save_quantised(b, samples, scl, offs, stand_in_meta=stand_in, **psrfits.archive_meta(ar))
                assert open(a, "rb").read() == open(b, "rb").read()
    # one polarisation without its axis, the form residual_quantised returns
    one = ica.Archive(data[:, :1], w, shift)
    q, scl, offs = psrfits.quantise(one._data)
    psrfits.save(one, str(tmp_path / "one_a"))
    psrfits.save_quantised(str(tmp_path / "one_b"), q[:, 0].astype(">i2"), scl[:, 0], offs[:, 0],
                           **psrfits.archive_meta(one))
    assert open(tmp_path / "one_a", "rb").read() == open(tmp_path / "one_b", "rb").read()


def _stub_loop(seen, residual):
    """run_loop stubbed: converges in one loop, zaps nothing, and hands back the
    residual in the form the call asked for."""
    from iterative_cleaner_amd import psrfits

    def run_loop(cube, w0, shift, args, **kw):
        seen.append(kw)
        nsub, nchan = np.shape(w0)
        out = dict(n_iter=1, converged=True, loops=1, changed=np.array([0]), nzero=np.array([0]),
                   bad_fits=np.array([0]), test=np.zeros((nsub, nchan)), weights=np.asarray(w0, np.float32))
        if kw.get("residual_quantised"):
            q, scl, offs = psrfits.quantise(residual[:, None])
            out["residual_q"] = (q[:, 0].astype(">i2"), scl[:, 0], offs[:, 0])
        else:
            out["residual"] = residual
        return out
    return run_loop


def test_clean_writes_the_residual_of_a_psrfits_input_as_psrfits(tmp_path, monkeypatch):
    from iterative_cleaner_amd import archive as ica
    from iterative_cleaner_amd import cleaner, psrfits
    monkeypatch.chdir(tmp_path)
    _archive(tmp_path)
    src = ica.Archive_load("obs.sf")
    src.get_Integration(1).set_weight(3, 0.0)
    src.unload("obs.sf")                                    # an input with a zero weight of its own
    src = ica.Archive_load("obs.sf")
    residual = np.random.default_rng(3).standard_normal((5, 12, 32)).astype(np.float32)
    seen = []
    monkeypatch.setattr(cleaner, "run_loop", _stub_loop(seen, residual))
    cleaner.clean(ica.Archive_load("obs.sf"), cleaner.parse_arguments(["-l", "-q", "-u", "obs.sf"]), "obs.sf")
    assert len(seen) == 1 and seen[0]["want_residual"] is True and seen[0]["residual_quantised"] is True
    name = "obs.sf_residual_1.ar"
    assert psrfits.is_psrfits(name)
    q, scl, offs, weights, shift, meta = psrfits.load_quantised(name)
    want = psrfits.quantise(residual[:, None])
    assert q.dtype == np.dtype(">i2") and q.shape == (5, 1, 12, 32)
    assert bits_equal(q.astype(np.int16), want[0]) and bits_equal(scl, want[1]) and bits_equal(offs, want[2])
    assert meta["state"] == "Intensity" and meta["npol"] == 1 and meta["dedispersed"] is False
    assert meta["source"] == src.get_source() and meta["baseline_duty"] == src.get_baseline_duty()
    assert bits_equal(weights, src.get_weights()) and weights[1, 3] == 0.0
    assert bits_equal(shift, src.get_dm_shift())
    back = ica.Archive_load(name)
    assert bits_equal(back.get_data(), psrfits.decode(*want))
    assert back.get_centre_frequency() == src.get_centre_frequency()
    assert abs(back.start_time().in_days() - src.start_time().in_days()) < 1e-9     # the header's split of the MJD
    # a loop that can only hand back the merged f32 residual (channel shards): encoded on the host, same file
    first = open(name, "rb").read()
    os.remove(name)

    def f32_only(cube, w0, shift, args, **kw):
        return _stub_loop([], residual)(cube, w0, shift, args, **dict(kw, residual_quantised=False))

    monkeypatch.setattr(cleaner, "run_loop", f32_only)
    cleaner.clean(ica.Archive_load("obs.sf"), cleaner.parse_arguments(["-l", "-q", "-u", "obs.sf"]), "obs.sf")
    assert open(name, "rb").read() == first


def test_clean_keeps_the_npz_residual_of_an_npz_input(tmp_path, monkeypatch):
    """The residual of an .npz input is the .npz it always was: the plain
    Archive of the f32 residual, the weights before the cleaning, the shifts."""
    from iterative_cleaner_amd import archive as ica
    from iterative_cleaner_amd import cleaner, psrfits
    monkeypatch.chdir(tmp_path)
    _archive(tmp_path, name="obs.ar")
    assert not psrfits.is_psrfits("obs.ar")
    src = ica.Archive_load("obs.ar")
    residual = np.random.default_rng(4).standard_normal((5, 12, 32)).astype(np.float32)
    seen = []
    monkeypatch.setattr(cleaner, "run_loop", _stub_loop(seen, residual))
    cleaner.clean(ica.Archive_load("obs.ar"), cleaner.parse_arguments(["-l", "-q", "-u", "obs.ar"]), "obs.ar")
    assert len(seen) == 1 and not seen[0]["residual_quantised"]
    name = "obs.ar_residual_1.ar"
    got = open(name, "rb").read()
    os.remove(name)
    ica.Archive(residual[:, None], src.get_weights(), src.get_dm_shift(), dedispersed=False, dm_delay=None,
                filename="residual.ar", source=src.get_source()).unload(name)
    assert not psrfits.is_psrfits(name) and open(name, "rb").read() == got
