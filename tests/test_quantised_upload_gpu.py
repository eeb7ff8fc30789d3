"""GPU tests of the quantised uploads (ic_upload_quantised[_async],
ic_decode_profiles): PSRFITS int16 samples with their per-(subint, pol, channel)
scale and offset cross the bus as stored and are decoded on the device.  The
decoded, polarisation-summed cube must carry exactly the bits of the host's
psrfits.decode + archive.py pscrunch (three separate f32 roundings, no fused
multiply-add), so a session fed the samples gives the results of a session fed
the host-decoded cube, through every layer: kernel, session, shards, the
asynchronous queue, the batch ring and the CLI."""
import threading

import numpy as np
import pytest

from helpers import bits_equal, bits_equal_nan

pytestmark = pytest.mark.gpu

SHAPE = (6, 96, 128)
_CACHE = {}


def _quantised(nsub, npol, nchan, nbin, seed=300, rfi=0.1):
    """quantise(make_cube) with pol 1 perturbed (synth makes pol 1 ~ pol 0, whose
    sum would be exact); cached: (q, scl, offs, w0, shift), never modified."""
    from iterative_cleaner_amd import psrfits, synth
    key = (nsub, npol, nchan, nbin, seed, rfi)
    if key not in _CACHE:
        data, w0, shift = synth.make_cube(nsub, nchan, nbin, seed, rfi, npol=npol)
        if npol > 1:
            rng = np.random.default_rng(seed + 1)
            data[:, 1] += (0.37 * rng.standard_normal(data[:, 1].shape)).astype(np.float32)
        _CACHE[key] = psrfits.quantise(data) + (w0, shift)
    return _CACHE[key]


def _host(q, scl, offs, nsum):
    """psrfits.decode, then archive.py's polarisation rule."""
    from iterative_cleaner_amd import psrfits
    with np.errstate(all="ignore"):
        d = psrfits.decode(np.asarray(q).astype(np.int16), scl, offs)
        return np.ascontiguousarray(d[:, 0] if nsum == 1 else (d[:, 0] + d[:, 1]).astype(np.float32))


DECODE_CASES = [
    # (nsub, npol, nchan, nbin, nsum)
    (3, 2, 5, 64, 2),
    (3, 2, 5, 64, 1),
    (3, 4, 5, 64, 1),        # skipped polarisations: the strided copies
    (3, 4, 5, 64, 2),
    (3, 2, 5, 50, 2),        # nbin % 8 != 0: the scalar path
    (3, 2, 5, 50, 1),
    (1, 1, 1, 8, 1),         # one group
    (64, 1, 520, 512, 1),    # more groups than one pass of the capped grid (8192 x 256 x 8 samples)
]


@pytest.mark.parametrize("case", DECODE_CASES, ids=lambda c: "%dx%dx%dx%d-nsum%d" % c)
def test_decode_equals_host_decode(case):
    from iterative_cleaner_amd import _native
    nsub, npol, nchan, nbin, nsum = case
    q, scl, offs = _quantised(nsub, npol, nchan, nbin)[:3]
    got = _native.decode_profiles(q, scl, offs, nsum)
    assert bits_equal(got, _host(q, scl, offs, nsum))


def test_bit_exactness_can_see_a_fused_multiply_add():
    """A decode with one rounding for q * scl + offs (what a fused multiply-add
    gives) differs from psrfits.decode in a large share of the first case's
    samples: the bit comparisons above do pin the rounding."""
    from iterative_cleaner_amd import psrfits
    q, scl, offs = _quantised(3, 2, 5, 64)[:3]
    fused = (q.astype(np.float64) * scl.astype(np.float64)[..., None]
             + offs.astype(np.float64)[..., None]).astype(np.float32)
    frac = np.mean(fused != psrfits.decode(q, scl, offs))
    print("fused != separate roundings in %.1f %% of the samples" % (100 * frac))
    assert frac >= 0.10


@pytest.mark.parametrize("nsum", [1, 2])
@pytest.mark.parametrize("nbin", [16, 12])
def test_decode_edge_values(nsum, nbin):
    """The int16 extremes, scl = 0, scl = inf on q = 0 (NaN), offs = NaN: the
    host's bits, NaN where the host gives NaN."""
    from iterative_cleaner_amd import _native
    rng = np.random.default_rng(7)
    q = rng.integers(-32768, 32768, size=(2, 2, 3, nbin)).astype(np.int16)
    scl = rng.uniform(0.001, 2.0, size=(2, 2, 3)).astype(np.float32)
    offs = rng.standard_normal((2, 2, 3)).astype(np.float32)
    q[0, 0, 0, :3] = (-32768, 32767, 0)
    q[1, 1, 2, -3:] = (0, 32767, -32768)
    scl[0, 0, 1] = 0.0
    scl[0, 1, 2] = np.inf
    q[0, 1, 2, :] = 0
    q[0, 1, 2, 5] = 3
    scl[1, 0, 0] = np.inf
    q[1, 0, 0, ::2] = 0
    offs[1, 0, 1] = np.nan
    offs[1, 1, 0] = -np.inf
    want = _host(q, scl, offs, nsum)
    assert np.isnan(want).any() and np.isinf(want).any()
    assert bits_equal_nan(_native.decode_profiles(q, scl, offs, nsum), want)


@pytest.mark.parametrize("case", [(3, 2, 5, 64, 2), (3, 4, 5, 50, 2), (3, 4, 5, 64, 1)],
                         ids=lambda c: "%dx%dx%dx%d-nsum%d" % c)
def test_big_endian_samples_give_the_same_cube(case):
    from iterative_cleaner_amd import _native
    nsub, npol, nchan, nbin, nsum = case
    q, scl, offs = _quantised(nsub, npol, nchan, nbin)[:3]
    be = q.astype(">i2")
    assert be.tobytes() != q.tobytes()
    assert bits_equal(_native.decode_profiles(be, scl, offs, nsum), _native.decode_profiles(q, scl, offs, nsum))


def _results(s):
    out = s.run()
    out["residual"] = s.residual()
    return out


def _same(a, b):
    assert a["loops"] == b["loops"] and a["n_iter"] == b["n_iter"]
    assert np.array_equal(a["changed"], b["changed"]) and np.array_equal(a["nzero"], b["nzero"])
    assert bits_equal(a["weights"], b["weights"]) and bits_equal_nan(a["test"], b["test"])
    if "residual" in a and "residual" in b:
        assert bits_equal_nan(a["residual"], b["residual"])


def _session_kinds():
    from iterative_cleaner_amd import _native, synth
    shift = synth.make_cube(1, SHAPE[1], SHAPE[2], 0, 0.0)[2]
    return {"default": {}, "closed": {"fit_mode": _native.FIT_CLOSED},
            "fft": {"delay": synth.fractional_delays(shift, SHAPE[2])}}


@pytest.mark.parametrize("kind", ["default", "closed", "fft"])
@pytest.mark.parametrize("npol,nsum", [(2, 2), (4, 1)])
def test_session_upload_quantised_matches_host_decoded_upload(kind, npol, nsum):
    """upload_quantised + run == upload(host-decoded, host-pscrunched) + run, for a
    default session, the fast mode (no fit cube) and FFT dedispersion; an f32
    upload on the same session afterwards still gives its own results, and a
    second quantised upload (the staging reused) repeats the first."""
    from iterative_cleaner_amd import _native
    kw = _session_kinds()[kind]
    q, scl, offs, w0, shift = _quantised(*SHAPE[:1], npol, *SHAPE[1:])
    q2, scl2, offs2, w2, _ = _quantised(*SHAPE[:1], 1, *SHAPE[1:], seed=301, rfi=0.2)
    other = _host(q2, scl2, offs2, 1)
    with _native.GpuSession(*SHAPE, device=0, **kw) as s:
        s.upload(_host(q, scl, offs, nsum), w0, shift)
        ref = _results(s)
        s.upload(other, w2, shift)
        ref_other = _results(s)
    assert not bits_equal(ref["weights"], ref_other["weights"])
    with _native.GpuSession(*SHAPE, device=0, **kw) as s:
        s.upload_quantised(q, scl, offs, w0, shift, nsum)
        _same(_results(s), ref)
        s.upload(other, w2, shift)
        _same(_results(s), ref_other)
        s.upload_quantised(q.astype(">i2"), scl, offs, w0, shift, nsum)
        _same(_results(s), ref)
        s.upload_quantised(q2[:, 0], scl2, offs2, w2, shift, 1)      # 3-D samples: one polarisation
        _same(_results(s), ref_other)


def test_shards_upload_their_quantised_slices():
    """World 2, in process: each shard uploads its channel slice of the samples;
    the merged result is the unsharded session's."""
    from iterative_cleaner_amd import _native
    nsub, nchan, nbin = 4, 512, 64
    q, scl, offs, w0, shift = _quantised(nsub, 2, nchan, nbin, seed=310, rfi=0.2)
    with _native.GpuSession(nsub, nchan, nbin, device=0) as s:
        s.upload(_host(q, scl, offs, 2), w0, shift)
        one = s.run()
    chans, _ = _native.shard_layout(nsub, nchan, 2)
    results, errors = [None, None], []
    with _native.ShardGroup(2) as group:
        sessions = [_native.ShardSession(nsub, nchan, nbin, r, 2, group=group, device=0) for r in range(2)]
        try:
            for r, s in enumerate(sessions):
                c0, c1 = chans[r]
                s.upload_quantised(q[:, :, c0:c1], scl[:, :, c0:c1], offs[:, :, c0:c1], w0[:, c0:c1],
                                   shift[c0:c1], 2)

            def work(r):
                try:
                    results[r] = sessions[r].run()
                except Exception as e:  # noqa: BLE001 - reported below
                    errors.append(e)

            threads = [threading.Thread(target=work, args=(r,)) for r in range(2)]
            for t in threads:
                t.start()
            for t in threads:
                t.join()
        finally:
            for s in sessions:
                s.close()
    assert not errors, errors
    for out in results:
        assert out["loops"] == one["loops"] and np.array_equal(out["changed"], one["changed"])
        assert np.array_equal(out["nzero"], one["nzero"])
    for key in ("weights", "test"):
        merged = np.concatenate([results[r][key] for r in range(2)], axis=1)
        assert chans[0][1] == chans[1][0] and bits_equal(merged, one[key]), key


def _pinned(arrays):
    from iterative_cleaner_amd import _native
    out = []
    for a in arrays:
        p = _native.PinnedArray(a.shape, a.dtype)
        p.array[...] = a
        out.append(p)
    return out


def test_pipeline_mixes_f32_and_quantised_items_and_queue_rules():
    from iterative_cleaner_amd import _native, batch
    arcs = [_quantised(SHAPE[0], 2, *SHAPE[1:], seed=320 + k, rfi=0.1 + 0.05 * k) for k in range(4)]
    refs, pinned, items = [], [], []
    with _native.GpuSession(*SHAPE, device=0) as s:
        for q, scl, offs, w0, shift in arcs:
            s.upload(_host(q, scl, offs, 2), w0, shift)
            refs.append(s.run())
    for k, (q, scl, offs, w0, shift) in enumerate(arcs):
        sh = shift.astype(np.int32)
        if k % 2 == 0:
            trio = _pinned((_host(q, scl, offs, 2), w0, sh))
        else:   # quantised, one of them in the FITS byte order
            trio = _pinned((q.astype(">i2") if k == 1 else q, scl, offs, w0, sh))
        pinned.append(trio)
        items.append(tuple(p.array for p in trio))
    assert [len(i) for i in items] == [3, 5, 3, 5]
    with _native.GpuSession(*SHAPE, device=0) as s:
        order = (0, 1, 2, 3, 1, 3, 0)
        outs = list(batch.pipeline(s, [items[i] for i in order], nsum=2))
        assert len(outs) == len(order)
        for i, out in zip(order, outs):
            _same(out, refs[i])
        # two slots: a third pending upload, and a synchronous one behind a pending one, are refused
        s.upload_quantised_async(*items[1], 2)
        with pytest.raises(_native.NativeError, match=r"rc=-4"):
            s.upload_quantised(*arcs[0], 2)
        s.upload_async(*items[0])
        with pytest.raises(_native.NativeError, match=r"rc=-4"):
            s.upload_quantised_async(*items[3], 2)
        _same(s.run(), refs[1])
        _same(s.run(), refs[0])
        s.upload_quantised(*arcs[3], 2)
        _same(s.run(), refs[3])
        # as strict as upload_async about what it is handed
        with pytest.raises(ValueError):
            s.upload_quantised_async(items[1][0].astype(np.int32), *items[1][1:], 2)
        with pytest.raises(ValueError):
            s.upload_quantised_async(items[1][0][:, :, ::2], *items[1][1:], 2)
    for trio in pinned:
        for p in trio:
            p.close()


@pytest.mark.parametrize("lanes", [1, 2])
def test_clean_batch_quantised_matches_single_sessions(lanes):
    from iterative_cleaner_amd import _native, batch
    arcs = []
    for k in range(7):
        q, scl, offs, w0, shift = _quantised(SHAPE[0], 2, *SHAPE[1:], seed=320 + k, rfi=0.1 + 0.05 * (k % 3))
        arcs.append((q.astype(">i2"), scl, offs, w0, shift))       # as psrfits.load_quantised hands them
    got = list(batch.clean_batch(iter(arcs), SHAPE, device=0, lanes=lanes, quantised=True, nsum=2))
    assert len(got) == len(arcs)
    with _native.GpuSession(*SHAPE, device=0) as s:
        for (q, scl, offs, w0, shift), out in zip(arcs, got):
            s.upload(_host(q, scl, offs, 2), w0, shift)
            _same(out, s.run())


def test_argument_errors():
    from iterative_cleaner_amd import _native
    lib = _native.load_library()
    q, scl, offs, w0, shift = _quantised(3, 2, 5, 64)
    out = np.empty((3, 5, 64), np.float32)
    p = _native._ptr

    def decode(npol, nsum, flags, scl_ptr):
        return lib.ic_decode_profiles(0, 3, npol, nsum, 5, 64, p(q), scl_ptr, p(offs), flags, p(out))

    for args in ((2, 3, 0, p(scl)),       # nsum = 3
                 (1, 2, 0, p(scl)),       # nsum = 2 with npol = 1
                 (2, 2, 2, p(scl)),       # an unknown flag
                 (2, 2, 0, None)):        # a null scl
        assert decode(*args) == -1, args
        assert _native._err(lib), args
    assert decode(2, 2, 0, p(scl)) == 0
    with _native.GpuSession(3, 5, 64, device=0) as s:
        sh = shift.astype(np.int32)
        for bad in (64, -1):
            sh[3] = bad
            for fn in (lib.ic_upload_quantised, lib.ic_upload_quantised_async):
                assert fn(s.h, p(q), p(scl), p(offs), 2, 2, 0, p(w0), p(sh)) == -1
                assert "shift" in _native._err(lib)
        sh[3] = 3
        assert lib.ic_upload_quantised(s.h, p(q), p(scl), p(offs), 2, 3, 0, p(w0), p(sh)) == -1
        assert lib.ic_upload_quantised_async(s.h, p(q), None, p(offs), 2, 2, 0, p(w0), p(sh)) == -1
        assert lib.ic_upload_quantised(s.h, p(q), p(scl), p(offs), 2, 2, 4, p(w0), p(sh)) == -1
        with pytest.raises(_native.NativeError, match=r"rc=-1"):
            s.upload_quantised(q[:, :1], scl[:, :1], offs[:, :1], w0, shift, 2)
        assert lib.ic_upload_quantised(s.h, p(q), p(scl), p(offs), 2, 2, 0, p(w0), p(sh)) == 0


@pytest.mark.parametrize("extra,calls", [([], 1), (["-p"], 0)])
def test_cli_takes_the_quantised_upload(tmp_path, monkeypatch, capsys, oracle_lib, extra, calls):
    """A 2-pol PSRFITS archive through cleaner.main: its samples go up as stored
    (one upload_quantised call); with -p the archive is pscrunched on the host
    first, which ends the quantisation, and the f32 path serves.  Same weights."""
    from iterative_cleaner_amd import _native, cleaner, synth
    from iterative_cleaner_amd import archive as ica
    monkeypatch.chdir(tmp_path)
    synth.make_archive(16, 64, 128, seed=41, rfi_frac=0.2, npol=2, filename="obs.sf").unload("obs.sf")
    src = ica.Archive_load("obs.sf")
    dec = src.get_data()
    ref = oracle_lib.clean_loop((dec[:, 0] + dec[:, 1]).astype(np.float32), src.get_weights(), src.get_dm_shift())
    seen = []
    orig = _native.GpuSession.upload_quantised

    def spy(self, q, scl, offs, w0, shift, nsum):
        seen.append((q.shape, nsum))
        return orig(self, q, scl, offs, w0, shift, nsum)

    monkeypatch.setattr(_native.GpuSession, "upload_quantised", spy)
    cleaner.main(cleaner.parse_arguments(["-l", "-q", *extra, "obs.sf"]))
    assert len(seen) == calls
    if calls:
        assert seen[0] == ((16, 2, 64, 128), 2)
    res = ica.Archive_load("obs_cleaned.ar")
    assert bits_equal(res.get_weights(), ref["weights"])
