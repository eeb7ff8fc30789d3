"""Batches of archives with fractional delays (ic_upload_delays_async): the
delays of an archive go up with its asynchronous upload, the channel phasor
table is built on the device (k_phasor_table) behind the copy, and the ic_run
that consumes the upload cleans with them.  Every pipelined result must carry
the bits of a fresh session that was given the same delays with set_delays
(whose table the same kernel builds; the anchor ties that to the C oracle)."""
import os

import numpy as np
import pytest

from helpers import bits_equal, bits_equal_nan

pytestmark = pytest.mark.gpu

SHAPE = (6, 24, 256)
_CACHE = {}


def _archives():
    """A, B: per-channel delays (A's first channels 0.0, 7.0, 0.25); C, D: per
    profile, every row different.  (cube, w0, zero shifts, delay), never modified."""
    if "arcs" not in _CACHE:
        from iterative_cleaner_amd import synth
        nsub, nchan, nbin = SHAPE
        arcs = {}
        for k, name in enumerate("ABCD"):
            data, w0, shift = synth.make_cube(nsub, nchan, nbin, 700 + k, 0.15 + 0.05 * k)
            d = synth.fractional_delays(shift, nbin) + 0.11 * k
            if name == "A":
                d[:3] = (0.0, 7.0, 0.25)
            if name in "CD":
                d = np.ascontiguousarray(d[None, :] * (1.0 + (1e-6 if name == "C" else 3e-4) * np.arange(nsub))[:, None])
                assert np.all(d[1:] != d[:-1])
            arcs[name] = (np.ascontiguousarray(data[:, 0]), w0, np.zeros(nchan, np.int32), d)
        _CACHE["arcs"] = arcs
    return _CACHE["arcs"]


def _single(arc, shape=SHAPE, **kw):
    """The archive on a fresh session with its delays given at creation."""
    from iterative_cleaner_amd import _native
    cube, w0, shift, d = arc
    with _native.GpuSession(*shape, device=0, delay=d, **kw) as s:
        s.upload(cube, w0, shift)
        out = s.run()
        out["amp"], out["info"] = s.fit()
        out["residual"] = s.residual()
    return out


def _refs():
    if "refs" not in _CACHE:
        _CACHE["refs"] = {name: _single(arc) for name, arc in _archives().items()}
    return _CACHE["refs"]


def _same(a, b):
    assert a["loops"] == b["loops"] and a["n_iter"] == b["n_iter"]
    assert np.array_equal(a["changed"], b["changed"]) and np.array_equal(a["nzero"], b["nzero"])
    assert bits_equal(a["weights"], b["weights"]) and bits_equal_nan(a["test"], b["test"])


def _same_state(s, ref):
    amp, info = s.fit()
    assert bits_equal_nan(amp, ref["amp"]) and bits_equal(info, ref["info"])
    assert bits_equal_nan(s.residual(), ref["residual"])


class _Pinned:
    """Page-locked copies of items (tuples of arrays), closed together."""

    def __init__(self):
        self.held = []

    def item(self, arrays):
        from iterative_cleaner_amd import _native
        out = []
        for a in arrays:
            p = _native.PinnedArray(a.shape, a.dtype)
            p.array[...] = a
            self.held.append(p)
            out.append(p.array)
        return tuple(out)

    def close(self):
        for p in self.held:
            p.close()


@pytest.fixture
def pinned():
    p = _Pinned()
    yield p
    p.close()


def test_anchor_set_delays_matches_the_oracle(oracle_lib):
    """The references of this file: a fresh session with delay=.  A's is the C
    oracle's loop (weights, amplitudes, status and residual bit for bit, the
    test values within the FFT tests' 1e-9); the four differ from each other."""
    cube, w0, shift, d = _archives()["A"]
    refs = _refs()
    ora = oracle_lib.clean_loop(cube, w0, shift, want_residual=True, want_details=True, delay=d)
    a = refs["A"]
    assert a["loops"] == ora["loops"]
    assert bits_equal(a["weights"], ora["weights"])
    assert bits_equal(a["amp"], ora["amp"]) and bits_equal(a["info"], ora["info"])
    assert bits_equal_nan(a["residual"], ora["residual"])
    t, u = a["test"], ora["test"]
    assert np.all((t == u) | (np.abs(t - u) <= 1e-9 * np.maximum(1.0, np.abs(u))) | (np.isnan(t) & np.isnan(u)))
    for x, y in ("AB", "AC", "CD", "BD"):
        assert not bits_equal(refs[x]["test"], refs[y]["test"])


def test_pipeline_alternates_per_channel_and_per_profile_delays(pinned):
    from iterative_cleaner_amd import _native, batch
    arcs, refs = _archives(), _refs()
    items = {name: pinned.item(arc) for name, arc in arcs.items()}
    assert all(len(i) == 4 for i in items.values())
    order = "ACBDCAA"
    with _native.GpuSession(*SHAPE, device=0, dedisp_fft=True) as s:
        outs = list(batch.pipeline(s, [items[n] for n in order]))
        assert len(outs) == len(order)
        for n, out in zip(order, outs):
            _same(out, refs[n])
        _same_state(s, refs["A"])
        _same(s.run(), refs["A"])                 # a re-run: the delays stay in force
        _same_state(s, refs["A"])
        s.upload(*arcs["B"][:3])                   # a synchronous upload, delays by set_delays
        s.set_delays(arcs["B"][3])
        _same(s.run(), refs["B"])
        _same_state(s, refs["B"])
        # an upload without delays keeps the session's, also when the next upload
        # brings new ones into the input slot the session's came with
        for first, second in ("AB", "CD", "CA"):
            s.upload_async(*items[first])
            _same(s.run(), refs[first])
            s.upload_async(*items[first][:3])
            s.upload_async(*items[second])
            _same(s.run(), refs[first])
            _same(s.run(), refs[second])
        # set_delays between an upload with delays and its run: the pending delays win at their run
        s.upload_async(*items["D"][:3])
        s.upload_async(*items["B"])
        s.set_delays(arcs["D"][3])
        _same(s.run(), refs["D"])
        _same(s.run(), refs["B"])


def test_queue_rules(pinned):
    from iterative_cleaner_amd import _native
    lib = _native.load_library()
    p = _native._ptr
    arcs, refs = _archives(), _refs()
    cube, w0, shift, dA = pinned.item(arcs["A"])
    bad = dA.copy()
    bad[5] = np.nan
    with _native.GpuSession(*SHAPE, device=0, dedisp_fft=True) as s:
        assert lib.ic_upload_delays_async(s.h, p(dA), 0) == -4          # nothing pending
        assert "pending" in _native._err(lib)
        s.upload_async(cube, w0, shift)
        assert lib.ic_upload_delays_async(s.h, p(bad), 0) == -1         # checked at the call, nothing queued
        assert "finite" in _native._err(lib)
        assert lib.ic_upload_delays_async(s.h, p(dA), 2) == -1
        assert lib.ic_upload_delays_async(s.h, None, 0) == -1
        assert lib.ic_upload_delays_async(s.h, p(dA), 0) == 0           # the same upload still takes delays
        assert lib.ic_upload_delays_async(s.h, p(dA), 0) == -4          # once
        _same(s.run(), refs["A"])
        assert lib.ic_upload_delays_async(s.h, p(dA), 0) == -4          # consumed: nothing pending
        for wrong in (dA.astype(np.float32), dA[::2], np.zeros((2, SHAPE[1])), list(dA)):
            with pytest.raises(ValueError):
                s.upload_async(cube, w0, shift, delay=wrong)
        assert lib.ic_upload_delays_async(s.h, p(dA), 0) == -4          # a refused delay queued no upload
    with _native.GpuSession(*SHAPE, device=0) as s:                     # integer shifts
        s.upload_async(cube, w0, shift)
        assert lib.ic_upload_delays_async(s.h, p(dA), 0) == -4
        assert "dedisp_mode" in _native._err(lib)
        s.run()
    with _native.GpuSession(*SHAPE, device=0, dedisp_fft=True) as s:    # no delays yet: the existing rule
        s.upload_async(cube, w0, shift)
        with pytest.raises(_native.NativeError, match=r"rc=-4"):
            s.run()


def test_nbin64_mixes_f32_and_quantised_items(pinned):
    """nbin 64 (the table's rows are 33 phasors), f32 items alternating with
    PSRFITS samples decoded on the GPU, every item with its delays."""
    from iterative_cleaner_amd import _native, batch, psrfits, synth
    shape = (5, 16, 64)
    nsub, nchan, nbin = shape
    refs, items = [], []
    for k in range(4):
        data, w0, shift = synth.make_cube(nsub, nchan, nbin, 720 + k, 0.2, npol=2)
        data[:, 1] += (0.37 * np.random.default_rng(k).standard_normal(data[:, 1].shape)).astype(np.float32)
        q, scl, offs = psrfits.quantise(data)
        dec = psrfits.decode(q, scl, offs)
        cube = np.ascontiguousarray((dec[:, 0] + dec[:, 1]).astype(np.float32))
        d = synth.fractional_delays(shift, nbin) + 0.07 * k
        if k >= 2:
            d = np.ascontiguousarray(d[None, :] * (1.0 + 2e-4 * np.arange(nsub))[:, None])
        zero = np.zeros(nchan, np.int32)
        refs.append(_single((cube, w0, zero, d), shape))
        if k % 2 == 0:
            items.append(pinned.item((cube, w0, zero, d)))
        else:
            items.append(pinned.item((q.astype(">i2") if k == 1 else q, scl, offs, w0, zero, d)))
    assert [len(i) for i in items] == [4, 6, 4, 6]
    order = (0, 1, 2, 3, 1, 2, 0, 3)
    with _native.GpuSession(*shape, device=0, dedisp_fft=True) as s:
        outs = list(batch.pipeline(s, [items[i] for i in order], nsum=2))
    assert len(outs) == len(order)
    for i, out in zip(order, outs):
        _same(out, refs[i])


def test_grid_cap_takes_the_table_kernel_past_its_first_trip(pinned):
    """grid_cap 2: k_phasor_table walks its 24 x 129 elements in 7 trips of two
    blocks, under set_delays (the capped references) and on the attached path;
    both give the uncapped bits."""
    from iterative_cleaner_amd import _native, batch
    arcs, refs = _archives(), _refs()
    cap = {"grid_cap": 2}
    for n in "ACBD":
        _same(_single(arcs[n], options=cap), refs[n])
    items = [pinned.item(arcs[n]) for n in "ACBD"]
    with _native.GpuSession(*SHAPE, device=0, dedisp_fft=True, options=cap) as s:
        assert s.get_option("grid_cap") == 2
        outs = list(batch.pipeline(s, items))
    for n, out in zip("ACBD", outs):
        _same(out, refs[n])


def test_equal_rows_take_the_channel_table(pinned):
    from iterative_cleaner_amd import _native
    arcs, refs = _archives(), _refs()
    cube, w0, shift, dA = arcs["A"]
    rows = np.ascontiguousarray(np.broadcast_to(dA, SHAPE[:2]))
    cube, w0, shift, rows = pinned.item((cube, w0, shift, rows))
    with _native.GpuSession(*SHAPE, device=0, dedisp_fft=True) as s:
        s.upload_async(cube, w0, shift, delay=rows)
        _same(s.run(), refs["A"])
        _same_state(s, refs["A"])


def _batch_arcs(n):
    arcs = _archives()
    return [arcs["ACBD"[k % 4]] for k in range(n)], ["ACBD"[k % 4] for k in range(n)]


@pytest.mark.parametrize("lanes", [1, 2])
def test_clean_batch_fft_matches_single_sessions(lanes):
    from iterative_cleaner_amd import batch
    refs = _refs()
    arcs, names = _batch_arcs(7)
    got = list(batch.clean_batch(iter(arcs), SHAPE, device=0, lanes=lanes, dedisp="fft"))
    assert len(got) == 7
    for n, out in zip(names, got):
        _same(out, refs[n])


def test_clean_batch_fft_passes_the_fit_mode_on_and_checks_its_items():
    from iterative_cleaner_amd import _native, batch
    arcs, names = _batch_arcs(3)
    got = list(batch.clean_batch(iter(arcs), SHAPE, device=0, dedisp="fft", fit_mode=_native.FIT_CLOSED))
    assert len(got) == 3
    differs = False
    for arc, n, out in zip(arcs, names, got):
        ref = _single(arc, fit_mode=_native.FIT_CLOSED)
        _same(out, ref)
        differs = differs or not bits_equal_nan(ref["test"], _refs()[n]["test"])
    assert differs                       # the closed-form fit is not the exact fit's arithmetic
    with pytest.raises(ValueError, match="delays"):
        list(batch.clean_batch(iter([arcs[0][:3]]), SHAPE, device=0, dedisp="fft"))
    with pytest.raises(ValueError, match="fft"):
        list(batch.clean_batch(iter([arcs[0]]), SHAPE, device=0))


@pytest.mark.parametrize("periods", ["constant", "per_row"])
def test_psrfits_files_end_to_end(tmp_path, oracle_lib, periods):
    """Three foreign PSRFITS files (DM, channel frequencies, folding periods; no
    stand-in columns) through psrfits_loader and clean_batch: the zap masks of
    the C oracle's loop on the decoded, pscrunched cube with the files' delays."""
    from iterative_cleaner_amd import archive as ica
    from iterative_cleaner_amd import batch, psrfits, synth
    shape = (10, 64, 256)
    paths, want = [], []
    for k in range(3):
        data, w, _ = synth.make_cube(*shape, 61 + k, 0.2, npol=2)
        path = str(tmp_path / ("dm%d.sf" % k))
        ar = ica.Archive(data, w, np.zeros(64, np.int64), filename=os.path.basename(path))
        ar._chan_freqs = 1300.0 + np.arange(64) * 3.0
        ar._period = 0.0125 if periods == "constant" else 0.0125 * (1.0 + 3e-4 * np.cos(np.arange(10) + k))
        ar._dm = 20.0
        psrfits.save(ar, path, stand_in_meta=False)
        src = psrfits.load(path)
        delay = src.get_dm_delay()
        assert delay.shape == ((64,) if periods == "constant" else (10, 64))
        dec = src.get_data()
        cube = (dec[:, 0] + dec[:, 1]).astype(np.float32)
        want.append(oracle_lib.clean_loop(cube, src.get_weights(), src.get_dm_shift(), delay=delay))
        paths.append(path)
    got = list(batch.clean_batch(batch.psrfits_loader(paths, "fft"), shape, device=0, quantised=True, nsum=2,
                                 dedisp="fft"))
    assert len(got) == 3
    for out, ref in zip(got, want):
        assert out["loops"] == ref["loops"]
        assert bits_equal(out["weights"], ref["weights"])
