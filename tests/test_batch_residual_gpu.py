"""GPU tests of residuals from the batch scheduler (clean_batch(...,
residuals=True)): every archive's encoded residual equals the one a single
session gives it (residual_quantised(big_endian=True), itself held to the
host's psrfits.quantise by test_encode_gpu / test_residual_async_gpu), in input
order, and asking for residuals changes nothing else."""
import numpy as np
import pytest

from helpers import bits_equal, bits_equal_nan

pytestmark = pytest.mark.gpu

SHAPE = (6, 96, 128)
N = 5
KINDS = ("exact", "closed", "quantised", "fft-channel", "fft-profile")
_CACHE = {}


def _setup(kind):
    """(loader items, clean_batch keywords, single-session references) of a
    kind, built once and never modified."""
    if kind in _CACHE:
        return _CACHE[kind]
    from iterative_cleaner_amd import _native, psrfits, synth
    nsub, nchan, nbin = SHAPE
    items, refs, kw, skw = [], [], {}, {}
    if kind == "closed":
        kw["fit_mode"] = skw["fit_mode"] = _native.FIT_CLOSED
    if kind == "quantised":
        kw.update(quantised=True, nsum=2)
    if kind.startswith("fft"):
        kw["dedisp"] = "fft"
    for k in range(N):
        data, w0, shift = synth.make_cube(*SHAPE, seed=200 + k, rfi_frac=0.1 + 0.05 * (k % 3),
                                          npol=2 if kind == "quantised" else 1)
        if kind == "quantised":
            rng = np.random.default_rng(900 + k)
            data[:, 1] += (0.37 * rng.standard_normal(data[:, 1].shape)).astype(np.float32)
            q, scl, offs = psrfits.quantise(data)
            items.append((q, scl, offs, w0, shift))
        elif kind.startswith("fft"):
            d = synth.fractional_delays(shift, nbin) + 0.11 * k
            if kind == "fft-profile":
                d = np.ascontiguousarray(d[None, :] * (1.0 + 3e-4 * np.arange(nsub))[:, None])
            items.append((np.ascontiguousarray(data[:, 0]), w0, np.zeros(nchan, np.int32), d))
        else:
            items.append((np.ascontiguousarray(data[:, 0]), w0, shift))
    for item in items:
        dk = {"delay": item[3]} if kind.startswith("fft") else {}
        with _native.GpuSession(*SHAPE, device=0, **skw, **dk) as s:
            if kind == "quantised":
                s.upload_quantised(*item, 2)
            else:
                s.upload(*item[:3])
            out = s.run()
            assert out["n_iter"] >= 1
            out["residual_q"] = s.residual_quantised(big_endian=True)
        refs.append(out)
    assert not bits_equal(refs[0]["residual_q"][0], refs[1]["residual_q"][0])
    _CACHE[kind] = (items, kw, refs)
    return _CACHE[kind]


def _same_triple(got, want):
    assert got[0].dtype == np.dtype(">i2") and got[0].shape == SHAPE
    assert got[0].tobytes() == want[0].tobytes(), "%d samples differ" % int((got[0] != want[0]).sum())
    assert bits_equal_nan(got[1], want[1]) and bits_equal_nan(got[2], want[2])


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("kind", KINDS)
def test_batch_residuals_match_single_sessions(kind, lanes):
    from iterative_cleaner_amd import batch
    items, kw, refs = _setup(kind)
    plain = list(batch.clean_batch(iter(items), SHAPE, device=0, lanes=lanes, **kw))
    assert all("residual_q" not in o for o in plain)
    n = 0
    for k, out in enumerate(batch.clean_batch(iter(items), SHAPE, device=0, lanes=lanes, residuals=True, **kw)):
        _same_triple(out["residual_q"], refs[k]["residual_q"])       # compared while the views are valid
        for other in (refs[k], plain[k]):                             # residuals change nothing else
            assert out["loops"] == other["loops"] and np.array_equal(out["changed"], other["changed"])
            assert bits_equal(out["weights"], other["weights"]) and bits_equal(out["test"], other["test"])
        n += 1
    assert n == N


def test_native_byte_order():
    from iterative_cleaner_amd import batch
    items, kw, refs = _setup("exact")
    for k, out in enumerate(batch.clean_batch(iter(items[:3]), SHAPE, device=0, residuals=True,
                                              residual_big_endian=False)):
        q = out["residual_q"][0]
        assert q.dtype == np.int16 and bits_equal(q, refs[k]["residual_q"][0].astype(np.int16))


@pytest.mark.parametrize("lanes", [1, 2])
def test_views_and_their_life(lanes, tmp_path):
    """A yielded triple is a view into the batch's page-locked ring: intact for
    as long as the generator has not been advanced (the lanes go on cleaning
    behind it), written as it is by psrfits.save_quantised; stopping after the
    second item closes cleanly."""
    from iterative_cleaner_amd import batch, psrfits
    items, kw, refs = _setup("exact")
    gen = batch.clean_batch(iter(items), SHAPE, device=0, lanes=lanes, residuals=True)
    first = next(gen)
    q, scl, offs = first["residual_q"]
    assert not q.flags.owndata and q.flags.c_contiguous
    snap = tuple(a.copy() for a in (q, scl, offs))
    _same_triple(snap, refs[0]["residual_q"])
    second = next(gen)                              # the lanes are now archives ahead of the consumer
    _same_triple(second["residual_q"], refs[1]["residual_q"])
    path = str(tmp_path / "res.sf")
    _, w0, shift = items[1]
    psrfits.save_quantised(path, *second["residual_q"], w0, shift)
    back = psrfits.load_quantised(path)
    assert bits_equal(np.asarray(back[0]).astype(np.int16)[:, 0], refs[1]["residual_q"][0].astype(np.int16))
    assert bits_equal(np.asarray(back[1])[:, 0], refs[1]["residual_q"][1])
    assert bits_equal(np.asarray(back[2])[:, 0], refs[1]["residual_q"][2])
    _same_triple(second["residual_q"], refs[1]["residual_q"])       # still intact: next() not called since
    gen.close()
