"""Host side of the quantised uploads (no GPU): the PSRFITS reader hands out the
samples as stored, the archive knows while they still are its data, and the
batch scheduler sends five-element items to upload_quantised_async."""
import re
import threading

import numpy as np
import pytest

from helpers import bits_equal


def _file(tmp_path, npol=2, name="obs.sf", **kw):
    from iterative_cleaner_amd import synth
    path = str(tmp_path / name)
    synth.make_archive(5, 12, 32, seed=11, rfi_frac=0.2, npol=npol, filename=path, **kw).unload(path)
    return path


@pytest.mark.parametrize("channels", [None, (3, 10)])
def test_load_quantised_returns_what_load_decodes(tmp_path, channels):
    from iterative_cleaner_amd import psrfits
    path = _file(tmp_path)
    ar = psrfits.load(path, channels=channels)
    q0, scl0, offs0 = ar._psrfits_q
    q, scl, offs, weights, shift, meta = psrfits.load_quantised(path, channels=channels)
    assert q.dtype.kind == "i" and q.dtype.itemsize == 2
    assert q.shape == q0.shape and q.flags.c_contiguous
    assert bits_equal(q.astype(np.int16), q0)                   # after the byte-order conversion, if any
    assert bits_equal(scl, scl0) and bits_equal(offs, offs0)
    assert bits_equal(weights, ar.get_weights()) and bits_equal(shift, ar.get_dm_shift())
    assert meta["state"] == ar.get_state() and meta["npol"] == 2
    assert meta["dedispersed"] == ar.get_dedispersed() and meta["baseline_duty"] == ar.get_baseline_duty()
    assert bits_equal(psrfits.decode(q.astype(np.int16), scl, offs), ar.get_data())
    if channels is not None:
        whole = psrfits.load_quantised(path)
        assert np.array_equal(q, whole[0][:, :, 3:10]) and bits_equal(weights, whole[3][:, 3:10])


def test_get_quantised_follows_the_samples(tmp_path):
    from iterative_cleaner_amd import psrfits, synth
    from iterative_cleaner_amd import archive as ica
    two, one = _file(tmp_path), _file(tmp_path, npol=1, name="one.sf")

    ar = psrfits.load(two)
    got = ar.get_quantised()
    assert got is not None and all(a is b for a, b in zip(got, ar._psrfits_q))
    assert bits_equal(psrfits.decode(*got), ar.get_data())
    assert ar.clone().get_quantised() is not None
    ar.get_data()[0, 0, 0, 0] = 7.0                             # get_data hands out a copy
    ar.get_weights()
    ar.get_Integration(0).set_weight(1, 0.0)                    # weights are not samples
    ar.get_Profile(0, 0, 1).get_weight()
    assert ar.get_quantised() is not None

    ar1 = psrfits.load(one)
    ar1.pscrunch()                                              # one polarisation: nothing to add
    assert ar1.get_quantised() is not None

    def after(call, path=two):
        a = psrfits.load(path)
        assert a.get_quantised() is not None
        call(a)
        return a.get_quantised()

    assert after(lambda a: a.pscrunch()) is None
    assert after(lambda a: a.dedisperse()) is None
    assert after(lambda a: (a.dedisperse(), a.dededisperse())) is None
    assert after(lambda a: a.remove_baseline()) is None
    assert after(lambda a: a.fscrunch()) is None
    assert after(lambda a: a.tscrunch()) is None
    assert after(lambda a: a.get_Profile(1, 0, 2).get_amps()) is None
    assert after(lambda a: a.dededisperse()) is not None        # already dispersed: nothing moved
    assert synth.make_archive(5, 12, 32, npol=2).get_quantised() is None
    assert ica.Archive(np.zeros((1, 1, 2, 8), np.float32)).get_quantised() is None
    # the written view really is why get_amps must end it
    a = psrfits.load(two)
    a.get_Profile(0, 0, 0).get_amps()[:] = 0.0
    assert not bits_equal(psrfits.decode(*a._psrfits_q), a.get_data())


def test_cleaner_chooses_nsum_by_the_state(tmp_path):
    from iterative_cleaner_amd import cleaner, psrfits, synth
    from iterative_cleaner_amd import archive as ica
    q, scl, offs, nsum = cleaner._quantised_input(psrfits.load(_file(tmp_path)))
    assert nsum == 2 and q.shape == (5, 2, 12, 32)
    assert cleaner._quantised_input(psrfits.load(_file(tmp_path, npol=1, name="one.sf")))[3] == 1
    data, w, shift = synth.make_cube(5, 12, 32, 3, 0.2, npol=4)
    path = str(tmp_path / "iquv.sf")
    ica.Archive(data, w, shift, filename=path, state="Stokes").unload(path)
    assert cleaner._quantised_input(psrfits.load(path))[3] == 1
    assert cleaner._quantised_input(synth.make_archive(5, 12, 32, npol=2)) is None


class FakeSession:
    """Records which upload each item took (the protocol of
    tests/test_batch_host.py's stand-in)."""

    def __init__(self):
        self.queue, self.calls = [], []
        self.lock = threading.Lock()

    def upload_async(self, tag, *rest):
        assert len(rest) == 2
        with self.lock:
            assert len(self.queue) < 2, "more than two uploads in flight"
            self.queue.append(tag)
            self.calls.append(("f32", tag, None))

    def upload_quantised_async(self, tag, scl, offs, w0, shift, nsum):
        with self.lock:
            assert len(self.queue) < 2, "more than two uploads in flight"
            self.queue.append(tag)
            self.calls.append(("q", tag, nsum))

    def run(self, fetch=True):
        with self.lock:
            return {"tag": self.queue.pop(0)}


@pytest.mark.parametrize("lanes", [1, 2, 3])
def test_lanes_dispatch_on_the_item(lanes):
    from iterative_cleaner_amd import batch
    items = [(k, None, None) if k % 3 else (k, "scl", "offs", None, None) for k in range(20)]
    sessions = [FakeSession() for _ in range(lanes)]
    got = [out["tag"] for out in batch.run_lanes(sessions, items, nsum=2)]
    assert got == list(range(20))
    calls = sorted((c for s in sessions for c in s.calls), key=lambda c: c[1])
    assert calls == [("f32", k, None) if k % 3 else ("q", k, 2) for k in range(20)]
    s = FakeSession()
    assert [o["tag"] for o in batch.pipeline(s, items)] == list(range(20))
    assert [c[2] for c in s.calls if c[0] == "q"] == [1] * 7      # nsum defaults to one polarisation


def test_header_documents_the_new_entry_points():
    import os

    from iterative_cleaner_amd import _native
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(here, "include", "iterative_cleaner.h")) as fh:
        text = fh.read()
    for name in ("ic_upload_quantised", "ic_upload_quantised_async", "ic_decode_profiles"):
        assert re.search(r"\bint %s\(" % name, text) and name in _native.EXPORTS
    assert re.search(r"#define IC_ABI_VERSION 9\b", text) and _native.ABI_VERSION == 9
    assert re.search(r"#define IC_Q_BIG_ENDIAN 1\b", text) and _native.Q_BIG_ENDIAN == 1
