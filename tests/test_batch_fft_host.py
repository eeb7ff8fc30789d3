"""Host side of the batches of archives with fractional delays: the C-ABI
declares ic_upload_delays_async; batch.pipeline / run_lanes hand an item's
trailing delays to the session's upload call by keyword, and only when the item
has them; clean_batch refuses an unknown dedispersion before it touches the
GPU; batch.psrfits_loader yields a PSRFITS list's samples with the delays their
DM, frequencies and periods give, and names a file of the other mode."""
import os
import random
import re
import threading

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_entry_point():
    from iterative_cleaner_amd import _native
    with open(os.path.join(REPO, "include", "iterative_cleaner.h")) as fh:
        text = fh.read()
    assert re.search(r"\bint ic_upload_delays_async\(", text)
    assert "ic_upload_delays_async" in _native.EXPORTS
    assert re.search(r"#define IC_ABI_VERSION 9\b", text) and _native.ABI_VERSION == 9


class FakeSession:
    """Records the upload calls of one session: (call, tag, nsum, the delay
    keyword or the marker NO_KW when the call came without it)."""

    NO_KW = "no-keyword"

    def __init__(self):
        self.queue = []
        self.calls = []
        self.lock = threading.Lock()

    def _push(self, call, tag, nsum, delay):
        with self.lock:
            assert len(self.queue) < 2, "more than two uploads in flight"
            self.queue.append(tag)
            self.calls.append((call, tag, nsum, delay))

    def upload_async(self, cube, w0, shift, *, delay=NO_KW):
        self._push("f32", cube, None, delay)

    def upload_quantised_async(self, q, scl, offs, w0, shift, nsum, *, delay=NO_KW):
        assert (scl, offs) == ("scl", "offs")
        self._push("q", q, nsum, delay)

    def run(self, fetch=True):
        with self.lock:
            tag = self.queue.pop(0)
        return {"tag": tag}


def _items(n):
    """Items of lengths 3, 4, 5, 6 in turn, tagged by their position."""
    out = []
    for k in range(n):
        kind = k % 4
        if kind == 0:
            out.append((k, "w0", "shift"))
        elif kind == 1:
            out.append((k, "w0", "shift", "delay-%d" % k))
        elif kind == 2:
            out.append((k, "scl", "offs", "w0", "shift"))
        else:
            out.append((k, "scl", "offs", "w0", "shift", "delay-%d" % k))
    return out


def _expected(k):
    kind = k % 4
    call = "f32" if kind < 2 else "q"
    return (call, k, None if kind < 2 else 2, "delay-%d" % k if kind in (1, 3) else FakeSession.NO_KW)


def test_pipeline_hands_the_delay_on_by_keyword_only_when_present():
    from iterative_cleaner_amd import batch
    s = FakeSession()
    got = [out["tag"] for out in batch.pipeline(s, _items(9), nsum=2)]
    assert got == list(range(9))
    assert s.calls == [_expected(k) for k in range(9)]
    assert not s.queue


@pytest.mark.parametrize("lanes", [1, 2, 3])
def test_run_lanes_hands_the_delay_on(lanes):
    from iterative_cleaner_amd import batch
    random.seed(lanes)
    sessions = [FakeSession() for _ in range(lanes)]
    got = [out["tag"] for out in batch.run_lanes(sessions, _items(22), nsum=2)]
    assert got == list(range(22))
    calls = sorted((c for s in sessions for c in s.calls), key=lambda c: c[1])
    assert calls == [_expected(k) for k in range(22)]
    assert all(not s.queue for s in sessions)


def test_items_of_another_length_are_refused():
    from iterative_cleaner_amd import batch
    for bad in ((0, "w0"), (0, 1, 2, 3, 4, 5, 6)):
        with pytest.raises(ValueError):
            list(batch.pipeline(FakeSession(), [bad]))


def test_clean_batch_rejects_an_unknown_dedispersion_before_the_gpu(monkeypatch):
    from iterative_cleaner_amd import _native, batch

    def no_gpu(*a, **k):
        raise AssertionError("the GPU library was touched")

    monkeypatch.setattr(_native, "load_library", no_gpu)
    monkeypatch.setattr(_native, "GpuSession", no_gpu)
    monkeypatch.setattr(_native, "PinnedArray", no_gpu)
    gen = batch.clean_batch(iter([]), (4, 8, 64), dedisp="psrchive")
    with pytest.raises(ValueError, match="dedisp"):
        next(gen)
    with pytest.raises(ValueError, match="dedisp"):
        next(batch.psrfits_loader([], "psrchive"))


def _foreign_file(path, periods, dm=20.0, nsub=5, seed=61):
    """A PSRFITS file without the stand-in's columns (tests/test_psrfits_gpu.py):
    DM, 64 channels near 1400 MHz, nbin 256."""
    from iterative_cleaner_amd import archive as ica
    from iterative_cleaner_amd import psrfits, synth
    data, w, _ = synth.make_cube(nsub, 64, 256, seed, 0.2, npol=2)
    ar = ica.Archive(data, w, np.zeros(64, np.int64), filename=os.path.basename(path))
    ar._chan_freqs = 1300.0 + np.arange(64) * 3.0
    ar._period = 0.0125 if periods == "constant" else 0.0125 * (1.0 + 3e-4 * np.cos(np.arange(nsub)))
    ar._dm = dm
    psrfits.save(ar, path, stand_in_meta=False)
    return ar


def test_psrfits_loader_yields_the_files_delays(tmp_path):
    from iterative_cleaner_amd import batch, dedispersion, psrfits
    paths = [str(tmp_path / "const.sf"), str(tmp_path / "rows.sf")]
    ars = [_foreign_file(paths[0], "constant"), _foreign_file(paths[1], "per_row", seed=62)]
    items = list(batch.psrfits_loader(paths, "fft"))
    assert [len(i) for i in items] == [6, 6]
    for path, ar, item, shape in zip(paths, ars, items, ((64,), (5, 64))):
        q, scl, offs, w0, shift, delay = item
        want = dedispersion.delays_from_dm(20.0, ar._chan_freqs, 1400.0, np.broadcast_to(ar._period, (5,)), 256)
        assert delay.shape == shape and delay.dtype == np.float64 and delay.flags.c_contiguous
        assert np.array_equal(delay, want[0] if shape == (64,) else want)
        assert np.any(delay != np.rint(delay))
        ref = psrfits.load_quantised(path)
        assert q.dtype == np.dtype(">i2") and q.shape == (5, 2, 64, 256) and np.array_equal(q, ref[0])
        assert np.array_equal(scl, ref[1]) and np.array_equal(offs, ref[2]) and np.array_equal(w0, ref[3])
        assert np.array_equal(shift, np.zeros(64))


def test_psrfits_loader_names_a_file_of_the_other_mode(tmp_path):
    from iterative_cleaner_amd import batch
    frac, whole = str(tmp_path / "frac.sf"), str(tmp_path / "dm0.sf")
    _foreign_file(frac, "constant")
    _foreign_file(whole, "constant", dm=0.0)
    with pytest.raises(ValueError, match="dm0.sf"):
        list(batch.psrfits_loader([frac, whole], "fft"))
    with pytest.raises(ValueError, match="frac.sf"):
        list(batch.psrfits_loader([whole, frac], "shift"))
    items = list(batch.psrfits_loader([whole], "shift"))
    assert [len(i) for i in items] == [5]
