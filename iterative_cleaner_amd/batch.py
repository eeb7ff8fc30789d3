"""Batch scheduler for many archives of one shape on one GPU (config C4,
SURVEY.md §8(e)/(f) rank 4).

The reference cleans its archive list one after the other, reloading and
re-processing each (iterative_cleaner.py:59-62).  Here one session is reused
for every archive of a shape, and the host->device copy of archive k+1 runs on
the session's copy stream while archive k is cleaned (ic_upload_async, two
device input slots).  Archives may also go up as the int16 samples PSRFITS
stores (ic_upload_quantised_async), decoded on the copy stream: half the bytes
per archive.  Host staging goes through a ring of page-locked buffers
filled by a loader thread, so reading/decoding archive k+2 overlaps too.

A C4 archive (128 x 1024 x 512) is too small to fill an MI355X on its own:
its later fit rounds, the tail and the small reductions leave most CUs idle.
`lanes` > 1 runs that many sessions, each on its own HIP streams and host
thread (ctypes drops the GIL during ic_run), pulling archives from one queue,
so the kernels of different archives overlap on the GPU.  Results come back in
input order.  Under torchrun every rank runs its own batch (dist.shard of the
list): no collective.
"""
from __future__ import annotations

import queue
import sys
import threading
import time

import numpy as np

from . import _native

# how long closing the lanes waits, in all, for the workers' current ic_run calls (seconds)
JOIN_TIMEOUT_S = 600.0

# sessions of lanes that were still inside ic_run when the lanes closed, with
# every host array their queued copies and runs may still read: kept alive
# (never freed, never destroyed) for the life of the process
_LEAKED = []


def _queue_upload(session, arrays, nsum):
    """Queue one item's upload: (cube, w0, shift[, delay]) f32, or the PSRFITS
    samples (q, scl, offs, w0, shift[, delay]), decoded on the GPU.  A trailing
    delay (f64, per channel or per profile) goes up with the archive
    (ic_upload_delays_async); it is passed on, by keyword, only when the item
    has one."""
    n = len(arrays)
    if n not in (3, 4, 5, 6):
        raise ValueError("a batch item holds 3 or 4 arrays (cube, w0, shift[, delay]) or 5 or 6 "
                         "(q, scl, offs, w0, shift[, delay]), not %d" % n)
    kw = {"delay": arrays[-1]} if n in (4, 6) else {}
    if n >= 5:
        session.upload_quantised_async(*arrays[:5], nsum, **kw)
    else:
        session.upload_async(*arrays[:3], **kw)


def _residual_slots(session, residuals):
    """The (q, scl, offs) triples one session downloads its residuals into,
    checked (GpuSession.residual_quantised_async's rules): at least 2, because
    one is in flight while the consumer still holds the one yielded before."""
    slots = [tuple(t) for t in residuals]
    if len(slots) < 2:
        raise ValueError("residuals needs at least 2 (q, scl, offs) triples per session, not %d" % len(slots))
    for t in slots:
        if len(t) != 3:
            raise ValueError("a residual slot is a (q, scl, offs) triple, not %d arrays" % len(t))
        _native.check_residual_arrays(session.shape, *t, "residuals")
    return slots


class _ResidualQueue:
    """One session's residual downloads, one in flight at a time.  queue(out)
    after run() of archive k starts its encode and download into the next slot
    (round-robin) and returns True - or False for a run without an iteration,
    which has no residual (run_loop's rule).  land() waits for the download in
    flight and returns its dict, now holding out["residual_q"] = (q, scl,
    offs), or None.  Calling land() after the run of archive k+1 leaves the
    download of k the whole of that run (and the upload of k+2) to overlap."""

    def __init__(self, session, slots):
        self.session, self.slots = session, slots
        self.n = 0              # residuals queued so far
        self.inflight = None    # (dict, slot index)

    def next_slot(self):
        return self.n % len(self.slots)

    def queue(self, out):
        if out.get("n_iter", 0) <= 0:
            return False
        j = self.next_slot()
        self.session.residual_quantised_async(*self.slots[j])
        self.n += 1
        self.inflight = (out, j)
        return True

    def land(self):
        if self.inflight is None:
            return None, None
        out, j = self.inflight
        self.session.residual_wait()
        self.inflight = None
        out["residual_q"] = self.slots[j]
        return out, j


def pipeline(session, items, fetch=True, nsum=1, residuals=None, detrend=None, detrend_pieces=None,
             std_template=None, hotbins=None, dynspec=False):
    """Clean every item of `items` on `session`, overlapping each archive's
    upload with the previous archive's cleaning.  An item is (cube, w0, shift),
    or (q, scl, offs, w0, shift): int16 PSRFITS samples with their scales and
    offsets (GpuSession.upload_quantised_async; `nsum` polarisations summed);
    both kinds may alternate.  On a session of the FFT dedispersion
    (GpuSession(dedisp_fft=True)) an item may end in its archive's fractional
    delays, f64 (nchan,) or (nsub, nchan): (cube, w0, shift, delay) or (q, scl,
    offs, w0, shift, delay); they are copied, and the channel phasor table built,
    behind the archive's copy, and become the session's delays for that archive
    and after it.  The arrays must stay valid until their result is
    yielded (page-locked for the copies to overlap).  Yields the ic_run dicts in
    order.

    residuals: a sequence of at least 2 (q, scl, offs) triples, used round-robin
    (GpuSession.residual_quantised_async: int16 native or '>i2' (nsub, nchan,
    nbin), f32 (nsub, nchan); page-locked for the download to overlap).  After
    run() of archive k its residual is encoded on the GPU and its download
    queued; the dict of archive k is yielded with out["residual_q"] = (q, scl,
    offs) once that has landed, which is after the clean of archive k+1 has
    been issued: the download runs beside that clean and the upload of k+2.
    The triple is valid until the generator is advanced twice more (with 2
    slots: once more).  An archive whose run made no iteration has no
    "residual_q".

    detrend = (chan_order, subint_order[, rounds, clip]): set on the session
    before the first run (GpuSession.set_detrend); None leaves the session as
    it is.  detrend_pieces = (chan, subint): likewise
    (GpuSession.set_detrend_pieces).  std_template: the standard profile every
    archive is cleaned against (GpuSession.set_std_template; a profile, a path,
    or a pair with the align mode), set once before the first run and aligned
    against each archive; every dict then holds out["std_alignment"].  None
    leaves the session as it is (clean_batch and run_loop are where the
    IC_STD_TEMPLATE switch is read).  hotbins = (threshold, on_start, on_end[,
    rounds]): the hot-bin repair (GpuSession.set_hotbins; hotbins.py), set
    before the first run; every archive gets its own pass when its upload is
    consumed, and every dict then holds out["hotbins"].  None leaves the
    session as it is (clean_batch and run_loop read the IC_HOTBINS switch).
    dynspec=True: every dict holds out["dynspec"] = dict(amp, err, base), the
    dynamic spectrum of its archive (GpuSession.dynspec; dynspec.py), taken
    right after the archive's run."""
    if hotbins is not None:
        session.set_hotbins(*hotbins)
    if std_template is not None:
        from .std_template import normalise
        session.set_std_template(*normalise(std_template, session.shape[2]))
    if detrend is not None:
        session.set_detrend(*detrend)
    if detrend_pieces is not None:
        session.set_detrend_pieces(*detrend_pieces)
    rq = _ResidualQueue(session, _residual_slots(session, residuals)) if residuals is not None else None

    def after_run(out):
        if rq is None:
            yield out
            return
        landed, _ = rq.land()
        queued = rq.queue(out)   # before the yield: it travels while the consumer works on `landed`
        if landed is not None:
            yield landed
        if not queued:
            yield out

    it = iter(items)
    first = next(it, None)
    if first is None:
        return
    _queue_upload(session, first, nsum)
    for nxt in it:
        _queue_upload(session, nxt, nsum)
        yield from after_run(_run(session, fetch, dynspec))
    yield from after_run(_run(session, fetch, dynspec))
    if rq is not None:
        landed, _ = rq.land()
        if landed is not None:
            yield landed


def _run(session, fetch, dynspec):
    """session.run(fetch), with the archive's dynamic spectrum when asked for
    (the session still holds the cube, template and weights of that run)."""
    out = session.run(fetch)
    if dynspec and out.get("n_iter", 0) > 0:
        out["dynspec"] = session.dynspec()
    return out


_EXITED = -2   # a worker's last message (run_lanes)


def run_lanes(sessions, items, fetch=True, stop=None, join_timeout=None, nsum=1, residuals=None,
              std_template=None, hotbins=None, dynspec=False):
    """Clean every item of `items` ((cube, w0, shift) or (q, scl, offs, w0, shift),
    each with or without trailing delays, as `pipeline`) on `len(sessions)` sessions of one
    shape concurrently (one host thread per session, shared work queue; each
    session overlaps its next upload with its current run).  The arrays must
    stay valid until their result is yielded.  Yields the ic_run dicts in input
    order.  One session: exactly `pipeline`.

    residuals: per session a sequence of at least 2 (q, scl, offs) triples, as
    `pipeline`'s: every dict comes with out["residual_q"], a triple of its
    lane, valid until the generator is advanced past it - a lane takes a slot
    again only after the consumer has moved on from the result that held it.

    std_template, hotbins: `pipeline`'s, set on every session before the first run.
    dynspec: `pipeline`'s.

    On a worker error, or when the consumer stops early (generator closed), the
    lanes stop: the `stop` event (created here if not given) is set, queued work
    is dropped, and the generator returns only after every worker thread has
    exited - a worker finishes at most the run it is in, so no thread is inside
    ic_run when the caller closes the sessions.  The workers share one deadline
    (`join_timeout`, default JOIN_TIMEOUT_S): a lane still inside ic_run then is
    leaked, its session marked (`_ic_leaked`, handle dropped so nothing
    destroys it under the running call) and, with the arrays it was handed,
    kept in _LEAKED."""
    if residuals is not None and len(residuals) != len(sessions):
        raise ValueError("residuals needs one sequence of (q, scl, offs) triples per session (%d), not %d"
                         % (len(sessions), len(residuals)))
    if std_template is not None:
        from .std_template import normalise
        for sess in sessions:
            sess.set_std_template(*normalise(std_template, sess.shape[2]))
    if hotbins is not None:
        for sess in sessions:
            sess.set_hotbins(*hotbins)
    if len(sessions) == 1:
        yield from pipeline(sessions[0], items, fetch, nsum, None if residuals is None else residuals[0],
                            dynspec=dynspec)
        return
    rqs = None
    if residuals is not None:
        rqs = [_ResidualQueue(sess, _residual_slots(sess, r)) for sess, r in zip(sessions, residuals)]
        # slot j of lane q is free: taken by the worker before it queues a
        # download into it, given back by the consumer once it has moved on
        slot_free = [[threading.Semaphore(1) for _ in rq.slots] for rq in rqs]
    rslot = {}   # archive index -> (lane, slot) of its residual, until the consumer has moved on
    stop = stop if stop is not None else threading.Event()
    work = queue.Queue(maxsize=2 * len(sessions))
    done = queue.Queue()

    held = [[] for _ in sessions]   # per lane: the arrays of its uploads not yet consumed by a run

    def worker(lane, sess):
        pending = None   # index uploaded to this session, not yet run
        rq = rqs[lane] if rqs is not None else None
        flying = None    # index of the archive whose residual download is in flight

        def land():
            nonlocal flying
            out, j = rq.land()
            if out is not None:
                rslot[flying] = (lane, j)
                done.put((flying, out))
                flying = None

        def finish(idx, out):
            """hand over a run's result: at once, or with residuals the one before it"""
            nonlocal flying
            if rq is None:
                done.put((idx, out))
                return
            land()   # first: the consumer may need it to free the slot waited for below
            sem = slot_free[lane][rq.next_slot()]
            while out.get("n_iter", 0) > 0 and not sem.acquire(timeout=0.1):
                if stop.is_set():
                    return
            if rq.queue(out):
                flying = idx
            else:
                done.put((idx, out))

        try:
            while not stop.is_set():
                try:
                    item = work.get_nowait()
                except queue.Empty:
                    if pending is not None:   # nothing queued: run what we hold
                        finish(pending, _run(sess, fetch, dynspec))
                        pending = None
                        continue
                    if flying is not None:    # nothing to overlap it with: hand it over
                        land()
                        continue
                    item = work.get()
                if item is None or stop.is_set():
                    break
                idx, arrays = item
                held[lane].append(arrays)
                del held[lane][:-3]             # an upload is consumed by the second run after it
                _queue_upload(sess, arrays, nsum)
                if pending is not None:
                    finish(pending, _run(sess, fetch, dynspec))
                pending = idx
            if pending is not None and not stop.is_set():
                finish(pending, _run(sess, fetch, dynspec))
            if flying is not None and not stop.is_set():
                land()
        except BaseException as e:  # noqa: BLE001 - re-raised by the consumer
            stop.set()
            done.put((-1, e))
        finally:
            done.put((_EXITED, lane))   # the consumer counts the live workers down without polling

    threads = [threading.Thread(target=worker, args=(q, sess), daemon=True) for q, sess in enumerate(sessions)]
    for th in threads:
        th.start()
    n = 0
    feed_error = []

    def put(item):
        while not stop.is_set():
            try:
                work.put(item, timeout=0.1)
                return True
            except queue.Full:
                continue
        return False

    def feed():
        nonlocal n
        try:
            for arrays in items:
                if not put((n, arrays)):
                    return
                n += 1
        except BaseException as e:  # noqa: BLE001
            feed_error.append(e)
            stop.set()
        finally:
            for _ in threads:
                if not put(None):
                    break

    feeder = threading.Thread(target=feed, daemon=True)
    feeder.start()
    ready, nxt, live = {}, 0, len(threads)
    try:
        while True:
            if nxt in ready:
                yield ready.pop(nxt)
                if nxt in rslot:          # the consumer has moved on: its residual's slot is free
                    lane, j = rslot.pop(nxt)
                    slot_free[lane][j].release()
                nxt += 1
                continue
            if live == 0:
                feeder.join()   # past its items (or stopped): it returns within one put timeout
                break
            idx, out = done.get()
            if idx == _EXITED:
                live -= 1
                continue
            if idx < 0:
                raise out
            ready[idx] = out
        if feed_error:
            raise feed_error[0]
        if ready or nxt != n:
            raise RuntimeError("batch lanes lost archives %d..%d" % (nxt, n - 1))
    finally:
        stop.set()
        while True:                       # drop queued work; wake blocked workers
            try:
                work.get_nowait()
            except queue.Empty:
                break
        for _ in threads:
            try:
                work.put_nowait(None)
            except queue.Full:
                break
        limit = JOIN_TIMEOUT_S if join_timeout is None else float(join_timeout)
        deadline = time.monotonic() + limit   # one deadline for every lane
        for q, (th, sess) in enumerate(zip(threads, sessions)):
            th.join(timeout=max(0.0, deadline - time.monotonic()))   # at most the run a worker is in
            if th.is_alive():
                # a worker stuck inside ic_run: leak its session (never destroyed
                # under a running call) and keep what it may still read alive,
                # rather than hang the caller's cleanup
                sys.stderr.write("iterative_cleaner: batch lane %d still inside ic_run after %.0f s; "
                                 "leaking its session\n" % (q, limit))
                _LEAKED.append((sess, getattr(sess, "h", None),
                                list(held[q]) + (list(residuals[q]) if residuals is not None else [])))
                if hasattr(sess, "h"):
                    sess.h = None
                sess._ic_leaked = True
        feeder.join(timeout=5.0)          # may wait in `items`: the caller's stop ends that


class _Ring:
    """`n` page-locked (cube, w0, shift) slots, or with `q_spec` = (npol, dtype)
    (q, scl, offs, w0, shift) slots of int16 samples in that byte order.
    delays: each slot ends in an (nsub, nchan) f64 buffer for the archive's
    fractional delays."""

    def __init__(self, n, nsub, nchan, nbin, q_spec=None, delays=False):
        if q_spec is None:
            spec = [((nsub, nchan, nbin), np.float32)]
        else:
            npol, dtype = q_spec
            spec = [((nsub, npol, nchan, nbin), dtype), ((nsub, npol, nchan), np.float32),
                    ((nsub, npol, nchan), np.float32)]
        spec += [((nsub, nchan), np.float32), ((nchan,), np.int32)]
        if delays:
            spec += [((nsub, nchan), np.float64)]
        self.slots = [tuple(_native.PinnedArray(shape, dt) for shape, dt in spec) for _ in range(n)]

    def arrays(self, i):
        return tuple(p.array for p in self.slots[i])

    def close(self):
        for slot in self.slots:
            for p in slot:
                p.close()


class _ResultRing:
    """`n` page-locked (q, scl, offs) slots for one lane's residual downloads:
    int16 samples (nsub, nchan, nbin) of `dtype` ('>i2' or native), f32 scales
    and offsets (nsub, nchan)."""

    def __init__(self, n, nsub, nchan, nbin, dtype):
        spec = [((nsub, nchan, nbin), dtype), ((nsub, nchan), np.float32), ((nsub, nchan), np.float32)]
        self.slots = [tuple(_native.PinnedArray(shape, dt) for shape, dt in spec) for _ in range(n)]

    def triples(self):
        return [tuple(p.array for p in slot) for slot in self.slots]

    def close(self):
        for slot in self.slots:
            for p in slot:
                p.close()


def clean_batch(loader, shape, device=0, ring=None, max_iter=5, chanthresh=5.0, subintthresh=5.0,
                pulse_region=(0, 0, 1), baseline_duty=0.15, lanes=1, join_timeout=None, quantised=False, nsum=1,
                dedisp="shift", input_dedispersed=False, fit_mode=_native.FIT_EXACT, options=None,
                any_length=None, residuals=False, residual_big_endian=True, detrend=None,
                detrend_pieces=None, std_template=None, hotbins=None, dynspec=None):
    """Clean the archives produced by `loader` (an iterable of (cube, w0, shift)
    host arrays of one (nsub, nchan, nbin) shape; shift is reduced mod nbin).
    A loader thread copies them into a ring of page-locked slots; the GPU
    pipeline overlaps each upload with the previous cleaning, on `lanes`
    concurrent sessions.  Yields one ic_run dict per archive, in order.

    quantised=True: the loader yields (q, scl, offs, w0, shift) instead, the
    int16 samples (nsub, npol, nchan, nbin) of a fold-mode PSRFITS archive with
    their scales and offsets (nsub, npol, nchan) (psrfits.load_quantised); the
    cleaned cube is polarisation 0 (nsum 1) or pol 0 + pol 1 (nsum 2) of their
    decode, made on the GPU.  The ring then holds the first `nsum`
    polarisations as page-locked int16 in the byte order of the loader's first
    item ('>i2' as stored, or native): half the bytes of an f32 cube cross the
    bus, and none of the polarisations the loop never reads.

    dedisp="fft": the archives are dedispersed by the FFT phase rotation
    (IC_DEDISP_FFT), each by its own fractional delays: every loader item ends
    in them, (cube, w0, shift, delay) or (q, scl, offs, w0, shift, delay), f64
    in bins, (nchan,) per channel or (nsub, nchan) per profile (both kinds may
    alternate; psrfits_loader yields such items).  The delays are staged in the
    ring and go up with their archive.  An item without delays raises
    ValueError, as does one with delays when dedisp is "shift".
    input_dedispersed, fit_mode, options (a dict of schedule options) and
    any_length (None = the IC_ANY_NBIN switch: IC_DEDISP_FFT_ANY, any nbin in
    16..4096) are handed to every lane's GpuSession.

    residuals=True: every dict of an archive that was cleaned (n_iter > 0) comes
    with out["residual_q"] = (q, scl, offs), its pulse-free residual as a
    fold-mode PSRFITS file stores it (GpuSession.residual_quantised: int16
    (nsub, nchan, nbin), '>i2' unless residual_big_endian is False, and f32
    (nsub, nchan) scales and offsets), encoded on the GPU and downloaded while
    the lane cleans its next archive.  The three arrays are views into a
    page-locked result ring of the batch (2 slots with one lane, else 3 per
    lane), not copies: they expire when the generator is advanced to the next
    result, or closed - write or copy them before that;
    psrfits.save_quantised(path, *out["residual_q"], ...) writes them as they
    are.  Stopping early and a leaked lane follow the input ring's rules: the
    result ring of a batch with a leaked lane is never freed.

    detrend = (chan_order, subint_order[, rounds, clip]): the opt-in detrended
    scaling (detrend.py) on every lane's session; None reads the IC_DETREND
    switch (unset, empty or 0: off).  detrend_pieces = (chan, subint): piecewise
    detrending (cleaner.run_loop's); None reads the IC_DETREND_PIECES switch.
    std_template (cleaner.run_loop's: a profile (nbin,), a path, or a pair with
    the align mode): every archive is cleaned against this standard profile
    (std_template.py), set once on every lane's session and aligned against
    each archive; out["std_alignment"] is per archive, and a failed alignment
    warns on stderr.  None reads the IC_STD_TEMPLATE switch.
    hotbins = (threshold, on_start, on_end[, rounds]): the opt-in hot-bin
    repair (hotbins.py) on every lane's session: each archive's off-pulse hot
    bins are repaired before it is cleaned, and out["hotbins"] = dict(count,
    total, offsets, bins) is per archive.  None reads the IC_HOTBINS switch
    ("thr,start,end[,rounds]"; unset, empty or 0: off).
    dynspec=True: out["dynspec"] = dict(amp, err, base) per archive, its dynamic
    spectrum (dynspec.py).  None reads the IC_DYNSPEC switch (unset, empty or
    0: off; no file is written here)."""
    from . import dynspec as dsm
    from . import hotbins as hbm
    dyn = dsm.normalise(dynspec) is not None
    from . import std_template as stdt
    hot = hbm.normalise(hotbins)
    from .detrend import normalise, normalise_pieces
    detrend = normalise(detrend)
    detrend_pieces = normalise_pieces(detrend_pieces, int(shape[0]), int(shape[1]), detrend)
    if dedisp not in ("shift", "fft"):
        raise ValueError("dedisp must be 'shift' or 'fft', not %r" % (dedisp,))
    fft = dedisp == "fft"
    nsum = int(nsum)
    if quantised and nsum not in (1, 2):
        raise ValueError("nsum must be 1 or 2")
    nsub, nchan, nbin = (int(x) for x in shape)
    std = stdt.normalise(std_template, nbin)
    lanes = int(lanes)
    if lanes < 1:
        raise ValueError("lanes must be >= 1")
    if ring is None:
        ring = 3 * lanes + 1
    if ring < 3 * lanes:
        raise ValueError("ring must hold >= 3 slots per lane (loading, copying, cleaning)")
    free = queue.Queue()
    full = queue.Queue(maxsize=ring)
    stop = threading.Event()
    error = []
    rings = [] if quantised else [_Ring(ring, nsub, nchan, nbin, delays=fft)]   # quantised: made for the first item's byte order
    for i in range(ring):
        free.put(i)

    def stage_quantised(i, q, scl, offs):
        q = np.asarray(q)
        if q.ndim == 3:
            q = q.reshape(nsub, 1, nchan, nbin)
        if q.dtype.kind != "i" or q.dtype.itemsize != 2:
            raise ValueError("quantised samples must be int16 (native or '>i2'), got %s" % q.dtype)
        if q.ndim != 4 or q.shape[0] != nsub or q.shape[2:] != (nchan, nbin) or q.shape[1] < nsum:
            raise ValueError("quantised samples %s != (%d, npol >= %d, %d, %d)" % (q.shape, nsub, nsum, nchan, nbin))
        if not rings:
            rings.append(_Ring(ring, nsub, nchan, nbin, (nsum, q.dtype), delays=fft))
        dq, dscl, doffs = rings[0].arrays(i)[:3]
        np.copyto(dq, q[:, :nsum])   # (a later item in the other byte order is converted to the ring's)
        npol = q.shape[1]
        np.copyto(dscl, np.asarray(scl, np.float32).reshape(nsub, npol, nchan)[:, :nsum])
        np.copyto(doffs, np.asarray(offs, np.float32).reshape(nsub, npol, nchan)[:, :nsum])

    def split_delay(item):
        """(the item without its delays, the delays or None)"""
        item = tuple(item)
        base = 5 if quantised else 3
        if len(item) not in (base, base + 1):
            raise ValueError("a loader item holds %d arrays, or %d with its delays, not %d"
                             % (base, base + 1, len(item)))
        delay = item[base] if len(item) > base else None
        if fft and delay is None:
            raise ValueError("dedisp='fft': every loader item ends in its archive's fractional delays")
        if not fft and delay is not None:
            raise ValueError("a loader item with delays needs dedisp='fft'")
        return item[:base], delay

    views = {}   # ring slot -> the delays of the archive staged in it, as handed to the session

    def stage_delay(i, delay):
        d = np.asarray(delay, np.float64)
        buf = rings[0].arrays(i)[-1]
        if d.shape == (nchan,):
            np.copyto(buf[0], d)        # per channel: row 0
            views[i] = buf[0]
        elif d.shape == (nsub, nchan):
            np.copyto(buf, d)
            views[i] = buf
        else:
            raise ValueError("delays %s != (%d,) or (%d, %d)" % (d.shape, nchan, nsub, nchan))

    def load():
        try:
            for item in loader:
                i = free.get()
                if stop.is_set():
                    return
                item, delay = split_delay(item)
                if quantised:
                    q, scl, offs, w0, shift = item
                    stage_quantised(i, q, scl, offs)
                else:
                    cube, w0, shift = item
                    np.copyto(rings[0].arrays(i)[0], np.asarray(cube, np.float32).reshape(nsub, nchan, nbin))
                if fft:
                    stage_delay(i, delay)
                w, s = rings[0].arrays(i)[-3:-1] if fft else rings[0].arrays(i)[-2:]
                np.copyto(w, np.asarray(w0, np.float32).reshape(nsub, nchan))
                np.copyto(s, np.mod(np.asarray(shift), nbin).astype(np.int32).reshape(nchan))
                full.put(i)
        except Exception as e:  # noqa: BLE001 - re-raised in the consumer
            error.append(e)
        finally:
            full.put(None)

    th = threading.Thread(target=load, daemon=True)
    th.start()

    def staged():
        while True:
            i = full.get()
            if i is None:
                return
            order.append(i)
            arrays = rings[0].arrays(i)
            yield arrays[:-1] + (views[i],) if fft else arrays

    order = []
    sessions = []
    result_rings = []
    lanes_gen = None
    try:
        if residuals:
            for _ in range(lanes):
                result_rings.append(_ResultRing(2 if lanes == 1 else 3, nsub, nchan, nbin,
                                                ">i2" if residual_big_endian else np.int16))
        for _ in range(lanes):
            sessions.append(_native.GpuSession(nsub, nchan, nbin, max_iter, chanthresh, subintthresh,
                                               pulse_region, baseline_duty, device=device, fit_mode=fit_mode,
                                               options=options, input_dedispersed=input_dedispersed,
                                               dedisp_fft=fft, any_length=any_length, detrend=detrend,
                                               detrend_pieces=detrend_pieces, std_template=std, hotbins=hot))
        lanes_gen = run_lanes(sessions, staged(), stop=stop, join_timeout=join_timeout, nsum=nsum,
                              residuals=[rr.triples() for rr in result_rings] if residuals else None, dynspec=dyn)
        for k, out in enumerate(lanes_gen):
            free.put(order[k])          # archive k's slot is free once its result is yielded
            if std is not None:
                stdt.warn_failed(out.get("std_alignment"), std[1], "archive %d of the batch" % k)
            yield out
        if error:
            raise error[0]
    finally:
        stop.set()                      # loader and lanes stop taking archives
        for _ in range(ring):
            free.put(0)                 # a loader waiting for a slot wakes up and returns
        if lanes_gen is not None:
            lanes_gen.close()           # returns once no worker thread is inside ic_run
        th.join(timeout=60)
        for sess in sessions:
            sess.close()
        if any(getattr(sess, "_ic_leaked", False) for sess in sessions):
            _LEAKED.extend(rings)       # a leaked lane's copies may still read the page-locked ring
            _LEAKED.extend(result_rings)   # ... and its downloads still write the result ring
        else:
            # (sess.close() above has drained every lane's download stream)
            for rg in rings + result_rings:
                rg.close()


def psrfits_loader(paths, dedisp="shift", any_length=None):
    """Loader for clean_batch(..., quantised=True, dedisp=dedisp) over fold-mode
    PSRFITS files (psrfits.load_quantised): yields (q, scl, offs, w0, shift),
    or with dedisp="fft" (q, scl, offs, w0, shift, delay), the delays the file's
    DM, channel frequencies and folding periods give (per channel, or per
    profile when the rows' periods differ).  Raises ValueError naming the file
    whose dedispersion is not `dedisp`: one with integral delays in an "fft"
    list, one with fractional delays in a "shift" list.  The delays are never
    rounded, and integral ones never take the rotation, which is not exact.
    any_length: psrfits.load_quantised's (dedispersion.plan's opt-in)."""
    if dedisp not in ("shift", "fft"):
        raise ValueError("dedisp must be 'shift' or 'fft', not %r" % (dedisp,))
    from . import psrfits
    for path in paths:
        q, scl, offs, w0, shift, meta = psrfits.load_quantised(path, any_length=any_length)
        delay = meta["delay"]
        if (delay is not None) != (dedisp == "fft"):
            raise ValueError("%s: the archive is dedispersed by %s, the batch by %s"
                             % (path, "fractional delays (FFT rotation)" if delay is not None
                                else "integer shifts", "the FFT rotation (dedisp='fft')" if dedisp == "fft"
                                else "integer shifts (dedisp='shift')"))
        if delay is None:
            yield q, scl, offs, w0, shift
        else:
            yield q, scl, offs, w0, shift, np.ascontiguousarray(delay, dtype=np.float64)
