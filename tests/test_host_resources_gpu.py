"""GPU tests of the host layer's resource handling (ic_session.hip): sessions
that are created, fed through every upload path, read back and destroyed over
and over neither lose device memory nor change their results, and every
one-shot entry point and every upload that rejects its arguments leaves the
library and the session as they were."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHURN_SHAPE = (16, 64, 4096)   # f32 cube: 16 MiB
CUBE_BYTES = 4 * CHURN_SHAPE[0] * CHURN_SHAPE[1] * CHURN_SHAPE[2]
CYCLES = 12
SMALL = (2, 8, 64)


def _bits(a):
    """The array's bytes as unsigned integers: equal NaNs compare equal."""
    a = np.ascontiguousarray(a)
    return a.view("u%d" % a.dtype.itemsize)


def _same_run(a, b):
    return (np.array_equal(_bits(a["weights"]), _bits(b["weights"]))
            and np.array_equal(_bits(a["test"]), _bits(b["test"])))


def _free_bytes():
    import torch
    return int(torch.cuda.mem_get_info(0)[0])


@pytest.fixture(scope="module")
def churn_inputs():
    from iterative_cleaner_amd import psrfits, synth
    nsub, nchan, nbin = CHURN_SHAPE
    data, w0, shift = synth.make_cube(nsub, nchan, nbin, 41, 0.1, npol=2)
    rng = np.random.default_rng(42)
    data[:, 1] += (0.37 * rng.standard_normal(data[:, 1].shape, dtype=np.float32))
    q, scl, offs = psrfits.quantise(data)
    cube = np.ascontiguousarray((data[:, 0] + data[:, 1]).astype(np.float32))
    return dict(q=np.ascontiguousarray(q), scl=np.ascontiguousarray(scl, dtype=np.float32),
                offs=np.ascontiguousarray(offs, dtype=np.float32), cube=cube,
                w0=np.ascontiguousarray(w0, dtype=np.float32),
                shift=np.ascontiguousarray(np.mod(shift, nbin), dtype=np.int32),
                dchan=np.ascontiguousarray(synth.fractional_delays(shift, nbin)),
                dprof=np.ascontiguousarray(synth.per_profile_delays(shift, nbin, nsub)))


def _session(x):
    from iterative_cleaner_amd import _native
    nsub, nchan, nbin = CHURN_SHAPE
    return _native.GpuSession(nsub, nchan, nbin, max_iter=1, delay=x["dchan"])


def _cycle(x):
    """One session's life; the result of its last run."""
    with _session(x) as s:
        s.upload_quantised(x["q"], x["scl"], x["offs"], x["w0"], x["shift"], 1)
        s.run()
        s.upload_quantised(x["q"], x["scl"], x["offs"], x["w0"], x["shift"], 2)   # the staging regrows
        s.run()
        s.upload_quantised_async(x["q"], x["scl"], x["offs"], x["w0"], x["shift"], 2, delay=x["dchan"])
        s.upload_async(x["cube"], x["w0"], x["shift"], delay=x["dprof"])   # second slot, both slots' delays
        s.run()
        s.run()
        s.residual()
        s.residual_quantised()
        s.set_option("rot_stats", 0)   # the residual rows measured in a pass of their own: R
        return s.run()


@pytest.fixture(scope="module")
def churn(churn_inputs):
    """CYCLES session lives: the results of the first and the last, and the
    device's free memory after the second and after the last."""
    first = last = None
    free = {}
    _free_bytes()   # the reading's own one-time cost comes before the first reading that counts
    for c in range(1, CYCLES + 1):
        last = _cycle(churn_inputs)
        if c == 1:
            first = last
        if c in (2, CYCLES):
            free[c] = _free_bytes()
    return dict(first=first, last=last, free=free)


def test_lifecycle_churn_keeps_device_memory(churn):
    """Ten session lives (cycles 3 to 12) that allocate every lazily allocated
    buffer must not cost the device more than 5 cubes of free memory: half of
    what losing one cube-sized buffer (slot_raw, slot_q, res_q, R, dr, Tc, D) per
    life would cost.  A derived bound; it does not see a lost small buffer
    (weights, delays, phasor tables), and other users of the device add noise."""
    drop = churn["free"][2] - churn["free"][CYCLES]
    print("free after cycle 2: %d, after cycle %d: %d, drop %d bytes (bound %d)"
          % (churn["free"][2], CYCLES, churn["free"][CYCLES], drop, 5 * CUBE_BYTES))
    assert drop <= 5 * CUBE_BYTES


def test_churn_leaves_results_unchanged(churn, churn_inputs):
    """The last run of the first and of the last life give the same bits, which
    are those of a fresh session given that archive alone."""
    from iterative_cleaner_amd import _native
    assert _same_run(churn["first"], churn["last"])
    x = churn_inputs
    nsub, nchan, nbin = CHURN_SHAPE
    with _native.GpuSession(nsub, nchan, nbin, max_iter=1, delay=x["dprof"]) as s:
        s.upload(x["cube"], x["w0"], x["shift"])
        fresh = s.run()
    assert fresh["n_iter"] == churn["last"]["n_iter"] == 1
    assert _same_run(fresh, churn["last"])


# ------------------------------------------------------------- one-shots

def _small_inputs():
    from iterative_cleaner_amd import psrfits, synth
    nsub, nchan, nbin = SMALL
    data, w0, shift = synth.make_cube(nsub, nchan, nbin, 5, 0.2, npol=2)
    q, scl, offs = psrfits.quantise(data)
    return dict(data=data, cube=np.ascontiguousarray(data[:, 0]), w0=w0, shift=shift,
                q=np.ascontiguousarray(q), scl=np.ascontiguousarray(scl, dtype=np.float32),
                offs=np.ascontiguousarray(offs, dtype=np.float32),
                delay=synth.fractional_delays(shift, nbin))


def _raises(match, fn, *a, **kw):
    from iterative_cleaner_amd import _native
    with pytest.raises(_native.NativeError, match=match) as e:
        fn(*a, **kw)
    assert "rc=-1" in str(e.value)


def _rotate(x):
    from iterative_cleaner_amd import _native
    good = lambda: (_native.rotate_profiles(x["cube"], x["delay"]),)

    def bad():
        d = x["delay"].copy()
        d[3] = np.nan
        _raises("not finite", _native.rotate_profiles, x["cube"], d)
        _raises("power-of-two", _native.rotate_profiles, np.zeros((2, 8, 48), np.float32), x["delay"])
        _raises("out of range", _native.rotate_profiles, x["cube"], x["delay"], device=10 ** 6)
    return good, bad


def _encode(x):
    from iterative_cleaner_amd import _native
    lib = _native.load_library()
    nsub, nchan, nbin = SMALL
    good = lambda: _native.encode_profiles(x["cube"])

    def bad():
        q = np.empty(SMALL, np.int16)
        so = np.empty((2, nsub, nchan), np.float32)
        rc = lib.ic_encode_profiles(0, nsub, nchan, nbin, _native._ptr(x["cube"]), 2, _native._ptr(q),
                                    _native._ptr(so[0]), _native._ptr(so[1]))
        assert rc == -1 and "flag" in _native._err(lib)
        _raises("out of range", _native.encode_profiles, x["cube"], device=10 ** 6)
    return good, bad


def _decode(x):
    from iterative_cleaner_amd import _native
    lib = _native.load_library()
    nsub, nchan, nbin = SMALL
    good = lambda: (_native.decode_profiles(x["q"], x["scl"], x["offs"], 2),)

    def bad():
        out = np.empty(SMALL, np.float32)
        rc = lib.ic_decode_profiles(0, nsub, 2, 2, nchan, nbin, _native._ptr(x["q"]), _native._ptr(x["scl"]),
                                    _native._ptr(x["offs"]), 2, _native._ptr(out))
        assert rc == -1 and "flag" in _native._err(lib)
        _raises("nsum=2 > npol=1", _native.decode_profiles, x["q"][:, :1], x["scl"][:, :1], x["offs"][:, :1], 2)
        _raises("out of range", _native.decode_profiles, x["q"], x["scl"], x["offs"], 2, device=10 ** 6)
    return good, bad


def _stats(x):
    from iterative_cleaner_amd import _native

    def good():
        test, diag = _native.comprehensive_stats(x["cube"], x["w0"], diagnostics=True)
        return (test,) + diag

    def bad():
        _raises("rowstat_waves", _native.comprehensive_stats, x["cube"], x["w0"], rowstat_waves=3)
        _raises("out of range", _native.comprehensive_stats, x["cube"], x["w0"], device=10 ** 6)
    return good, bad


def _fit(x):
    from iterative_cleaner_amd import _native
    profiles = x["cube"].reshape(-1, SMALL[2])
    T = profiles.mean(axis=0)
    good = lambda: _native.fit_profiles(profiles, T)

    def bad():
        _raises("rc=-1", _native.fit_profiles, profiles[:0], T)
        _raises("out of range", _native.fit_profiles, profiles, T, device=10 ** 6)
    return good, bad


@pytest.mark.parametrize("oneshot", [_rotate, _encode, _decode, _stats, _fit], ids=lambda f: f.__name__.strip("_"))
def test_oneshot_error_then_success(oneshot):
    """Each one-shot entry point refuses bad arguments (IC_EINVAL) and then gives
    the bits it gave before."""
    good, bad = oneshot(_small_inputs())
    before = good()
    bad()
    after = good()
    assert len(before) == len(after)
    for a, b in zip(before, after):
        assert a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


# --------------------------------------------------------------- uploads

def test_upload_argument_errors_leave_the_session_usable():
    """A shift outside [0, nbin) is refused by every upload that takes host
    pointers (called on the C-ABI: the Python wrappers reduce shifts modulo
    nbin) and the session then cleans as a fresh one; the asynchronous queue
    holds two uploads, and a synchronous upload waits for it to drain."""
    from iterative_cleaner_amd import _native
    lib = _native.load_library()
    p = _native._ptr
    x = _small_inputs()
    nsub, nchan, nbin = SMALL
    cube, w0 = x["cube"], np.ascontiguousarray(x["w0"], dtype=np.float32)
    shift = np.ascontiguousarray(np.mod(x["shift"], nbin), dtype=np.int32)
    bad = shift.copy()
    bad[nchan - 1] = nbin
    q1 = np.ascontiguousarray(x["q"][:, :1])
    s1, o1 = np.ascontiguousarray(x["scl"][:, :1]), np.ascontiguousarray(x["offs"][:, :1])

    def uploads(s, sh):
        return [("ic_upload", lambda: lib.ic_upload(s.h, p(cube), p(w0), p(sh))),
                ("ic_upload_pols", lambda: lib.ic_upload_pols(s.h, p(x["data"]), 2, p(w0), p(sh))),
                ("ic_upload_async", lambda: lib.ic_upload_async(s.h, p(cube), p(w0), p(sh))),
                ("ic_upload_quantised",
                 lambda: lib.ic_upload_quantised(s.h, p(q1), p(s1), p(o1), 1, 1, 0, p(w0), p(sh))),
                ("ic_upload_quantised_async",
                 lambda: lib.ic_upload_quantised_async(s.h, p(q1), p(s1), p(o1), 1, 1, 0, p(w0), p(sh)))]

    with _native.GpuSession(nsub, nchan, nbin) as fresh:
        fresh.upload(cube, w0, shift)
        want = fresh.run()
    with _native.GpuSession(nsub, nchan, nbin) as s:
        for name, call in uploads(s, bad):
            assert call() == -1, name
            assert re.search(r"out of \[0,nbin\)", _native._err(lib)), name
        s.upload(cube, w0, shift)
        got = s.run()
        assert got["loops"] == want["loops"] and _same_run(got, want)
        s.upload_async(cube, w0, shift)
        s.upload_async(cube, w0, shift)
        assert lib.ic_upload_async(s.h, p(cube), p(w0), p(shift)) == -4
        assert "pending" in _native._err(lib)
        s.run()   # one upload still queued
        for name, call in uploads(s, shift):
            if not name.endswith("async"):
                assert call() == -4, name
                assert "pending" in _native._err(lib), name
        again = s.run()
        assert _same_run(again, want)
