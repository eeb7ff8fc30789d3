"""GPU tests of the fused residual encode (k_residual_q) and the asynchronous
residual download (ic_get_residual_quantised_async, ic_residual_wait).

The reference of every comparison is host code that predates both:
psrfits.quantise(session.residual()[:, None]), the host's arithmetic on the
f32 residual that the parity tests hold to the oracle.  Bits are compared, not
values (a NaN equals any NaN)."""
import numpy as np
import pytest

from helpers import bits_equal
from test_encode_gpu import _case, _same

pytestmark = pytest.mark.gpu


def _host(s):
    """The host's encode of the session's f32 residual: (q, scl, offs)."""
    from iterative_cleaner_amd import psrfits
    with np.errstate(all="ignore"):
        q, scl, offs = psrfits.quantise(s.residual()[:, None])
    return np.ascontiguousarray(q[:, 0]), scl[:, 0], offs[:, 0]


class _Slots:
    """`n` page-locked (q, scl, offs) triples of one shape and byte order."""

    def __init__(self, shape, n=1, big_endian=False):
        from iterative_cleaner_amd import _native
        nsub, nchan, _ = shape
        self.pinned = [(_native.PinnedArray(shape, ">i2" if big_endian else np.int16),
                        _native.PinnedArray((nsub, nchan)), _native.PinnedArray((nsub, nchan)))
                       for _ in range(n)]
        for trio in self.pinned:
            trio[0].array[:] = 12345        # nothing of an earlier download passes for this one
            trio[1].array[:] = -1.0
            trio[2].array[:] = -1.0

    def __getitem__(self, i):
        return tuple(p.array for p in self.pinned[i])

    def close(self):
        for trio in self.pinned:
            for p in trio:
                p.close()


def _async(s, slots, i=0):
    s.residual_quantised_async(*slots[i])
    s.residual_wait()
    return slots[i]


# the smallest shapes that reach each load / store path of k_residual_q and,
# with grid_cap 1 and 3, the multi-trip profile loop
FUSED = {
    "tiled": ((6, 40, 128), {}),                                       # tiled fit cube, 16-byte stores
    "row-major": ((6, 40, 128), {"options": {"fit_tiled": 0}}),
    "closed": ((6, 40, 128), {"fit_mode": 1}),                        # the raw - base branch
    "pulse-region": ((6, 40, 128), {"pulse_region": (0.5, 20, 60)}),
    "nbin-100": ((5, 33, 100), {}),                                    # nbin % 8 != 0
    "nbin-50": ((5, 33, 50), {}),                                      # nbin % 4 != 0: no 16-byte loads
    "nbin-125": ((4, 9, 125), {}),                                     # odd rows on 2-byte boundaries
    "nbin-125-closed": ((4, 9, 125), {"fit_mode": 1}),
    "nbin-8192": ((2, 3, 8192), {}),                                   # the largest row held on chip
}


@pytest.mark.parametrize("name", list(FUSED))
def test_fused_kernel_equals_host_quantise(name):
    """Integer shifts (c mod 7: rows wrap), RFI fraction 0.2, at grid_cap 0, 1
    and 3: residual_quantised() and the asynchronous call into page-locked
    arrays, both byte orders, against the host's encode of the f32 residual
    (computed once, at grid_cap 0: the cap changes no residual)."""
    from iterative_cleaner_amd import _native, synth
    shape, kw = FUSED[name]
    kw = dict(kw)
    opts = dict(kw.pop("options", {}))
    data, w0, shift = synth.make_cube(*shape, 70 + shape[2], 0.2)
    assert np.array_equal(shift, np.arange(shape[1]) % 7)
    raw = np.ascontiguousarray(data[:, 0])
    native, big = _Slots(shape), _Slots(shape, big_endian=True)
    want = None
    try:
        for cap in (0, 1, 3):
            o = dict(opts, grid_cap=cap) if cap else opts
            with _native.GpuSession(*shape, device=0, options=o or None, **kw) as s:
                s.upload(raw, w0, shift)
                assert s.run()["n_iter"] >= 1
                if want is None:
                    want = _host(s)
                    assert np.count_nonzero(want[0]) > want[0].size // 2
                _same(s.residual_quantised(), want)
                _same(s.residual_quantised(big_endian=True), want, True)
                _same(_async(s, native), want)
                _same(_async(s, big), want, True)
    finally:
        native.close()
        big.close()


def _edge_cube(nonfinite):
    from iterative_cleaner_amd import synth
    shape = (6, 40, 128)
    data, w0, shift = synth.make_cube(*shape, 91, 0.2)
    raw = np.ascontiguousarray(data[:, 0])
    w0 = w0.copy()
    phase = (np.arange(128) + 0.5) / 128
    pulse = np.exp(-0.5 * ((phase - 0.3) / 0.02) ** 2).astype(np.float32)
    raw[1, 3] = 3.0 * np.roll(pulse, int(shift[3]))      # the template's shape times a scalar, no noise
    raw[2, 5] = 0.0                                       # all zero
    w0[:, 8] = 1.0
    w0[3, 8] = 0.0                                        # a zero-weight profile among live ones
    if nonfinite:
        raw[4, 10, 17] = np.nan
        raw[0, 12, 99] = np.inf
    return shape, raw, w0, shift


@pytest.mark.parametrize("fit_mode", [0, 1], ids=["exact", "closed"])
@pytest.mark.parametrize("nonfinite", [False, True], ids=["finite", "nan-inf"])
def test_edge_rows(nonfinite, fit_mode):
    """A profile that is the pulse times a scalar, an all-zero profile (its row
    is zero: scl 1, offs 0), a zero-weight profile, and - in the second cube -
    one NaN and one +Inf sample: the NaN flag and the scl fallback survive the
    fusion, the bits are the host's.

    The all-zero profile is fitted with amplitude 0 and status 4, so its
    residual 0 * T - 0 is a row of zeros of both signs.  There the host's offs
    is 0 with a sign that numpy's min / max leave to their vector reduction
    order (np.float32 zeros with a single -0.0: min() gives +0.0), so the
    reference defines the zero, not its sign; the device gives such a row the
    sign of its sample 0, as the two-kernel encode before the fusion did, and
    that is what the row is held to.  Every other row: the host's bits."""
    from iterative_cleaner_amd import _native
    shape, raw, w0, shift = _edge_cube(nonfinite)
    slots = _Slots(shape, big_endian=True)
    try:
        with _native.GpuSession(*shape, device=0, fit_mode=fit_mode) as s:
            s.upload(raw, w0, shift)
            assert s.run()["n_iter"] >= 1
            want = _host(s)
            res = s.residual()
            zero = ~res.any(axis=-1) & ~np.isnan(res).any(axis=-1)      # rows of zeros
            assert np.all(want[1][zero] == 1.0) and np.all(want[2][zero] == 0.0) and not want[0][zero].any()
            want[2][zero] = res[zero, 0]                                # ... take sample 0's sign
            got = s.residual_quantised()
            _same(got, want)
            _same(_async(s, slots), want, True)
            if nonfinite:
                # the input does reach the NaN flag or the scl fallback (the closed
                # form's status turns the rows of a non-finite template to zero)
                assert np.isnan(want[2]).any() or np.any(want[1] == 1.0)
                assert np.all(got[1][np.isnan(got[2])] == 1.0)
            else:
                assert np.isfinite(got[1]).all() and np.isfinite(got[2]).all()
                assert zero[2, 5] and got[1][2, 5] == 1.0 and got[2][2, 5] == 0.0 and not got[0][2, 5].any()
    finally:
        slots.close()


@pytest.mark.parametrize("name", ["fft-channel", "fft-profile"])
def test_fft_mode_keeps_its_bits(name):
    """FFT dedispersion keeps its two steps (rotation, k_encode_q) through a
    session-owned f32 cube: async == sync == the host's encode, twice (the
    staging is reused), and a further run still cleans as before."""
    from iterative_cleaner_amd import _native, synth
    shape, kw = _case(name)
    data, w0, shift = synth.make_cube(*shape, 70 + shape[2], 0.2)
    raw = np.ascontiguousarray(data[:, 0])
    slots = _Slots(shape, 2)
    try:
        with _native.GpuSession(*shape, device=0, **kw) as s:
            s.upload(raw, w0, shift)
            first = s.run()
            want = _host(s)
            for i in range(2):
                _same(s.residual_quantised(), want)
                _same(_async(s, slots, i), want)
            again = s.run()                         # the f32 staging is the run's scratch again
            assert bits_equal(again["weights"], first["weights"]) and bits_equal(again["test"], first["test"])
            _same(_async(s, slots, 0), want)
    finally:
        slots.close()


def test_the_upload_into_the_slot_the_encode_reads_waits_for_it():
    """Closed form: the residual reads the raw cube of the input slot the run
    used.  upload_async(a2) right after residual_quantised_async targets that
    slot (a0's): a0's residual must come out whole, then a1's."""
    from iterative_cleaner_amd import _native, synth
    shape = (6, 40, 128)
    arcs, pinned = [], []
    for k in range(3):
        data, w0, shift = synth.make_cube(*shape, 400 + k, 0.1 + 0.1 * k)
        arcs.append((np.ascontiguousarray(data[:, 0]), w0, shift.astype(np.int32)))
        trio = (_native.PinnedArray(shape), _native.PinnedArray(w0.shape), _native.PinnedArray(shift.shape, np.int32))
        for p, a in zip(trio, arcs[-1]):
            p.array[:] = a
        pinned.append(trio)
    items = [tuple(p.array for p in trio) for trio in pinned]
    want = []
    for cube, w0, shift in arcs[:2]:
        with _native.GpuSession(*shape, device=0, fit_mode=_native.FIT_CLOSED) as s:
            s.upload(cube, w0, shift)
            s.run()
            want.append(_host(s))
    assert not bits_equal(want[0][0], want[1][0])
    slots = _Slots(shape, 2)
    try:
        with _native.GpuSession(*shape, device=0, fit_mode=_native.FIT_CLOSED) as s:
            s.upload_async(*items[0])
            s.upload_async(*items[1])
            s.run()
            s.residual_quantised_async(*slots[0])
            s.upload_async(*items[2])               # a0's input slot
            s.run()                                 # a1
            s.residual_wait()
            _same(slots[0], want[0])
            _same(_async(s, slots, 1), want[1])
    finally:
        slots.close()
        for trio in pinned:
            for p in trio:
                p.close()


def test_state_rules():
    from iterative_cleaner_amd import _native, batch, synth
    shape = (6, 40, 128)
    data, w0, shift = synth.make_cube(*shape, 70 + shape[2], 0.2)
    raw = np.ascontiguousarray(data[:, 0])
    slots = _Slots(shape, 2)
    try:
        with _native.GpuSession(*shape, device=0) as s:
            s.residual_wait()                                   # nothing pending: OK
            s.upload(raw, w0, shift)
            with pytest.raises(_native.NativeError, match=r"rc=-4"):
                s.residual_quantised_async(*slots[0])           # before any run
            s.run()
            want = _host(s)
            s.residual_quantised_async(*slots[0])               # two calls back to back, one wait
            s.residual_quantised_async(*slots[1])
            s.residual_wait()
            _same(slots[0], want)
            _same(slots[1], want)
            s.residual_wait()
            with pytest.raises(ValueError):
                s.residual_quantised_async(slots[0][0].astype(np.float32), *slots[0][1:])
            with pytest.raises(ValueError):
                s.residual_quantised_async(slots[0][0][:, :, :64], *slots[0][1:])
        s = _native.GpuSession(*shape, device=0)
        s.upload(raw, w0, shift)
        s.run()
        s.residual_quantised_async(*slots[0])
        s.close()                                               # a download in flight: drained, no error
        _same(slots[0], want)
        # a run without an iteration has no residual
        outs = list(batch.clean_batch(iter([(raw, w0, shift)] * 3), shape, device=0, max_iter=0, residuals=True))
        assert len(outs) == 3 and all(o["n_iter"] == 0 and "residual_q" not in o for o in outs)
    finally:
        slots.close()
