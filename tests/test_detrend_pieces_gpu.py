"""Piecewise detrending on the GPU (k_linetrend_pw, k_combine_pw;
ic_set_detrend_pieces, ic_get_trends_pieces,
ic_comprehensive_stats_detrend_pieces) against the written definition.

The yardstick is test_detrend_gpu.py's: the GPU's own std / mean / ptp / fftmax
of the run and valid = (w0 != 0) go through the piecewise statement
(iterative_cleaner_amd/detrend.py) and tests/detrend_pieces_ref.combine
(restated's scalers and NaN rule).  The test values, the weights and every
piece's coefficients must match BIT FOR BIT (a NaN matches a NaN); no tolerance.

The session cube (detrend_pieces_ref.teeth_cube): the 12 x 96 x 128 synthetic
cube under a sawtooth gain of period 16 channels (a parabola per subband, gain
1 at its edge channels and 3 in the middle), four profiles at subband-edge
channels carrying extra noise.  Checked on the CPU before the seeds were fixed:
the first iteration of the statement fed with the C oracle's diagnostics (exact
fit, integer shifts), for 5 noise levels x 16 seeds x 2 noise seeds.  A planted
profile at an edge channel is hard for every form: its channel (12 subints of
one gain) sees it with or without pieces, and a 16-channel parabola gives its
end points enough leverage to absorb part of an outlier there.  In most of the
160 cubes the three forms zap the same planted profiles, or the unpieced ones
more.  With seeds (22, 112) and 1.1 sigma of extra noise the statement zaps 4
of the 4 with orders (1, 2) and subint pieces w16, 2 of 4 with the unpieced
orders (1, 3) and 2 of 4 undetrended (112, 88 and 89 profiles in all), and no
test value of the three lies within 1.6e-2 of the threshold; these were fixed.
(At 1.3 sigma: 4 / 3 / 2; at 0.9: 1 / 0 / 0; at 1.0 a piecewise test value lies
3.6e-4 from the threshold.)

Every test here fails on a library without the ic_set_detrend_pieces symbol.
"""
import numpy as np
import pytest

import detrend_pieces_ref as ref
import detrend_ref
from helpers import bits_equal, bits_equal_nan
from iterative_cleaner_amd import detrend as dt

pytestmark = pytest.mark.gpu

SEED, SEED2, EXTRA = 22, 112, 1.1
SHAPE = (12, 96, 128)
ORDERS = (1, 2)
W16 = "w16"
IC_EINVAL, IC_ESTATE = -1, -4

_CUBES = {}


def _teeth(shape=SHAPE):
    if shape not in _CUBES:
        planted = ref.PLANTED if shape[:2] == (12, 96) else ((1, 48), (3, 63), (5, 80), (6, 95))
        _CUBES[shape] = ref.teeth_cube(*shape, SEED, SEED2, planted=planted, extra=EXTRA)
    return _CUBES[shape]


def _run(cube, shape, detrend="never", pieces="never", max_iter=1, delay=None, fit_mode=0, options=None,
         data_f64=False, timing=False):
    """One session run; "never": ic_set_detrend / ic_set_detrend_pieces is not called."""
    from iterative_cleaner_amd import _native
    raw, w0, shift = cube
    kw = {} if detrend == "never" else {"detrend": detrend}
    if pieces != "never":
        kw["detrend_pieces"] = pieces
    with _native.GpuSession(*shape, max_iter=max_iter, device=0, delay=delay, fit_mode=fit_mode, options=options,
                            data_f64=data_f64, **kw) as s:
        if timing:
            s.set_timing(True)
        s.upload(raw, w0, np.zeros_like(shift) if delay is not None else shift)
        out = s.run()
        out["diags"] = s.diagnostics()
        out["stats"] = s.run_stats()
        if timing:
            out["launches"] = {k: v["launches"] for k, v in s.kernel_times().items()}
        try:
            out["trends"] = s.trends()
        except _native.NativeError as e:
            out["trends_error"] = str(e)
    return out


def _starts(pieces, shape):
    return tuple(dt.resolve_pieces(p, n) for p, n in zip(pieces, shape[:2]))


def _check_yardstick(out, w0, detrend, pieces, shape, chanthresh=5.0, subintthresh=5.0):
    valid = np.asarray(w0) != 0
    cb, sb = _starts(pieces, shape)
    test, cc, sc = ref.combine(out["diags"], valid, chanthresh, subintthresh, detrend, cb, sb)
    assert bits_equal_nan(out["test"], test), "test values (%d differ)" % int(
        (~((out["test"] == test) | (np.isnan(out["test"]) & np.isnan(test)))).sum())
    with np.errstate(invalid="ignore"):
        want_w = np.where(test >= 1.0, np.float32(0.0), np.asarray(w0, np.float32)).astype(np.float32)
    assert bits_equal(out["weights"], want_w), "weights"
    gc, gs = out["trends"]
    assert gc.shape == cc.shape and gs.shape == sc.shape
    assert bits_equal_nan(gc, cc), "channel coefficients"
    assert bits_equal_nan(gs, sc), "subint coefficients"
    return test


# ------------------------------------------------------------------ one-shot

ONE_SHOT = (((3, 65), (None, [0, 1, 3, 64])),      # pieces of 1, 2, 61 and 1 entries: retired beside live ones
            ((65, 4), ([0, 64], None)),            # a 64-entry piece and a 1-entry piece
            ((130, 7), ([0, 1, 66], None)),        # a 64-entry piece off the 64-lane grid; chain wrap in the last
            ((8, 160), (None, "w16")),             # ten LOFAR-like pieces
            ((2, 600), (None, 512)))               # the cap: pieces of 1 and 2 entries (one wave per row)


@pytest.mark.parametrize("data_f64", (False, True), ids=("f32", "f64"))
@pytest.mark.parametrize("orders", ((1, 1), (2, 3), (3, 0), (0, 2)))
@pytest.mark.parametrize("shape,pieces", ONE_SHOT, ids=("3x65", "65x4", "130x7", "8x160", "2x600"))
def test_one_shot_matches_the_statement(shape, pieces, orders, data_f64):
    from iterative_cleaner_amd import _native
    nsub, nchan = shape
    data, w = detrend_ref.hard_cube(nsub, nchan, 64, 40 + nsub)
    test, (cc, sc), diags = _native.comprehensive_stats(data, w, 5.0, 4.0, diagnostics=True, detrend=orders,
                                                        data_f64=data_f64, detrend_pieces=pieces)
    assert diags[2].dtype == (np.float64 if data_f64 else np.float32)
    cb, sb = _starts(pieces, shape)
    want, wc, ws = ref.combine(diags, w != 0, 5.0, 4.0, orders, cb, sb)
    assert cc.shape == wc.shape and sc.shape == ws.shape
    assert bits_equal_nan(test, want)
    assert bits_equal_nan(cc, wc) and bits_equal_nan(sc, ws)
    if nchan >= 5 and nsub >= 3:
        assert np.isnan(want).any() and not np.isnan(want).all()
    if min(orders) == 0:                       # the direction that is off has no trend
        assert not (cc if orders[0] == 0 else sc).any()
    if shape == (3, 65) and orders[1]:         # 1-entry pieces are retired; the 61-entry one is fitted
        assert not sc[:, :, 0].any() and not sc[:, :, 3].any() and sc[0, :, 2].any()
    if shape == (130, 7) and orders[0]:
        assert not cc[:, :, 0].any() and cc[0, 0, 1].any() and cc[0, 0, 2].any()
    if shape == (8, 160) and orders[1]:
        assert all(sc[0, 1, q].any() for q in range(10))


def test_one_shot_refusals():
    from iterative_cleaner_amd import _native
    data, w = detrend_ref.hard_cube(3, 5, 64, 1)
    for bad in (([1, 2], None), (None, [0, 3, 2]), (None, [0, 2, 2]), ([0, 3], None), (None, [0, 5]),
                (list(range(513)), None), (None, list(range(513)))):
        with pytest.raises(_native.NativeError, match=r"rc=-1"):
            _native.comprehensive_stats(data, w, detrend=(1, 1), detrend_pieces=bad)
    lib = _native.load_library()                 # a NULL pointer with npieces > 0
    test = np.empty((3, 5))
    assert lib.ic_comprehensive_stats_detrend_pieces(0, 3, 5, 64, data.ctypes.data, w.ctypes.data, 5.0, 5.0,
                                                     test.ctypes.data, None, None, None, None, 0, 1, 1, 4, 5.0, None,
                                                     None, 2, None, 0, None) == IC_EINVAL


# ------------------------------------------------------------------ sessions: the teeth

def _planted_hits(test):
    with np.errstate(invalid="ignore"):
        return sum(bool(test[s, c] >= 1.0) for s, c in ref.PLANTED)


@pytest.mark.parametrize("max_iter", (1, 3))
def test_teeth_exact_fit_integer_shifts(max_iter):
    """Orders (1, 2) with a piece every 16 channels zap strictly more of the
    planted profiles than the undetrended loop and than the unpieced (1, 3)."""
    cube = _teeth()
    out = _run(cube, SHAPE, ORDERS, (None, W16), max_iter)
    _check_yardstick(out, cube[1], ORDERS, (None, W16), SHAPE)
    assert out["trends"][1].shape == (4, 12, 6, 4) and out["trends"][0].shape == (4, 96, 1, 4)
    assert out["stats"]["near_threshold"] == 0
    plain = _run(cube, SHAPE, "never", "never", max_iter)
    whole = _run(cube, SHAPE, (1, 3), "never", max_iter)
    hits = [_planted_hits(o["test"]) for o in (out, whole, plain)]
    print("planted zapped: %d in pieces, %d unpieced (1, 3), %d undetrended" % tuple(hits))
    assert hits[0] > hits[1] and hits[0] > hits[2]


# ------------------------------------------------------------------ sessions: other modes

def test_session_fractional_delays():
    from iterative_cleaner_amd import synth
    cube = _teeth()
    out = _run(cube, SHAPE, ORDERS, (None, W16), 2, delay=synth.fractional_delays(cube[2], SHAPE[2]))
    _check_yardstick(out, cube[1], ORDERS, (None, W16), SHAPE)


def test_session_closed_form_fit():
    from iterative_cleaner_amd import _native
    cube = _teeth()
    out = _run(cube, SHAPE, ORDERS, (None, W16), 2, fit_mode=_native.FIT_CLOSED)
    _check_yardstick(out, cube[1], ORDERS, (None, W16), SHAPE)


def test_session_f64_data_chan_pieces():
    cube = _teeth()
    out = _run(cube, SHAPE, (2, 3), ([0, 6], None), 2, data_f64=True)
    _check_yardstick(out, cube[1], (2, 3), ([0, 6], None), SHAPE)
    assert out["trends"][0].shape == (4, 96, 2, 4) and out["trends"][0][0, :, 1].any()


# ------------------------------------------------------------------ the two kernel pairs

_SLOPED = {}


def _sloped():
    if not _SLOPED:
        _SLOPED[0] = detrend_ref.sloped_cube(*SHAPE, 12, 112, extra=1.0)
    return _SLOPED[0]


def _launches(s):
    return {k: v["launches"] for k, v in s.kernel_times().items()}


def _rerun_launches(cube, detrend):
    """The launch counts of a session's second run (no upload in them), on a
    session that never set pieces."""
    from iterative_cleaner_amd import _native
    with _native.GpuSession(*SHAPE, max_iter=3, device=0, detrend=detrend) as s:
        s.set_timing(True)
        s.upload(*cube)
        s.run()
        before = _launches(s)
        s.run()
        after = _launches(s)
    return {k: after[k] - before[k] for k in after}


def test_one_piece_runs_the_piecewise_kernels_to_the_same_bits():
    """set_detrend_pieces([0], [0]) (k_linetrend_pw / k_combine_pw) against a
    session that never set pieces (k_linetrend / k_combine_dt), on the sloped
    cube of the whole-line tests; pieces taken back; detrending off."""
    from iterative_cleaner_amd import _native
    cube = _sloped()
    raw, w0, shift = cube
    never = _run(cube, SHAPE, ORDERS, "never", 3, timing=True)
    one = _run(cube, SHAPE, ORDERS, ([0], [0]), 3, timing=True)
    assert bits_equal_nan(one["test"], never["test"]) and bits_equal(one["weights"], never["weights"])
    assert one["trends"][0].shape == (4, 96, 1, 4) and never["trends"][0].shape == (4, 96, 4)
    assert bits_equal_nan(one["trends"][0][:, :, 0], never["trends"][0])
    assert bits_equal_nan(one["trends"][1][:, :, 0], never["trends"][1])
    assert never["trends"][0].any() and never["trends"][1].any()
    assert one["launches"] == never["launches"]            # both pairs are timed as k_linestats / k_combine
    plain = _run(cube, SHAPE, "never", "never", 3, timing=True)
    with _native.GpuSession(*SHAPE, max_iter=3, device=0) as s:
        s.set_timing(True)
        s.upload(raw, w0, shift)
        s.set_detrend_pieces([0], [0])                     # before ic_set_detrend: any order
        s.set_detrend(*ORDERS)
        a = s.run()
        assert bits_equal_nan(a["test"], never["test"])
        cc1, sc1 = s.trends()
        cc, sc = np.empty((4, 96, 4)), np.empty((4, 12, 4))    # one piece each: ic_get_trends answers too
        assert s.lib.ic_get_trends(s.h, cc.ctypes.data, sc.ctypes.data) == 0
        assert bits_equal_nan(cc, cc1[:, :, 0]) and bits_equal_nan(sc, sc1[:, :, 0])
        s.set_detrend_pieces(None, [0, 40])
        b = s.run()
        assert not bits_equal_nan(b["test"], never["test"])
        assert s.lib.ic_get_trends(s.h, cc.ctypes.data, sc.ctypes.data) == IC_ESTATE
        assert s.trends()[1].shape == (4, 12, 2, 4)
        # taken back: the whole-line kernels' bits and launch counts
        s.set_detrend_pieces(None, None)
        before = _launches(s)
        c = s.run()
        after = _launches(s)
        assert bits_equal_nan(c["test"], never["test"]) and bits_equal(c["weights"], never["weights"])
        assert {k: after[k] - before[k] for k in after} == _rerun_launches(cube, ORDERS)
        assert bits_equal_nan(s.trends()[0], never["trends"][0])
        assert s.lib.ic_get_trends_pieces(s.h, None, None) == IC_ESTATE
        # detrending off, pieces set: a session that never heard of either
        s.set_detrend(0, 0)
        s.set_detrend_pieces(3, "w16")
        before = after
        d = s.run()
        after = _launches(s)
        assert bits_equal_nan(d["test"], plain["test"]) and bits_equal(d["weights"], plain["weights"])
        assert {k: after[k] - before[k] for k in after} == _rerun_launches(cube, None)
        assert s.lib.ic_get_trends_pieces(s.h, None, None) == IC_ESTATE
        with pytest.raises(_native.NativeError, match="rc=%d" % IC_ESTATE):
            s.trends()
        for bad in (([1, 2], None), (None, [0, 3, 2]), ([0, 12], None), (None, [0, 96]), (None, list(range(513)))):
            with pytest.raises(_native.NativeError, match="rc=%d" % IC_EINVAL):
                s.set_detrend_pieces(*bad)
        assert s.lib.ic_set_detrend_pieces(s.h, 2, None, 0, None) == IC_EINVAL
    off = _run(cube, SHAPE, (0, 0), (3, W16), 3, timing=True)
    assert bits_equal_nan(off["test"], plain["test"]) and off["launches"] == plain["launches"]


# ------------------------------------------------------------------ schedules

SCHEDULES = ({}, {"grid_cap": 1}, {"rowstat_waves": 0}, {"rowstat_waves": 4, "rowstat_minlen": 64},
             {"rowstat_waves": 8, "rowstat_minlen": 64}, {"diag_fork": 0})


def test_schedules_give_the_same_bits():
    """8 x 160 x 64, subint pieces w16 and chan pieces [0, 3]: one wave per line
    and the multi-wave rows (k_linetrend_pw<1>, <4>, <8>)."""
    shape = (8, 160, 64)
    cube = _teeth(shape)
    pieces = ([0, 3], W16)
    first = None
    for opts in SCHEDULES:
        out = _run(cube, shape, ORDERS, pieces, 2, options=opts)
        if first is None:
            first = out
            _check_yardstick(out, cube[1], ORDERS, pieces, shape)
            assert out["trends"][0].shape == (4, 160, 2, 4) and out["trends"][1].shape == (4, 8, 10, 4)
            assert out["trends"][1].any() and out["trends"][0].any()
            continue
        assert bits_equal_nan(out["test"], first["test"]), opts
        assert bits_equal(out["weights"], first["weights"]), opts
        assert bits_equal_nan(out["trends"][0], first["trends"][0]), opts
        assert bits_equal_nan(out["trends"][1], first["trends"][1]), opts


# ------------------------------------------------------------------ batch and refusals

@pytest.mark.parametrize("lanes", (1, 2))
def test_batch_equals_single_sessions(lanes, monkeypatch):
    from iterative_cleaner_amd import _native, batch, synth
    monkeypatch.delenv("IC_DETREND", raising=False)
    monkeypatch.delenv("IC_DETREND_PIECES", raising=False)
    shape = (4, 16, 64)
    arcs, refs = [], []
    for k in range(3):
        data, w0, shift = synth.make_cube(*shape, 300 + k, 0.1)
        cube = np.ascontiguousarray(data[:, 0] * ref.tooth_gain(16, 4).astype(np.float32)[None, :, None])
        arcs.append((cube, w0, shift))
        with _native.GpuSession(*shape, device=0, detrend=(1, 2), detrend_pieces=(None, 4)) as s:
            s.upload(cube, w0, shift)
            refs.append(s.run())
        with _native.GpuSession(*shape, device=0, detrend=(1, 2)) as s:
            s.upload(cube, w0, shift)
            whole = s.run()
        assert not bits_equal_nan(whole["test"], refs[-1]["test"])
    got = list(batch.clean_batch(iter(arcs), shape, device=0, lanes=lanes, detrend=(1, 2), detrend_pieces=(None, 4)))
    assert len(got) == 3
    for a, b in zip(got, refs):
        assert a["loops"] == b["loops"] and a["n_iter"] == b["n_iter"]
        assert bits_equal_nan(a["test"], b["test"]) and bits_equal(a["weights"], b["weights"])


def test_shard_session_refuses():
    from iterative_cleaner_amd import _native
    with _native.ShardGroup(2) as g:
        sess = [_native.ShardSession(3, 512, 64, r, 2, group=g, device=0) for r in range(2)]
        try:
            for s in sess:
                with pytest.raises(_native.NativeError, match="rc=%d" % IC_EINVAL):
                    s.set_detrend_pieces(None, [0, 16])
                with pytest.raises(_native.NativeError, match="rc=%d" % IC_EINVAL):
                    s.set_detrend_pieces(None, None)
        finally:
            for s in sess:
                s.close()
