"""Detrended scaling on the GPU (k_linetrend, k_combine_dt; ic_set_detrend,
ic_get_trends, ic_comprehensive_stats_detrend) against the written definition.

The yardstick: the GPU's own std / mean / ptp / fftmax of the run and valid =
(w0 != 0) go through iterative_cleaner_amd/detrend.py and the tests' combine
(tests/detrend_ref.combine: restated's scalers and NaN rule).  The test values,
the weights and the trend coefficients must match BIT FOR BIT (a NaN matches a
NaN).  No tolerance: the diagnostics are the GPU's own, so fftmax's last bits
do not enter, and every trend operation is a separately rounded f64 operation
on both sides.

The session cube is the 12 x 96 x 128 synthetic cube with a 3x gain slope across
the band and four profiles at the low-gain end carrying extra noise
(detrend_ref.sloped_cube, seeds fixed here).  The extra noise is 1.0 of the
channel's sigma: at 1.5 sigma the channel direction alone (12 subints of equal
gain) already zaps all four planted profiles of this generator with and
without detrending, so nothing could hide; at 1.0 the first iteration of the
statement, fed with the C oracle's diagnostics, zaps 1 of the 4 undetrended
and 3 of the 4 detrended with orders (1, 2) (exact and closed-form fit; 1 and
2 with the fractional delays), and no test value lies within 1e-2 of the
threshold: checked on the CPU before the seeds were fixed.

Every test here fails on a library without the ic_set_detrend symbol.
"""
import argparse

import numpy as np
import pytest

import detrend_ref
from helpers import bits_equal, bits_equal_nan

pytestmark = pytest.mark.gpu

SEED, SEED2, EXTRA = 12, 112, 1.0
ORDERS = (1, 2)
IC_EINVAL, IC_ESTATE = -1, -4

_CUBES = {}


def _cube(shape):
    if shape not in _CUBES:
        planted = detrend_ref.PLANTED if shape[:2] == (12, 96) else ((1, 150), (3, 155), (5, 148), (6, 158))
        _CUBES[shape] = detrend_ref.sloped_cube(*shape, SEED, SEED2, planted=planted, extra=EXTRA)
    return _CUBES[shape]


def _run(shape, detrend="never", max_iter=1, delay=None, fit_mode=0, options=None, data_f64=False, timing=False):
    """One session run; detrend "never": ic_set_detrend is not called."""
    from iterative_cleaner_amd import _native
    raw, w0, shift = _cube(shape)
    kw = {} if detrend == "never" else {"detrend": detrend}
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


def _check_yardstick(out, w0, detrend, chanthresh=5.0, subintthresh=5.0):
    valid = np.asarray(w0) != 0
    test, cc, sc, _ = detrend_ref.combine(out["diags"], valid, chanthresh, subintthresh, detrend)
    assert bits_equal_nan(out["test"], test), "test values (%d differ)" % int(
        (~((out["test"] == test) | (np.isnan(out["test"]) & np.isnan(test)))).sum())
    with np.errstate(invalid="ignore"):
        want_w = np.where(test >= 1.0, np.float32(0.0), np.asarray(w0, np.float32)).astype(np.float32)
    assert bits_equal(out["weights"], want_w), "weights"
    gc, gs = out["trends"]
    assert bits_equal_nan(gc, cc), "channel coefficients"
    assert bits_equal_nan(gs, sc), "subint coefficients"
    return test


# ------------------------------------------------------------------ one-shot

@pytest.mark.parametrize("data_f64", (False, True), ids=("f32", "f64"))
@pytest.mark.parametrize("orders", ((1, 1), (2, 3), (3, 0), (0, 2)))
@pytest.mark.parametrize("shape", ((1, 5), (2, 3), (3, 65), (65, 4), (130, 7)))
def test_one_shot_matches_the_statement(shape, orders, data_f64):
    """Lines of 1 and 2 values (a zero trend: n <= k, or the n == 1 pivot), the
    chain boundary 63/64/65 and three passes of a chain (130); a bandpass slope,
    zero-weight profiles, a dead channel, a NaN and an Inf sample, a constant
    channel; ptp in f32 and (data_f64) in f64."""
    from iterative_cleaner_amd import _native
    nsub, nchan = shape
    data, w = detrend_ref.hard_cube(nsub, nchan, 64, 40 + nsub)
    test, (cc, sc), diags = _native.comprehensive_stats(data, w, 5.0, 4.0, diagnostics=True, detrend=orders,
                                                        data_f64=data_f64)
    assert diags[2].dtype == (np.float64 if data_f64 else np.float32)
    want, wc, ws, used = detrend_ref.combine(diags, w != 0, 5.0, 4.0, orders)
    assert bits_equal_nan(test, want)
    assert bits_equal_nan(cc, wc) and bits_equal_nan(sc, ws)
    if nchan >= 5 and nsub >= 3:
        assert np.isnan(want).any() and not np.isnan(want).all()
    if min(orders) == 0:                       # the direction that is off has no trend
        assert not (cc if orders[0] == 0 else sc).any()
    if nsub <= orders[0]:
        assert not cc.any()
    if nsub >= 65 and orders[0] and nchan >= 4:
        assert cc[0, 0].any() and max(used) >= 1


def test_one_shot_refusals():
    from iterative_cleaner_amd import _native
    data, w = detrend_ref.hard_cube(3, 5, 64, 1)
    for bad in ((4, 0), (-1, 1), (1, 1, 0), (1, 1, 9), (1, 1, 4, 0.0), (1, 1, 4, float("nan"))):
        with pytest.raises(_native.NativeError, match=r"rc=-1"):
            _native.comprehensive_stats(data, w, detrend=bad)


# ------------------------------------------------------------------ sessions

SHAPE = (12, 96, 128)
_PLAIN = {}


def _plain(max_iter, **kw):
    key = (max_iter, tuple(sorted((k, id(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items())))
    if key not in _PLAIN:
        _PLAIN[key] = _run(SHAPE, "never", max_iter, **kw)
    return _PLAIN[key]


def _session_case(max_iter, **kw):
    raw, w0, shift = _cube(SHAPE)
    out = _run(SHAPE, ORDERS, max_iter, **kw)
    test = _check_yardstick(out, w0, ORDERS)
    assert out["stats"]["near_threshold"] == 0
    assert np.nanmin(np.abs(test - 1.0)) > 1e-9
    plain = _plain(max_iter, **kw)
    assert "trends_error" in plain and "rc=%d" % IC_ESTATE in plain["trends_error"]
    with np.errstate(invalid="ignore"):
        mask, mask0 = out["test"] >= 1.0, plain["test"] >= 1.0
    assert (mask != mask0).any(), "the detrended mask equals the undetrended one"
    hit = sum(bool(mask[s, c]) for s, c in detrend_ref.PLANTED)
    hit0 = sum(bool(mask0[s, c]) for s, c in detrend_ref.PLANTED)
    print("planted zapped: %d detrended, %d undetrended; %d decisions differ" % (hit, hit0, int((mask != mask0).sum())))
    assert hit > hit0
    return out


@pytest.mark.parametrize("max_iter", (1, 3))
def test_session_exact_fit_integer_shifts(max_iter):
    out = _session_case(max_iter)
    assert out["n_iter"] >= 1


def test_session_fractional_delays():
    from iterative_cleaner_amd import synth
    delay = synth.fractional_delays(_cube(SHAPE)[2], SHAPE[2])
    _session_case(3, delay=delay)


def test_session_closed_form_fit():
    from iterative_cleaner_amd import _native
    _session_case(3, fit_mode=_native.FIT_CLOSED)


def test_session_f64_data_and_other_orders():
    """data_f64 (ptp lines in f64) and the orders (2, 3), (3, 0): the yardstick alone."""
    raw, w0, shift = _cube(SHAPE)
    for orders, f64 in (((2, 3), True), ((3, 0, 2, 3.0), False)):
        out = _run(SHAPE, orders, 2, data_f64=f64)
        _check_yardstick(out, w0, orders)


# ------------------------------------------------------------------ schedules

SCHEDULES = ({}, {"grid_cap": 1}, {"rowstat_waves": 0}, {"rowstat_waves": 4, "rowstat_minlen": 64},
             {"rowstat_waves": 8, "rowstat_minlen": 64}, {"diag_fork": 0})


def test_schedules_give_the_same_bits():
    """8 x 160 x 64: the last two rowstat settings put the 160-long rows on the
    multi-wave path (k_linetrend<4>, <8>)."""
    shape = (8, 160, 64)
    raw, w0, shift = _cube(shape)
    ref = None
    for opts in SCHEDULES:
        out = _run(shape, ORDERS, 2, options=opts)
        if ref is None:
            ref = out
            _check_yardstick(out, w0, ORDERS)
            assert out["trends"][1].any() and out["trends"][0].any()
            continue
        assert bits_equal_nan(out["test"], ref["test"]), opts
        assert bits_equal(out["weights"], ref["weights"]), opts
        assert bits_equal_nan(out["trends"][0], ref["trends"][0]), opts
        assert bits_equal_nan(out["trends"][1], ref["trends"][1]), opts


# ------------------------------------------------------------------ off is off

def test_off_is_off(monkeypatch):
    """detrend=(0, 0) and an unset switch: the bits and the launch counts of a
    session that never called ic_set_detrend; ic_get_trends then IC_ESTATE."""
    from iterative_cleaner_amd import cleaner
    monkeypatch.delenv("IC_DETREND", raising=False)
    never = _run(SHAPE, "never", 3, timing=True)
    off = _run(SHAPE, (0, 0), 3, timing=True)
    again = _run(SHAPE, (0, 0, 8, 2.0), 3, timing=True)
    for o in (off, again):
        assert bits_equal_nan(o["test"], never["test"]) and bits_equal(o["weights"], never["weights"])
        assert o["launches"] == never["launches"]
        assert "rc=%d" % IC_ESTATE in o["trends_error"]
    assert "rc=%d" % IC_ESTATE in never["trends_error"]
    assert never["launches"]["k_linestats"] > 0 and never["launches"]["k_combine"] > 0
    # the switch unset (and "0"): run_loop gives the same bits; set, the detrended ones
    raw, w0, shift = _cube(SHAPE)
    args = argparse.Namespace(max_iter=3, chanthresh=5.0, subintthresh=5.0, pulse_region=[0, 0, 1])
    assert bits_equal_nan(cleaner.run_loop(raw, w0, shift, args)["test"], never["test"])
    monkeypatch.setenv("IC_DETREND", "0")
    assert bits_equal_nan(cleaner.run_loop(raw, w0, shift, args)["test"], never["test"])
    monkeypatch.setenv("IC_DETREND", "%d,%d" % ORDERS)
    on = _run(SHAPE, ORDERS, 3)
    assert bits_equal_nan(cleaner.run_loop(raw, w0, shift, args)["test"], on["test"])
    assert not bits_equal_nan(on["test"], never["test"])
    # switched on and off again on one session
    from iterative_cleaner_amd import _native
    with _native.GpuSession(*SHAPE, max_iter=3, device=0) as s:
        s.upload(raw, w0, shift)
        s.set_detrend(*ORDERS)
        assert bits_equal_nan(s.run()["test"], on["test"])
        s.trends()
        s.set_detrend(0, 0)
        with pytest.raises(_native.NativeError, match="rc=%d" % IC_ESTATE):
            s.trends()
        assert bits_equal_nan(s.run()["test"], never["test"])
        for bad in ((4, 1), (1, -1), (1, 1, 0), (1, 1, 9), (1, 1, 4, 0.0), (1, 1, 4, float("inf"))):
            with pytest.raises(_native.NativeError, match="rc=%d" % IC_EINVAL):
                s.set_detrend(*bad)


# ------------------------------------------------------------------ batch and refusals

@pytest.mark.parametrize("lanes", (1, 2))
def test_batch_equals_single_sessions(lanes, monkeypatch):
    from iterative_cleaner_amd import _native, batch, synth
    monkeypatch.delenv("IC_DETREND", raising=False)
    shape = (4, 16, 64)
    arcs, refs = [], []
    for k in range(3):
        data, w0, shift = synth.make_cube(*shape, 300 + k, 0.1)
        cube = np.ascontiguousarray(data[:, 0] * np.linspace(3.0, 1.0, 16, dtype=np.float32)[None, :, None])
        arcs.append((cube, w0, shift))
        with _native.GpuSession(*shape, device=0, detrend=(1, 2)) as s:
            s.upload(cube, w0, shift)
            refs.append(s.run())
        with _native.GpuSession(*shape, device=0) as s:
            s.upload(cube, w0, shift)
            plain = s.run()
        assert not bits_equal_nan(plain["test"], refs[-1]["test"])
    got = list(batch.clean_batch(iter(arcs), shape, device=0, lanes=lanes, detrend=(1, 2)))
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
                    s.set_detrend(1, 1)
                with pytest.raises(_native.NativeError, match="rc=%d" % IC_EINVAL):
                    s.set_detrend(0, 0)
        finally:
            for s in sess:
                s.close()


def test_run_loop_refuses_under_channel_sharding(monkeypatch):
    from iterative_cleaner_amd import _native, cleaner, dist
    assert _native.load_library().ic_set_detrend           # the feature's symbol
    monkeypatch.setattr(dist, "channel_sharding", lambda: True)

    def no_session(*a, **k):
        raise AssertionError("a session was made")
    monkeypatch.setattr(_native, "GpuSession", no_session)
    raw, w0, shift = _cube(SHAPE)
    args = argparse.Namespace(max_iter=1, chanthresh=5.0, subintthresh=5.0, pulse_region=[0, 0, 1])
    with pytest.raises(ValueError, match="channel sharding"):
        cleaner.run_loop(raw, w0, shift, args, detrend=ORDERS)
