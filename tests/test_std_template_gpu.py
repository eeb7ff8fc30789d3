"""Cleaning against a supplied standard profile on the GPU: the alignment
kernels against their written definition (std_template.py), the replay of the
reference's own iterations through an installed template, the one-pass loop,
and the feature under the other modes, on shards and in the batch scheduler."""
import os
import threading

import numpy as np
import pytest

from helpers import GOLDEN, bits_equal, bits_equal_nan, case_kwargs, load_clean_case
from std_template_cases import delayed, noisy, pulse

pytestmark = pytest.mark.gpu


def _fixture(name):
    return os.path.join(GOLDEN, "%s.npz" % name)


def _run(raw, w0, shift, std=None, max_iter=5, args=None, clear=False, **kw):
    """One session, one run: the ic_run dict plus T, amp, info, diag."""
    from iterative_cleaner_amd import _native
    a = dict(max_iter=max_iter, chanthresh=5.0, subintthresh=5.0, pulse_region=(0, 0, 1))
    a.update(args or {})
    a["max_iter"] = max_iter
    nsub, nchan, nbin = raw.shape
    with _native.GpuSession(nsub, nchan, nbin, a["max_iter"], a["chanthresh"], a["subintthresh"], a["pulse_region"],
                            device=0, std_template=std, **kw) as s:
        if clear:
            s.clear_std_template()
        s.upload(raw, w0, shift)
        out = s.run()
        out["T"] = s.template()
        out["amp"], out["info"] = s.fit()
        out["diag"] = s.diagnostics()
    return out


def _same_results(a, b, what=""):
    """Everything an iteration leaves, bit for bit."""
    assert bits_equal(a["weights"], b["weights"]), "weights %s (%d differ)" % (
        what, int((a["weights"] != b["weights"]).sum()))
    assert bits_equal_nan(a["test"], b["test"]), "test values " + what
    assert bits_equal(a["amp"], b["amp"]) and bits_equal(a["info"], b["info"]), "fit " + what
    for x, y, name in zip(a["diag"], b["diag"], ("std", "mean", "ptp", "fftmax")):
        assert bits_equal_nan(x, y), "%s %s" % (name, what)
    assert bits_equal(a["T"], b["T"]), "template " + what


# ---------------------------------------------------------------- 1. the kernels equal the module

# 64: one block; 100: no rotation (int only); 128: two blocks; 1000: the
# mixed-radix rotation; 1024; 2048: the rotation's LDS-table variant; 8192:
# the largest LDS footprint of k_std_ccf (64 KiB) and 128 blocks
ALIGN_NBINS = (64, 100, 128, 1000, 1024, 2048, 8192)

_module_cache = {}


def _module(S, A, mode):
    """std_template.align, computed once per input (the 8192-bin sums take a
    few tenths of a second on the host)."""
    from iterative_cleaner_amd import std_template as st
    key = (S.tobytes(), A.tobytes(), mode)
    if key not in _module_cache:
        _module_cache[key] = st.align(S, A, mode)
    return _module_cache[key]


def _standards(nbin):
    """(name, S) against A = the noisy test pulse: an integer delay, a fractional
    one and a half-bin one (rolls where the rotation does not serve nbin)."""
    from iterative_cleaner_amd.dedispersion import fft_supported
    P = pulse(nbin)
    if not fft_supported(nbin):
        return [("roll 0", P.copy()), ("roll 7", np.roll(P, -7)), ("roll n-1", np.roll(P, -(nbin - 1)))]
    return [("delay 11", np.roll(P, -11)), ("delay 3.37", delayed(P, 3.37)), ("delay 20.5", delayed(P, 20.5))]


@pytest.mark.parametrize("nbin", ALIGN_NBINS)
def test_align_template_equals_the_module(nbin):
    """ic_align_template against std_template.align: lag, shift and aligned
    equal, the installed template bit-equal, in every mode the length has, for
    three delays and for both failure cases (a NaN in A; A = -S)."""
    from iterative_cleaner_amd import _native
    from iterative_cleaner_amd.dedispersion import fft_supported
    A = noisy(pulse(nbin), nbin)
    modes = ("none", "int", "frac") if fft_supported(nbin) else ("none", "int")
    for name, S in _standards(nbin):
        for mode in modes:
            got, want = _native.align_template(S, A, mode), _module(S, A, mode)
            assert (got["aligned"], got["lag"], got["mode"]) == (want["aligned"], want["lag"], want["mode"]), (name, mode)
            assert got["shift"] == want["shift"], (name, mode, got["shift"], want["shift"])
            assert bits_equal(got["template"], want["template"]), (name, mode)
            if mode != "none":
                assert got["aligned"] == 1, (name, mode)
    S = _standards(nbin)[1][1]
    bad = A.copy()
    bad[nbin // 3] = np.nan
    for against in (bad, -S):
        for mode in modes[1:]:
            got = _native.align_template(S, against, mode)
            assert (got["aligned"], got["lag"], got["shift"]) == (0, 0, 0.0), mode
            assert bits_equal(got["template"], S), mode
            want = _module(S, against, mode)
            assert (want["aligned"], want["lag"], want["shift"]) == (0, 0, 0.0)
    if not fft_supported(nbin):
        with pytest.raises(ValueError, match="use 'int'"):
            _native.align_template(S, A, "frac")


def test_library_validates_the_standard():
    """ic_set_std_template's own checks (the Python layer checks first, so the
    library is called directly)."""
    import ctypes as C

    from iterative_cleaner_amd import _native
    from iterative_cleaner_amd import std_template as st
    with _native.GpuSession(2, 4, 100, device=0) as s:
        def rc(S, nbin, mode):
            S = np.ascontiguousarray(S, np.float32)
            return s.lib.ic_set_std_template(s.h, C.c_void_p(S.ctypes.data), nbin, mode)
        P = pulse(100)
        assert rc(P, 100, st.ALIGN_INT) == 0
        assert rc(P[:64], 64, st.ALIGN_INT) == -1                # another length
        assert rc(np.ones(100), 100, st.ALIGN_INT) == -1         # constant
        bad = P.copy()
        bad[5] = np.inf
        assert rc(bad, 100, st.ALIGN_INT) == -1
        assert rc(P, 100, 3) == -1
        assert rc(P, 100, st.ALIGN_FRAC) == -1                   # 100 bins: no rotation
        assert b"IC_ALIGN_INT" in s.lib.ic_last_error()
        with pytest.raises(_native.NativeError, match="before|no completed"):
            s.std_alignment()
    with _native.GpuSession(2, 4, 64, device=0) as s:
        with pytest.raises(_native.NativeError, match="no standard"):
            s.std_alignment()


@pytest.mark.parametrize("grid_cap", [1, 3])
@pytest.mark.parametrize("nbin,mode", [(100, "int"), (256, "int"), (256, "frac"), (1000, "frac"), (2048, "frac")])
def test_session_alignment_under_the_grid_cap(nbin, mode, grid_cap):
    """Through a session whose grids are capped at 1 and 3 blocks (k_std_ccf then
    walks 2 to 32 lag blocks per block, k_std_install more than one tile; at
    2048 bins the one-profile rotation is the variant that reads the session's
    own stage tables): the
    alignment record and the installed template are the module's for A = the
    archive's own first template, and equal the uncapped session's run."""
    from iterative_cleaner_amd import synth
    data, w0, shift = synth.make_cube(4, 24, nbin, 11, 0.2)
    raw = np.ascontiguousarray(data[:, 0])
    A = _run(raw, w0, shift, max_iter=1)["T"]
    S = np.roll(A, -13) if mode == "int" else delayed(A, 13.4)
    want = _module(S, A, mode)
    free = _run(raw, w0, shift, std=(S, mode), max_iter=1)
    capped = _run(raw, w0, shift, std=(S, mode), max_iter=1, options={"grid_cap": grid_cap})
    for out in (free, capped):
        al = out["std_alignment"]
        assert (al["aligned"], al["lag"], al["shift"]) == (want["aligned"], want["lag"], want["shift"])
        assert al["aligned"] == 1 and al["lag"] == 13
        assert bits_equal(out["T"], want["template"])
    _same_results(capped, free, "capped against uncapped")


# ---------------------------------------------------------------- 2. replay of the reference's iterations

REPLAY_FIXTURES = ["clean_s12x48x128", "clean_s12x40x128_pr", "clean_s12x48x128_f64", "clean_s12x48x128_fft",
                   "clean_s12x48x128_fft_pp", "clean_s10x40x100_thr3", "clean_s8x32x64_pol4", "clean_s6x48x1024",
                   "clean_s4x32x2048_rfi30", "clean_s4x16x8192_rfi20", "mr_clean_s4x16x1000_fft_pr"]


@pytest.mark.parametrize("name", REPLAY_FIXTURES)
def test_replay_of_the_references_iterations(name):
    """Iteration k of the reference depends on the mask only through its
    template T_k: a one-iteration session with std_template = (T_k, "none")
    must leave iteration k's records.  Bit-equal: amp, info, std, mean, ptp,
    weights_k, the template, and the counters against w0; fftmax and the test
    values by test_gpu_parity's 1e-9 rules."""
    import test_gpu_parity as parity
    from iterative_cleaner_amd import _native
    z, meta, raw, w0, shift, args = load_clean_case(_fixture(name))
    nsub, nchan, nbin = raw.shape
    with _native.GpuSession(nsub, nchan, nbin, 1, args["chanthresh"], args["subintthresh"], args["pulse_region"],
                            device=0, data_f64=meta.get("data_f64", False), **case_kwargs(z, meta)) as s:
        for k in range(1, int(z["n_iter"]) + 1):
            Tk = z["T_%d" % k]
            s.set_std_template(Tk, "none")
            s.upload(raw, w0, shift)
            out = s.run()
            amp, info = s.fit()
            sd, mn, pt, ff = s.diagnostics()
            assert out["n_iter"] == 1 and out["loops"] == 1
            assert bits_equal(s.template(), Tk), "template, iteration %d" % k
            assert bits_equal(amp.ravel(), z["amp_%d" % k]), "leastsq amplitudes, iteration %d" % k
            assert bits_equal(info.ravel(), z["info_%d" % k]), "leastsq status, iteration %d" % k
            assert bits_equal_nan(sd, z["diag_std_%d" % k]), "std, iteration %d" % k
            assert bits_equal_nan(mn, z["diag_mean_%d" % k]), "mean, iteration %d" % k
            assert bits_equal_nan(pt, z["diag_ptp_%d" % k]), "ptp, iteration %d" % k
            assert parity._close_fft(ff, z["diag_fft_%d" % k]), "fftmax, iteration %d" % k
            assert parity._close_test(out["test"], z["test_%d" % k]), "test, iteration %d" % k
            wk = z["weights_%d" % k]
            assert bits_equal(out["weights"], wk), "weights, iteration %d" % k
            assert out["changed"][0] == int(np.sum(wk != w0)), "changed against w0, iteration %d" % k
            assert out["nzero"][0] == int(wk.size - np.count_nonzero(wk)), "nzero, iteration %d" % k
            assert out["std_alignment"] == dict(aligned=0, lag=0, shift=0.0)


# ---------------------------------------------------------------- 3. one pass

def test_one_pass_reports_iteration_two():
    """A fixture whose iteration 1 zaps: max_iter 1 and 5 leave identical
    weights, test values, amp and diagnostics; with max_iter = 5 iteration 2 is
    reported (not launched): loops == n_iter == 2, changed == [c, 0],
    nzero[1] == nzero[0], converged, the same bad-fit count."""
    z, meta, raw, w0, shift, args = load_clean_case(_fixture("clean_s12x48x128"))
    T1 = z["T_1"]
    one = _run(raw, w0, shift, std=(T1, "none"), max_iter=1, args=args)
    five = _run(raw, w0, shift, std=(T1, "none"), max_iter=5, args=args)
    two = _run(raw, w0, shift, std=(T1, "none"), max_iter=2, args=args)
    c = int(np.sum(z["weights_1"] != w0))
    assert c > 0, "the fixture's first iteration zaps nothing"
    assert (one["loops"], one["n_iter"], one["converged"]) == (1, 1, False)
    assert list(one["changed"]) == [c]
    for out in (five, two):
        _same_results(out, one, "max_iter %d against 1" % out["loops"])
        assert (out["loops"], out["n_iter"], out["converged"]) == (2, 2, True)
        assert list(out["changed"]) == [c, 0]
        assert out["nzero"][1] == out["nzero"][0] == one["nzero"][0]
        assert list(out["bad_fits"]) == [one["bad_fits"][0]] * 2


def test_one_pass_unchanged_mask_ends_after_one_loop():
    """All weights zero: nothing can change, loops == 1 (and the zero template
    the archive gives fails the alignment, which is no error)."""
    z, meta, raw, w0, shift, args = load_clean_case(_fixture("clean_s4x16x64_w0_edge"))
    out = _run(raw, w0, shift, std=(pulse(64), "int"), max_iter=5, args=args)
    assert (out["loops"], out["n_iter"], out["converged"]) == (1, 1, True)
    assert list(out["changed"]) == [0]
    assert out["std_alignment"]["aligned"] == 0 and bits_equal(out["T"], pulse(64))
    assert bits_equal(out["weights"], w0)


# ---------------------------------------------------------------- 4. alignment end to end

@pytest.mark.parametrize("name", ["clean_s12x48x128", "clean_s6x48x1024"])
def test_alignment_end_to_end(name):
    """The fixture's final template, rolled by 37 bins, in mode int: lag == 37
    and every result bit-equal to the replay with the unrolled template.  In
    mode frac, delayed by 5.3 bins: the template in use is the module's aligned
    standard bit for bit, and the zap mask is the unrotated replay's."""
    z, meta, raw, w0, shift, args = load_clean_case(_fixture(name))
    T = z["T_%d" % int(z["n_iter"])]
    A = z["T_1"]     # the archive's own first template (pinned by test_gpu_parity)
    replay = _run(raw, w0, shift, std=(T, "none"), max_iter=5, args=args)
    rolled = _run(raw, w0, shift, std=(np.roll(T, -37), "int"), max_iter=5, args=args)
    assert rolled["std_alignment"]["aligned"] == 1 and rolled["std_alignment"]["lag"] == 37
    _same_results(rolled, replay, "rolled against unrolled")
    for key in ("loops", "n_iter", "converged"):
        assert rolled[key] == replay[key]
    assert np.array_equal(rolled["changed"], replay["changed"]) and np.array_equal(rolled["nzero"], replay["nzero"])
    S = delayed(T, 5.3)
    want = _module(S, A, "frac")
    frac = _run(raw, w0, shift, std=(S, "frac"), max_iter=5, args=args)
    al = frac["std_alignment"]
    assert (al["aligned"], al["lag"], al["shift"]) == (want["aligned"], want["lag"], want["shift"])
    print("%s: delay 5.3 recovered as %.6f" % (name, al["shift"]))
    assert al["aligned"] == 1 and al["lag"] == 5
    assert bits_equal(frac["T"], want["template"])
    differing = int((frac["weights"] != replay["weights"]).sum())
    assert differing == 0, "%d of %d profiles zapped differently after the fractional alignment" % (
        differing, replay["weights"].size)


# ---------------------------------------------------------------- 5. other modes

def _synth256():
    from iterative_cleaner_amd import synth
    data, w0, shift = synth.make_cube(6, 40, 256, 21, 0.25)
    return np.ascontiguousarray(data[:, 0]), w0, shift


def _other_modes():
    from iterative_cleaner_amd import _native, synth
    raw, w0, shift = _synth256()
    d2 = synth.per_profile_delays(shift, 256, 6)
    return {"closed": dict(fit_mode=_native.FIT_CLOSED), "fft_pp": dict(delay=d2), "detrend": dict(detrend=(1, 2))}


@pytest.mark.parametrize("mode", ["closed", "fft_pp", "detrend"])
def test_other_modes_replay_their_own_template(mode):
    """The closed-form fit (k_tnorm reads the installed T64), the FFT mode with
    per-profile delays, detrended scaling (1, 2): a default run followed by a
    replay with its own final template reproduces the last iteration bit for
    bit; and a session whose standard was set and then cleared runs the
    default loop's bits."""
    raw, w0, shift = _synth256()
    kw = _other_modes()[mode]
    default = _run(raw, w0, shift, max_iter=5, **kw)
    assert default["n_iter"] >= 2, "the synthetic archive converges at once: nothing to replay"
    replay = _run(raw, w0, shift, std=(default["T"], "none"), max_iter=1, **kw)
    _same_results(replay, default, "replay against the default run's last iteration (%s)" % mode)
    cleared = _run(raw, w0, shift, std=(np.roll(default["T"], 9), "int"), max_iter=5, clear=True, **kw)
    _same_results(cleared, default, "set then cleared (%s)" % mode)
    for key in ("loops", "n_iter", "converged"):
        assert cleared[key] == default[key]
    assert np.array_equal(cleared["changed"], default["changed"]) and "std_alignment" not in cleared


# ---------------------------------------------------------------- 6. shards

def _shard_archive():
    from iterative_cleaner_amd import synth
    data, w0, shift = synth.make_cube(3, 300, 128, 5, 0.2)
    return np.ascontiguousarray(data[:, 0]), w0, shift


def test_two_shards_equal_one_gpu():
    """Two in-process shards, the standard rolled, mode int: every rank aligns
    for itself against the same scrunched template; the merged result is the
    single session's bit for bit."""
    from iterative_cleaner_amd import sharded
    raw, w0, shift = _shard_archive()
    T = _run(raw, w0, shift, max_iter=5)["T"]
    S = np.roll(T, -21)
    one = _run(raw, w0, shift, std=(S, "int"), max_iter=5)
    out = sharded.clean_cube_local(raw, w0, shift, 2, want_details=True, std_template=(S, "int"))
    assert out["std_alignment"] == one["std_alignment"] and out["std_alignment"]["lag"] == 21
    assert bits_equal(out["weights"], one["weights"]) and bits_equal_nan(out["test"], one["test"])
    assert bits_equal(out["amp"], one["amp"]) and bits_equal(out["info"], one["info"])
    for x, y in zip((out["std"], out["mean"], out["ptp"], out["fft"]), one["diag"]):
        assert bits_equal_nan(x, y)
    assert bits_equal(out["T"], one["T"]) and bits_equal(out["T"], T)
    for key in ("loops", "n_iter", "converged"):
        assert out[key] == one[key]
    assert np.array_equal(out["changed"], one["changed"]) and np.array_equal(out["nzero"], one["nzero"])


@pytest.mark.parametrize("modes", [("int", "none"), ("int", None), (None, "frac")])
def test_shards_that_disagree_are_detected(modes):
    """A rank that set a different mode, or is the only one to set a standard
    (None: none set), is DETECTED, not refused when it is set (a rank knows
    nothing of its peers then): the counters' all-reduce of every shard run
    carries two words of a hash of the standard and mode, zeros where none is
    set, and ic_run fails with IC_EINVAL on every rank whose words differ from
    the sum's share.  No new exchange, no hang: both ranks fail at the same
    collective, whose count does not depend on what a rank set."""
    from iterative_cleaner_amd import _native
    raw, w0, shift = _shard_archive()
    nsub, nchan, nbin = raw.shape
    S = np.roll(pulse(nbin), -21)
    chans, _ = _native.shard_layout(nsub, nchan, 2)
    errors = [None, None]
    with _native.ShardGroup(2) as group:
        sessions = []
        try:
            for r, mode in enumerate(modes):
                sessions.append(_native.ShardSession(nsub, nchan, nbin, r, 2, group=group, device=0,
                                                     std_template=None if mode is None else (S, mode)))
            for r, s in enumerate(sessions):
                c0, c1 = chans[r]
                s.upload(raw[:, c0:c1], w0[:, c0:c1], shift[c0:c1])

            def work(r):
                try:
                    sessions[r].run()
                except _native.NativeError as e:
                    errors[r] = str(e)

            threads = [threading.Thread(target=work, args=(r,)) for r in range(2)]
            for t in threads:
                t.start()
            for t in threads:
                t.join()
        finally:
            for s in sessions:
                s.close()
    for e in errors:
        assert e is not None and "different standard templates or alignment" in e, e


# ---------------------------------------------------------------- 7. batch

@pytest.mark.parametrize("lanes", [1, 2])
def test_clean_batch_equals_single_sessions(lanes):
    """Four (8, 64, 128) archives with different seeds through the batch
    scheduler, the standard set once per lane and aligned per archive: the
    results and out["std_alignment"] are four single sessions'."""
    from iterative_cleaner_amd import batch, synth
    arcs = []
    for seed in (1, 2, 3, 4):
        data, w0, shift = synth.make_cube(8, 64, 128, seed, 0.2)
        arcs.append((np.ascontiguousarray(data[:, 0]), w0, shift.astype(np.int32)))
    S = delayed(_run(*arcs[0], max_iter=5)["T"], 9.25)
    got = list(batch.clean_batch(iter(arcs), (8, 64, 128), device=0, lanes=lanes, std_template=(S, "frac")))
    assert len(got) == 4
    shifts = set()
    for k, ((raw, w0, shift), out) in enumerate(zip(arcs, got)):
        ref = _run(raw, w0, shift, std=(S, "frac"), max_iter=5)
        assert out["std_alignment"] == ref["std_alignment"], k
        assert out["std_alignment"]["aligned"] == 1 and out["std_alignment"]["lag"] == 9, k
        shifts.add(out["std_alignment"]["shift"])
        assert out["loops"] == ref["loops"] and np.array_equal(out["changed"], ref["changed"]), k
        assert bits_equal(out["weights"], ref["weights"]) and bits_equal_nan(out["test"], ref["test"]), k
    assert len(shifts) > 1, "every archive gave the same sub-bin shift: the alignment is not per archive"
