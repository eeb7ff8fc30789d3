"""Hot-bin repair on the GPU: k_hotbins and the hit list against the written
definition (hotbins.py) bit for bit, sessions against the oracle's CPU loop run
on the definition's repaired cube, the benefit on spiked profiles, and the
feature off, re-run, re-uploaded, on shards and in the batch scheduler."""
import ctypes as C
import threading

import numpy as np
import pytest

import hotbins_cases as hc
from helpers import bits_equal, bits_equal_nan

pytestmark = pytest.mark.gpu

NBINS = (64, 100, 128, 1024, 1025, 2048, 8192)


# ---------------------------------------------------------------- 1. the kernels equal the module

_want = {}


def _module(nbin, name):
    """hotbins.repair_profiles of the shared profiles under one parameter set,
    computed once."""
    from iterative_cleaner_amd import hotbins as hb
    if (nbin, name) not in _want:
        X, w, offs, _ = hc.profiles(nbin)
        widen, thr, a, b, rounds = hc.param_sets(nbin)[name]
        _want[nbin, name] = hb.repair_profiles(X, w, offs, widen, thr, a, b, rounds)
    return _want[nbin, name]


def _same(got, want, what):
    out, count, bins = got
    wout, wcount, wbins = want
    assert np.array_equal(count, wcount), "%s: counts differ at %s (%s != %s)" % (
        what, np.nonzero(count != wcount)[0][:8], count[count != wcount][:8], wcount[count != wcount][:8])
    assert bits_equal(bins, wbins), "%s: hit list" % what
    assert bits_equal_nan(out, wout), "%s: repaired profiles %s differ" % (
        what, np.nonzero((out != wout).any(axis=1) & ~np.isnan(out).any(axis=1))[0][:8])


@pytest.mark.parametrize("nbin", NBINS)
def test_kernels_equal_the_module(nbin):
    """ic_hotbins_profiles against hotbins.repair_profiles: the output cube, the
    counts and the list, bit for bit and with no exclusions, for 6 x 8 profiles
    (every edge case of the definition, seeded noise with spikes) under every
    parameter set."""
    from iterative_cleaner_amd import _native
    X, w, offs, names = hc.profiles(nbin)
    seen = set()
    for name, (widen, thr, a, b, rounds) in hc.param_sets(nbin).items():
        want = _module(nbin, name)
        got = _native.hotbins_profiles(X, w, offs, widen, thr, a, b, rounds)
        _same(got, want, "nbin %d, %s" % (nbin, name))
        seen |= set(np.sign(want[1]).tolist())
    assert seen == {-1, 0, 1}      # capped, clean and repaired profiles all occur
    # the edge cases do what they were made for (the definition's own behaviour)
    count = _module(nbin, "plain")[1]
    n_off = len(hc.off_bins(nbin, 0, *hc.param_sets(nbin)["plain"][2:4]))
    cap = n_off // 4
    # (tied medians: an odd count puts the median on one of the two values and the MAD at 0)
    for k, c in ((0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (5, 2), (6, cap), (7, -1), (8, 0), (9, 0), (10, 3),
                 (11, 1 - n_off % 2), (12, 0)):
        assert count[k] == c, (nbin, names[k], int(count[k]), c)
    assert _module(nbin, "one round")[1][13] != count[13], "heavy tails: later rounds found nothing more"


def test_kernels_equal_the_module_no_offsets():
    """offsets NULL is offset 0."""
    from iterative_cleaner_amd import _native
    from iterative_cleaner_amd import hotbins as hb
    X, w, _, _ = hc.profiles(128)
    _same(_native.hotbins_profiles(X, w, None, 0, 4.0, 32, 48, 4), hb.repair_profiles(X, w, None, 0, 4.0, 32, 48, 4),
          "no offsets")


def _session_hot(nbin, options=None, **kw):
    """The shared profiles as a 6 x 8 archive through a session (their first
    eight offsets as the channels' shifts): the run's ``hotbins`` and the inputs
    the module needs to state the same."""
    from iterative_cleaner_amd import _native
    X, w, offs, _ = hc.profiles(nbin)
    widen, thr, a, b, rounds = hc.param_sets(nbin)["plain"]
    shift = np.mod(offs[:8].astype(np.int64), nbin)
    with _native.GpuSession(6, 8, nbin, max_iter=1, device=0, options=options, hotbins=(thr, a, b, rounds),
                            **kw) as s:
        s.upload(X.reshape(6, 8, nbin), w.reshape(6, 8), shift)
        out = s.run()
    return out["hotbins"], (X, w, np.tile(shift, 6), thr, a, b, rounds)


@pytest.mark.parametrize("nbin", (100, 1024, 2048))
def test_grid_stride_loop_makes_many_trips(nbin):
    """IC_OPT_GRID_CAP = 1: one block walks every profile (and the fill kernel
    every row); counts and list equal the module's."""
    from iterative_cleaner_amd import hotbins as hb
    got, (X, w, offs, thr, a, b, rounds) = _session_hot(nbin, options={"grid_cap": 1}, fit_mode=1)
    _, count, bins = hb.repair_profiles(X, w, offs, 0, thr, a, b, rounds)
    assert np.array_equal(got["count"].reshape(-1), count) and bits_equal(got["bins"], bins)
    assert got["total"] == bins.shape[0] and got["offsets"][-1] == got["total"]


# ---------------------------------------------------------------- 2. sessions

NSUB, NCHAN, NBIN = 12, 48, 128
HOT = (5.0, 30, 48)          # the synthetic pulse sits at phase 0.3: bins 30..47 hold it at 128 bins


def _archive(seed=3, spikes=True):
    """A 12 x 48 x 128 synthetic archive (no RFI of its own) with two or three
    +-40 spikes in the off-pulse bins of every 7th profile."""
    from iterative_cleaner_amd import synth
    data, w0, shift = synth.make_cube(NSUB, NCHAN, NBIN, seed, 0.0)
    raw = np.ascontiguousarray(data[:, 0])
    rng = np.random.default_rng(seed + 100)
    hit = []
    if spikes:
        for k in range(0, NSUB * NCHAN, 7):
            s, c = divmod(k, NCHAN)
            off = hc.off_bins(NBIN, int(shift[c]), HOT[1] - 2, HOT[2] + 2)
            bins = rng.choice(off, size=2 + k % 2, replace=False)
            raw[s, c, bins] += np.float32(40.0) * rng.choice([-1.0, 1.0], size=bins.shape[0]).astype(np.float32)
            hit.append((s, c))
    return raw, w0, shift, hit


def _gpu_clean(raw, w0, shift, hotbins=None, upload="plain", max_iter=5, options=None, **kw):
    from iterative_cleaner_amd import _native, psrfits
    nsub, nchan, nbin = raw.shape
    with _native.GpuSession(nsub, nchan, nbin, max_iter=max_iter, device=0, hotbins=hotbins, options=options,
                            **kw) as s:
        if upload == "quantised":
            q, scl, offs = psrfits.quantise(raw[:, None])
            s.upload_quantised(q, scl, offs, w0, shift, 1)
        else:
            s.upload(raw, w0, shift)
        return s.run()


def _close(t, u):
    return bool(np.all((t == u) | (np.abs(t - u) <= 1e-9) | (np.isnan(t) & np.isnan(u))))


SESSIONS = {
    "integer shifts": dict(),
    "FFT delays per channel": dict(delay="chan"),
    "FFT delays per profile": dict(delay="prof"),
    "input dedispersed": dict(delay="chan", input_dedispersed=True),
    "quantised upload": dict(upload="quantised"),
    "closed fit": dict(fit_mode=1),
    "fit tiled 0": dict(options={"fit_tiled": 0}),
    "fit tiled 1": dict(options={"fit_tiled": 1}),
}


@pytest.mark.parametrize("name", sorted(SESSIONS))
def test_session_equals_oracle_on_the_repaired_cube(name, oracle_lib):
    """A 12 x 48 x 128 clean with hot bins set equals oracle.lib's CPU loop run
    on the cube hotbins.py repairs: weights and loops bit for bit, test values
    to 1e-9; the counts and the list are the module's."""
    from iterative_cleaner_amd import hotbins as hb
    from iterative_cleaner_amd import psrfits, synth
    kw = dict(SESSIONS[name])
    raw, w0, shift, _ = _archive()
    delay = kw.pop("delay", None)
    if delay is not None:
        delay = synth.fractional_delays(shift, NBIN) if delay == "chan" else synth.per_profile_delays(shift, NBIN, NSUB)
    ded = kw.pop("input_dedispersed", False)
    cube = raw
    if kw.get("upload") == "quantised":
        cube = psrfits.decode(*psrfits.quantise(raw[:, None]))[:, 0]
    fixed, want = hb.repair_cube(cube, w0, HOT, shift=shift, delay=delay, input_dedispersed=ded)
    assert want["total"] > 0
    ref = oracle_lib.clean_loop(fixed, w0, shift, fit_mode=kw.get("fit_mode", 0), delay=delay, input_dedispersed=ded)
    got = _gpu_clean(raw, w0, shift, hotbins=HOT, delay=delay, input_dedispersed=ded, **kw)
    assert np.array_equal(got["hotbins"]["count"], want["count"]), name
    assert bits_equal(got["hotbins"]["bins"], want["bins"]) and got["hotbins"]["total"] == want["total"], name
    assert got["loops"] == ref["loops"], name
    assert bits_equal(got["weights"], ref["weights"]), "%s: %d weights differ" % (
        name, int((got["weights"] != ref["weights"]).sum()))
    assert _close(got["test"], ref["test"]), name


def test_benefit(oracle_lib):
    """The spiked profiles are zapped by the default clean and kept with the
    repair: first on the CPU (oracle on the raw cube, oracle on the repaired
    cube), then the GPU agrees with both.  Fails without the feature."""
    from iterative_cleaner_amd import hotbins as hb
    raw, w0, shift, hit = _archive()
    live = [(s, c) for s, c in hit if w0[s, c] != 0]
    assert len(live) > 10
    plain = oracle_lib.clean_loop(raw, w0, shift)
    fixed, want = hb.repair_cube(raw, w0, HOT, shift=shift)
    mended = oracle_lib.clean_loop(fixed, w0, shift)
    for s, c in live:
        assert plain["weights"][s, c] == 0, "the default clean keeps spiked profile (%d, %d)" % (s, c)
        assert mended["weights"][s, c] != 0, "the repaired clean zaps profile (%d, %d)" % (s, c)
        assert want["count"][s, c] in (2, 3)
    g_plain = _gpu_clean(raw, w0, shift)
    g_mended = _gpu_clean(raw, w0, shift, hotbins=HOT)
    assert bits_equal(g_plain["weights"], plain["weights"]) and g_plain["loops"] == plain["loops"]
    assert bits_equal(g_mended["weights"], mended["weights"]) and g_mended["loops"] == mended["loops"]
    assert "hotbins" not in g_plain and g_mended["hotbins"]["total"] == want["total"]


def test_off_means_off():
    """Never set, or set and cleared: the outputs and the kernel list of
    ic_get_kernel_times equal an untouched session's."""
    from iterative_cleaner_amd import _native
    raw, w0, shift, _ = _archive()

    def run(mode):
        with _native.GpuSession(NSUB, NCHAN, NBIN, device=0) as s:
            if mode == "cleared":
                s.set_hotbins(*HOT)
                s.clear_hotbins()
            elif mode == "on":
                s.set_hotbins(*HOT)
            s.set_timing(True)
            s.upload(raw, w0, shift)
            out = s.run()
            out["residual"] = s.residual()
            out["kernels"] = {k: v["launches"] for k, v in s.kernel_times().items()}
            if mode != "on":
                with pytest.raises(_native.NativeError, match="is off"):
                    s.hotbins()
        return out

    ref, cleared, on = run("never"), run("cleared"), run("on")
    assert ref["kernels"] == cleared["kernels"] and ref["kernels"]["k_hotbins"] == 0
    for key in ("weights", "test", "residual", "changed", "nzero"):
        assert bits_equal_nan(ref[key], cleared[key]), key
    assert ref["loops"] == cleared["loops"] and "hotbins" not in cleared
    assert on["kernels"]["k_hotbins"] == 1 and on["kernels"]["k_hotbin_scan"] == 1   # once per upload


def test_rerun_and_new_upload():
    """A second run of the same upload detects nothing again and keeps results,
    counts and list; a new upload resets them."""
    from iterative_cleaner_amd import _native
    from iterative_cleaner_amd import hotbins as hb
    raw, w0, shift, _ = _archive()
    raw2, w02, shift2, _ = _archive(seed=4, spikes=False)
    raw2[1, 2, 100] += 60.0
    with _native.GpuSession(NSUB, NCHAN, NBIN, device=0, hotbins=HOT) as s:
        with pytest.raises(_native.NativeError, match="no run"):
            s.hotbins()
        s.set_timing(True)
        s.upload(raw, w0, shift)
        with pytest.raises(_native.NativeError, match="no run"):
            s.hotbins()
        a = s.run()
        b = s.run()
        assert s.kernel_times()["k_hotbins"]["launches"] == 1       # two runs, one pass
        assert bits_equal(a["weights"], b["weights"]) and bits_equal_nan(a["test"], b["test"])
        assert a["loops"] == b["loops"]
        for key in ("count", "bins", "offsets"):
            assert bits_equal(a["hotbins"][key], b["hotbins"][key]), key
        assert a["hotbins"]["total"] == b["hotbins"]["total"] > 0
        s.upload(raw2, w02, shift2)
        with pytest.raises(_native.NativeError, match="no run"):
            s.hotbins()
        c = s.run()
        want = hb.repair_cube(raw2, w02, HOT, shift=shift2)[1]
        assert np.array_equal(c["hotbins"]["count"], want["count"]) and bits_equal(c["hotbins"]["bins"], want["bins"])
        assert c["hotbins"]["count"][1, 2] == 1 and c["hotbins"]["total"] == want["total"]
        assert s.kernel_times()["k_hotbins"]["launches"] == 2


def test_async_uploads_each_get_their_pass():
    """Behind ic_upload_async (two archives queued) and ic_upload_pols."""
    from iterative_cleaner_amd import _native
    from iterative_cleaner_amd import hotbins as hb
    raw, w0, shift, _ = _archive()
    raw2, w02, shift2, _ = _archive(seed=4)
    sh, sh2 = shift.astype(np.int32), shift2.astype(np.int32)
    with _native.GpuSession(NSUB, NCHAN, NBIN, device=0, hotbins=HOT) as s:
        s.upload_async(raw, w0, sh)
        s.upload_async(raw2, w02, sh2)
        for cube, w, shf in ((raw, w0, shift), (raw2, w02, shift2)):
            got = s.run()["hotbins"]
            want = hb.repair_cube(cube, w, HOT, shift=shf)[1]
            assert np.array_equal(got["count"], want["count"]) and bits_equal(got["bins"], want["bins"])
        half = (raw * np.float32(0.5)).astype(np.float32)
        pols = np.ascontiguousarray(np.stack([half, (raw - half).astype(np.float32)], axis=1))
        s.upload_pols(pols, w0, shift)
        got = s.run()["hotbins"]
        want = hb.repair_cube((pols[:, 0] + pols[:, 1]).astype(np.float32), w0, HOT, shift=shift)[1]
        assert np.array_equal(got["count"], want["count"]) and bits_equal(got["bins"], want["bins"])


def test_attached_channel_delays_stay_the_sessions_own():
    """An upload without delays keeps the session's per-channel delays for its
    hot-bin pass too, also when the next queued upload brings new delays into
    the input slot the session's came with (its copy is then in flight, or
    done, when the pass reads its offsets)."""
    from iterative_cleaner_amd import _native, synth
    from iterative_cleaner_amd import hotbins as hb
    arcs = {}
    for name, seed, extra in (("A", 3, 0.0), ("B", 4, 20.3), ("C", 5, -33.6)):
        raw, w0, shift, _ = _archive(seed=seed)
        d = np.ascontiguousarray(synth.fractional_delays(shift, NBIN) + extra)
        arcs[name] = (raw, w0, np.zeros(NCHAN, np.int32), d)
    arcs["D"] = arcs["A"][:3] + (np.ascontiguousarray(synth.per_profile_delays(shift, NBIN, NSUB) + 7.0),)
    want = {n: hb.repair_cube(a[0], a[1], HOT, delay=a[3])[1] for n, a in arcs.items()}
    # the delays matter: another archive's would move the window and change the counts
    assert not np.array_equal(want["A"]["count"], hb.repair_cube(arcs["A"][0], arcs["A"][1], HOT,
                                                                 delay=arcs["B"][3])[1]["count"])

    def check(out, name):
        got = out["hotbins"]
        assert np.array_equal(got["count"], want[name]["count"]), name
        assert bits_equal(got["bins"], want[name]["bins"]) and got["total"] == want[name]["total"] > 0, name

    with _native.GpuSession(NSUB, NCHAN, NBIN, device=0, dedisp_fft=True, hotbins=HOT) as s:
        for first, second in ("AB", "BC", "AD", "DB", "CA"):
            s.upload_async(*arcs[first])
            check(s.run(), first)
            s.upload_async(*arcs[first][:3])
            s.upload_async(*arcs[second])
            check(s.run(), first)
            check(s.run(), second)


def test_switched_on_after_a_run_starts_with_the_next_upload():
    from iterative_cleaner_amd import _native
    from iterative_cleaner_amd import hotbins as hb
    raw, w0, shift, _ = _archive()
    with _native.GpuSession(NSUB, NCHAN, NBIN, device=0) as s:
        s.set_timing(True)
        s.upload(raw, w0, shift)
        a = s.run()
        s.set_hotbins(*HOT)
        b = s.run()                                   # the upload already read: left alone
        assert s.kernel_times()["k_hotbins"]["launches"] == 0 and bits_equal(a["weights"], b["weights"])
        assert "hotbins" not in b
        with pytest.raises(_native.NativeError, match="no run"):
            s.hotbins()
        s.upload(raw, w0, shift)
        c = s.run()
        assert s.kernel_times()["k_hotbins"]["launches"] == 1
        assert np.array_equal(c["hotbins"]["count"], hb.repair_cube(raw, w0, HOT, shift=shift)[1]["count"])
    # set between the upload and its first run: that upload gets the pass
    with _native.GpuSession(NSUB, NCHAN, NBIN, device=0) as s:
        s.upload(raw, w0, shift)
        s.set_hotbins(*HOT)
        assert s.run()["hotbins"]["total"] == c["hotbins"]["total"]


def test_state_and_argument_errors():
    """IC_ESTATE and IC_EINVAL of the four calls."""
    from iterative_cleaner_amd import _native
    EINVAL, ESTATE = -1, -4
    with _native.GpuSession(2, 4, 64, device=0) as s:
        lib = s.lib
        total = C.c_int64()
        assert lib.ic_get_hotbins(s.h, None, C.byref(total)) == ESTATE          # off
        assert lib.ic_get_hotbin_list(s.h, None, 0) == ESTATE
        for thr, a, b, r in ((float("nan"), 0, 0, 4), (float("inf"), 0, 0, 4), (3.0, -1, 4, 4), (3.0, 64, 4, 4),
                             (3.0, 0, 65, 4), (3.0, 0, -1, 4), (3.0, 0, 0, 0), (3.0, 0, 0, 9), (3.0, 0, 57, 4),
                             (3.0, 60, 59, 4)):
            assert lib.ic_set_hotbins(s.h, thr, a, b, r) == EINVAL, (thr, a, b, r)
        assert lib.ic_set_hotbins(s.h, 3.0, 0, 56, 4) == 0                      # 8 off-pulse bins: the fewest
        assert lib.ic_get_hotbins(s.h, None, C.byref(total)) == ESTATE          # on, no run yet
        assert lib.ic_set_hotbins(s.h, 0.0, -7, 999, 99) == 0                   # off ignores the rest
        assert lib.ic_set_hotbins(s.h, -1.0, 0, 0, 4) == 0
        s.set_hotbins(3.0, 10, 20)
        x = np.zeros((2, 4, 64), np.float32)
        x[:, :, ::2] += 1.0                       # deviations all 0.5: nothing stands out
        s.upload(x, np.ones((2, 4), np.float32), np.zeros(4, np.int64))
        s.run()
        assert lib.ic_get_hotbins(s.h, None, C.byref(total)) == 0 and total.value == 0
        assert lib.ic_get_hotbin_list(s.h, None, 0) == 0
        assert lib.ic_get_hotbin_list(s.h, None, -1) == EINVAL
    # fractional delays widen the window: 8 off-pulse bins as given are 6
    with _native.GpuSession(2, 4, 64, device=0, delay=np.zeros(4)) as s:
        assert s.lib.ic_set_hotbins(s.h, 3.0, 0, 56, 4) == EINVAL
        assert s.lib.ic_set_hotbins(s.h, 3.0, 0, 54, 4) == 0
    X, w, offs, _ = hc.profiles(64)
    with pytest.raises(_native.NativeError, match="off-pulse"):
        _native.hotbins_profiles(X, w, offs, 1, 3.0, 0, 55, 4)
    with pytest.raises(_native.NativeError, match="nbin above"):
        _native.hotbins_profiles(np.zeros((1, 8200), np.float32), [1], None, 0, 3.0, 0, 0, 4)
    # a list buffer that is too small
    lib = _native.load_library()
    out, count, bins = _native.hotbins_profiles(X, w, offs, 0, 4.0, 16, 24, 4)
    assert bins.shape[0] > 1
    small = np.empty(1, np.int32)
    cnt = np.empty(hc.NPROF, np.int32)
    total = C.c_int64()
    rc = lib.ic_hotbins_profiles(0, hc.NPROF, 64, C.c_void_p(X.ctypes.data), C.c_void_p(w.ctypes.data),
                                 C.c_void_p(offs.ctypes.data), 0, 4.0, 16, 24, 4, None, C.c_void_p(cnt.ctypes.data), C.c_void_p(small.ctypes.data), 1,
                                 C.byref(total))
    assert rc == EINVAL and total.value == bins.shape[0] and np.array_equal(cnt, count)


# ---------------------------------------------------------------- 3. shards and the batch scheduler

def test_shards_equal_one_session():
    """An in-process group of world 2 at 4 x 512 x 64 equals one session:
    weights, counts and lists (each rank treats its own channels)."""
    from iterative_cleaner_amd import _native, synth
    nsub, nchan, nbin = 4, 512, 64
    hot = (5.0, 14, 25)
    data, w0, shift = synth.make_cube(nsub, nchan, nbin, 11, 0.05)
    raw = np.ascontiguousarray(data[:, 0])
    rng = np.random.default_rng(12)
    for k in range(0, nsub * nchan, 5):
        s, c = divmod(k, nchan)
        off = hc.off_bins(nbin, int(shift[c]), 13, 26)
        raw[s, c, rng.choice(off, size=2, replace=False)] += np.float32(35.0)
    one = _gpu_clean(raw, w0, shift, hotbins=hot)
    assert one["hotbins"]["total"] > 100
    world = 2
    outs = [None] * world
    errs = []
    with _native.ShardGroup(world) as group:
        def work(rank):
            try:
                with _native.ShardSession(nsub, nchan, nbin, rank, world, group=group, device=0, hotbins=hot) as s:
                    c0, c1 = s.chan_range
                    s.upload(np.ascontiguousarray(raw[:, c0:c1]), np.ascontiguousarray(w0[:, c0:c1]), shift[c0:c1])
                    outs[rank] = (s.run(), (c0, c1))
            except Exception as e:   # pragma: no cover
                errs.append(e)
        threads = [threading.Thread(target=work, args=(r,)) for r in range(world)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    assert not errs, errs
    from iterative_cleaner_amd import hotbins as hb
    weights = np.concatenate([o["weights"] for o, _ in outs], axis=1)
    merged = hb.merge_shards([o["hotbins"] for o, _ in outs])
    assert bits_equal(weights, one["weights"]) and outs[0][0]["loops"] == one["loops"]
    for key in ("count", "bins", "offsets"):
        assert bits_equal(merged[key], one["hotbins"][key]), key
    assert merged["total"] == one["hotbins"]["total"]


def test_batch_equals_single_sessions():
    """clean_batch(..., hotbins=...) over three archives, one with spikes,
    equals single sessions."""
    from iterative_cleaner_amd import batch
    cubes = [_archive(seed=21, spikes=False), _archive(seed=22, spikes=True), _archive(seed=23, spikes=False)]
    outs = list(batch.clean_batch([c[:3] for c in cubes], (NSUB, NCHAN, NBIN), hotbins=HOT))
    assert len(outs) == 3
    for out, (raw, w0, shift, _) in zip(outs, cubes):
        one = _gpu_clean(raw, w0, shift, hotbins=HOT)
        assert bits_equal(out["weights"], one["weights"]) and out["loops"] == one["loops"]
        for key in ("count", "bins", "offsets"):
            assert bits_equal(out["hotbins"][key], one["hotbins"][key]), key
    assert outs[1]["hotbins"]["total"] > 20 and outs[0]["hotbins"]["total"] <= 2
