"""The dynamic spectrum on the GPU: k_dynspec against the written definition
(dynspec.py) bit for bit (a NaN equals any NaN): the one-shot, sessions in
every mode ic_run serves, the opt-in modes, the grid cap, repeated calls, the
feature unused, channel shards and the batch scheduler."""
import numpy as np
import pytest

import dynspec_cases as dc
from helpers import bits_equal, bits_equal_nan

pytestmark = pytest.mark.gpu

F = np.float32
ESTATE = -4


# ---------------------------------------------------------------- 1. the one-shot

@pytest.mark.parametrize("nbin", dc.ONESHOT_NBINS)
def test_oneshot_equals_the_module(nbin):
    """ic_dynspec_profiles against dynspec.profiles for 1, 5 and 67 profiles
    (the last block partly filled): lanes without an element (4, 16, 63), uneven
    chains (65, 100), whole chains and the long-row plans (4096, 8192)."""
    from iterative_cleaner_amd import _native
    for nprof in dc.ONESHOT_NPROFS:
        T, X, w, _, _ = dc.profiles(nbin, nprof)
        assert dc.same(_native.dynspec_profiles(T, X, w), dc.module_profiles(nbin, nprof),
                       "nbin %d, %d profiles" % (nbin, nprof))


@pytest.mark.parametrize("nbin", (100, 1024, 4096))
def test_oneshot_masked_nan_row_and_inf(nbin):
    """A w = 0 row of NaNs gives zeros (the row is not read), a live row with an
    Inf gives what IEEE gives."""
    from iterative_cleaner_amd import _native
    from iterative_cleaner_amd import dynspec as ds
    T, X, w = dc.edge_profiles(nbin)
    got = _native.dynspec_profiles(T, X, w)
    assert dc.same(got, ds.profiles(T, X, w), "nbin %d" % nbin)
    for key in ("amp", "err", "base"):
        assert got[key][1] == 0 and not np.signbit(got[key][1]) and got[key][4] == 0 and not np.isfinite(got[key][2])


def test_oneshot_rows_beyond_the_register_plan():
    """8256 bins: k_dynspec_long reads the row twice; the same chains."""
    from iterative_cleaner_amd import _native
    T, X, w, _, _ = dc.profiles(8256, 5)
    assert dc.same(_native.dynspec_profiles(T, X, w), dc.module_profiles(8256, 5))


def test_oneshot_constant_template_and_refusals():
    from iterative_cleaner_amd import _native
    from iterative_cleaner_amd import dynspec as ds
    _, X, w, _, _ = dc.profiles(64, 5)
    flat = np.full(64, 1.5, F)
    got = _native.dynspec_profiles(flat, X, w)
    assert dc.same(got, ds.profiles(flat, X, w)) and np.all(np.isnan(got["amp"]))      # Stt == 0
    with pytest.raises(_native.NativeError, match="nbin=3"):
        _native.dynspec_profiles(flat[:3], X[:, :3], w)
    with pytest.raises(ValueError, match="template must be"):
        _native.dynspec_profiles(flat[:32], X, w)
    with pytest.raises(ValueError, match="weights"):
        _native.dynspec_profiles(flat, X, w[:2])


# ---------------------------------------------------------------- 2. sessions

SHAPES = ((4, 64), (3, 5))


def _delays(kind, shift, nbin, nsub):
    from iterative_cleaner_amd import synth
    if kind is None:
        return None
    return synth.fractional_delays(shift, nbin) if kind == "chan" else synth.per_profile_delays(shift, nbin, nsub)


def _run(raw, w0, shift, upload="plain", calls=1, **kw):
    """One session: (run dict, template, [dynspec of each call])."""
    from iterative_cleaner_amd import _native, psrfits
    nsub, nchan, nbin = raw.shape
    with _native.GpuSession(nsub, nchan, nbin, device=0, **kw) as s:
        if upload == "quantised":
            q, scl, offs = psrfits.quantise(raw[:, None])
            s.upload_quantised(q, scl, offs, w0, shift, 1)
        else:
            s.upload(raw, w0, shift)
        out = s.run()
        assert out["n_iter"] > 0
        dyn = [s.dynspec() for _ in range(calls)]
        return out, s.template(), dyn


def _check_session(nsub, nchan, nbin, delay=None, upload="plain", seed=5, **kw):
    """The session's dynamic spectrum equals dynspec.cube of the cube it consumed,
    its own template() and its own final weights."""
    from iterative_cleaner_amd import dynspec as ds
    from iterative_cleaner_amd import psrfits
    raw, w0, shift = dc.archive(nsub, nchan, nbin, seed)
    d = _delays(delay, shift, nbin, nsub)
    out, T, (dyn,) = _run(raw, w0, shift, upload=upload, delay=d, **kw)
    cube = raw if upload == "plain" else psrfits.decode(*psrfits.quantise(raw[:, None]))[:, 0]
    want = ds.cube(cube, T, out["weights"], shift=shift, delay=d, input_dedispersed=kw.get("input_dedispersed", False),
                   any_length=kw.get("any_length"))
    what = "%dx%dx%d %s %s" % (nsub, nchan, nbin, delay, sorted(kw))
    assert dc.same(dyn, want, what)
    zapped = out["weights"] == 0
    assert zapped.any() and not zapped.all(), what
    for key in ("amp", "err", "base"):
        assert np.all(dyn[key][zapped] == 0) and np.all(np.isfinite(dyn[key][~zapped])), (what, key)
    assert np.all(dyn["err"][~zapped] > 0)
    return out, dyn


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("nbin", (64, 100, 1024, 8192))
def test_session_integer_shifts(shape, nbin):
    _check_session(*shape, nbin)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("nbin", (64, 1024))
@pytest.mark.parametrize("mode", ("chan", "prof", "stored"))
def test_session_fft_delays(shape, nbin, mode):
    """IC_DEDISP_FFT per channel, per profile, and with input_dedispersed."""
    if mode == "stored":
        _check_session(*shape, nbin, delay="chan", input_dedispersed=True)
    else:
        _check_session(*shape, nbin, delay=mode)


@pytest.mark.parametrize("shape", SHAPES)
def test_session_mixed_radix_1000(shape):
    _check_session(*shape, 1000, delay="chan")


@pytest.mark.parametrize("shape", SHAPES)
def test_session_fft_any_100(shape):
    _check_session(*shape, 100, delay="chan", any_length=True)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kw", (dict(fit_mode=1), dict(data_f64=True), dict(upload="quantised"),
                                dict(fit_mode=1, delay="chan")), ids=lambda k: "-".join(sorted(k)))
def test_session_other_modes_at_64(shape, kw):
    """IC_FIT_CLOSED (also with FFT delays), data_f64 and a quantised upload."""
    _check_session(*shape, 64, **kw)


HOT = (5.0, 14, 25)          # the synthetic pulse sits at phase 0.3: bin 19 of 64
MODES = {
    "std": dict(std=True),
    "hot": dict(hot=True),
    "detrend": dict(detrend=(1, 1)),
    "all": dict(std=True, hot=True, detrend=(1, 1)),
    "all, FFT delays": dict(std=True, hot=True, detrend=(1, 1), delay="chan"),
}


@pytest.mark.parametrize("name", sorted(MODES))
def test_session_opt_in_modes(name):
    """Standard template, hot bins and detrending at 4 x 64 x 64, one at a time
    and together: the GPU's own template() (the aligned standard) and weights,
    and the cube hotbins.py repairs, feed dynspec.cube."""
    from iterative_cleaner_amd import dynspec as ds
    from iterative_cleaner_amd import hotbins as hb
    m = dict(MODES[name])
    nsub, nchan, nbin = 4, 64, 64
    raw, w0, shift = dc.archive(nsub, nchan, nbin, seed=8)
    for k in range(0, nsub * nchan, 9):                     # spikes for the repair to find
        s, c = divmod(k, nchan)
        raw[s, c, (int(shift[c]) + 40 + k % 7) % nbin] += F(45.0)
    d = _delays(m.pop("delay", None), shift, nbin, nsub)
    kw = {}
    if m.pop("std", False):
        kw["std_template"] = np.roll(dc.template(nbin, seed=3), 5)
    hot = m.pop("hot", False)
    if hot:
        kw["hotbins"] = HOT
    kw.update(m)
    out, T, (dyn,) = _run(raw, w0, shift, delay=d, **kw)
    cube = raw
    if hot:
        cube, res = hb.repair_cube(raw, w0, HOT, shift=shift, delay=d)
        assert res["total"] > 5 and np.array_equal(out["hotbins"]["count"], res["count"])
    if "std_template" in kw:
        assert not bits_equal(T, kw["std_template"]) and out["std_alignment"]["aligned"] == 1
    assert dc.same(dyn, ds.cube(cube, T, out["weights"], shift=shift, delay=d), name)
    assert (out["weights"] == 0).any()


@pytest.mark.parametrize("nbin,delay", ((64, None), (100, None), (1024, None), (4096, None), (1024, "chan")))
def test_grid_cap_gives_the_same_bits(nbin, delay):
    """IC_OPT_GRID_CAP = 1 and = 3: a few blocks walk every profile in many
    trips of the grid-stride loop; the bits of the default grid."""
    raw, w0, shift = dc.archive(3, 20, nbin, seed=6)
    d = _delays(delay, shift, nbin, 3)
    ref_out, _, (ref,) = _run(raw, w0, shift, delay=d, fit_mode=1)
    for cap in (1, 3):
        out, _, (dyn,) = _run(raw, w0, shift, delay=d, fit_mode=1, options={"grid_cap": cap})
        assert bits_equal(out["weights"], ref_out["weights"])
        assert dc.same(dyn, ref, "grid_cap %d" % cap)


def test_repeated_calls_and_second_run():
    """Two calls in a row give the same arrays, and so does a call after a
    second run(); before the first run the call is IC_ESTATE, and again after
    a new upload until that one has run."""
    from iterative_cleaner_amd import _native
    from iterative_cleaner_amd import dynspec as ds
    raw, w0, shift = dc.archive(4, 64, 64)
    raw2, w02, shift2 = dc.archive(4, 64, 64, seed=12)
    with _native.GpuSession(4, 64, 64, device=0) as s:
        amp = np.empty((4, 64))
        assert s.lib.ic_get_dynspec(s.h, None, None, None) == ESTATE
        with pytest.raises(_native.NativeError, match="no completed iteration"):
            s.dynspec()
        s.upload(raw, w0, shift)
        assert s.lib.ic_get_dynspec(s.h, C_ptr(amp), None, None) == ESTATE
        a = s.run()
        one, two = s.dynspec(), s.dynspec()
        assert dc.same(one, two)
        b = s.run()
        assert bits_equal(a["weights"], b["weights"]) and dc.same(s.dynspec(), one)
        # any of the three may be NULL
        assert s.lib.ic_get_dynspec(s.h, None, None, C_ptr(amp)) == 0 and bits_equal_nan(amp, one["base"])
        assert s.lib.ic_get_dynspec(s.h, None, None, None) == 0
        s.upload(raw2, w02, shift2)
        assert s.lib.ic_get_dynspec(s.h, None, None, None) == ESTATE
        c = s.run()
        assert dc.same(s.dynspec(), ds.cube(raw2, s.template(), c["weights"], shift=shift2))


def C_ptr(a):
    import ctypes
    return ctypes.c_void_p(a.ctypes.data)


def test_nothing_changes_when_unused():
    """A session that runs, calls dynspec() and runs again returns test, weights,
    loop records and residual bit-identical to a session that never calls it,
    whose k_dynspec launch count is 0."""
    from iterative_cleaner_amd import _native
    raw, w0, shift = dc.archive(4, 64, 64)

    def run(use):
        res = []
        with _native.GpuSession(4, 64, 64, device=0) as s:
            s.set_timing(True)
            s.upload(raw, w0, shift)
            for _ in range(2):
                out = s.run()
                if use:
                    out["dynspec"] = s.dynspec()
                out["residual"] = s.residual()
                res.append(out)
            kt = {k: v["launches"] for k, v in s.kernel_times().items()}
        return res, kt

    (u1, u2), kt_used = run(True)
    (n1, n2), kt_never = run(False)
    assert kt_never["k_dynspec"] == 0 and kt_used["k_dynspec"] == 2
    assert {k: v for k, v in kt_used.items() if k != "k_dynspec"} == {k: v for k, v in kt_never.items()
                                                                      if k != "k_dynspec"}
    for got, ref in ((u1, n1), (u2, n2), (u2, n1)):
        for key in ("test", "weights", "changed", "nzero", "bad_fits", "residual"):
            assert bits_equal_nan(got[key], ref[key]), key
        assert (got["loops"], got["n_iter"], got["converged"]) == (ref["loops"], ref["n_iter"], ref["converged"])
    assert "dynspec" not in n1


# ---------------------------------------------------------------- 3. shards, the batch scheduler, run_loop

def test_shards_equal_one_session():
    """In-process channel shards, world 2 at 4 x 512 x 64: every shard returns
    its slice, and the merged result equals one session's."""
    from iterative_cleaner_amd import sharded
    raw, w0, shift = dc.archive(4, 512, 64, seed=11, rfi=0.05)
    one_out, _, (one,) = _run(raw, w0, shift)
    got = sharded.clean_cube_local(raw, w0, shift, 2, dynspec=True)
    assert bits_equal(got["weights"], one_out["weights"]) and got["loops"] == one_out["loops"]
    assert got["dynspec"]["amp"].shape == (4, 512) and dc.same(got["dynspec"], one, "world 2")
    assert "dynspec" not in sharded.clean_cube_local(raw, w0, shift, 2)


def test_batch_equals_single_sessions():
    """clean_batch(..., dynspec=True) over three small archives equals three
    single sessions; off, the dicts carry no dynspec."""
    from iterative_cleaner_amd import batch
    cubes = [dc.archive(6, 24, 128, seed=s) for s in (21, 22, 23)]
    outs = list(batch.clean_batch(cubes, (6, 24, 128), dynspec=True))
    assert len(outs) == 3
    for out, (raw, w0, shift) in zip(outs, cubes):
        one_out, _, (one,) = _run(raw, w0, shift)
        assert bits_equal(out["weights"], one_out["weights"]) and dc.same(out["dynspec"], one)
    assert not bits_equal(outs[0]["dynspec"]["amp"], outs[1]["dynspec"]["amp"])
    assert all("dynspec" not in o for o in batch.clean_batch(cubes[:1], (6, 24, 128), dynspec=False))


def test_run_loop_keyword(monkeypatch):
    from iterative_cleaner_amd import cleaner
    monkeypatch.delenv("IC_DYNSPEC", raising=False)
    raw, w0, shift = dc.archive(4, 64, 64)
    args = cleaner.parse_arguments(["-q", "-l", "x.ar"])
    one_out, _, (one,) = _run(raw, w0, shift)
    assert "dynspec" not in cleaner.run_loop(raw, w0, shift, args)
    assert dc.same(cleaner.run_loop(raw, w0, shift, args, dynspec=True)["dynspec"], one)
    monkeypatch.setenv("IC_DYNSPEC", "1")
    assert dc.same(cleaner.run_loop(raw, w0, shift, args)["dynspec"], one)
