"""The opt-in modes together on the GPU, against the composed CPU yardstick
(compose_ref.clean): hot-bin repair, a standard template and detrended scaling
(whole lines, pieces, shards) in one session, with every output of the chain
compared - the hit list, the alignment, the installed template, the fit, the
diagnostics, the test values, the weights and loop records, and the residuals
(f32 and PSRFITS int16) that subtract amp x the INSTALLED template from the
REPAIRED cube.  No comparison here is against another GPU run unless it says
"equals one session".  test_compose_host.py pins the yardstick and the
conditions that make each case mean something; the tolerance on detrended test
values is the one measured there (compose_ref.TOL_DETREND)."""
import os

import numpy as np
import pytest

import compose_ref as cr
from helpers import bits_equal, bits_equal_nan

pytestmark = pytest.mark.gpu


def _session_kw(name, max_iter=None):
    """GpuSession's keywords of a composed case."""
    c, inp = cr.CASES[name], cr.case_inputs(name)
    ck = c["clean_kw"]
    kw = dict(max_iter=ck.get("max_iter", 5) if max_iter is None else max_iter, device=0,
              fit_mode=ck.get("fit_mode", 0), data_f64=ck.get("data_f64", False), delay=inp["delay"],
              input_dedispersed=inp["ded"], detrend=c["detrend"], detrend_pieces=c["pieces"],
              std_template=(inp["S"], c["std"]) if c["std"] else None, hotbins=inp["hot"])
    if "pulse_region" in ck:
        kw["pulse_region"] = list(ck["pulse_region"])
    return kw


def _upload(s, name):
    c, inp = cr.CASES[name], cr.case_inputs(name)
    if c["upload"] == "quantised":
        s.upload_quantised(*inp["quantised"], inp["w0"], inp["shift"], 1)
    elif c["upload"] == "pols":
        s.upload_pols(inp["pols"], inp["w0"], inp["shift"])
    else:
        s.upload(inp["raw"], inp["w0"], inp["shift"])


def _details(s, out, residuals=False):
    """Everything a session holds after run(), into its result."""
    out["T"] = s.template()
    out["amp"], out["info"] = s.fit()
    out["std"], out["mean"], out["ptp"], out["fft"] = s.diagnostics()
    if residuals:
        out["residual"] = s.residual()
        out["residual_q"] = s.residual_quantised()
        out["residual_q_be"] = s.residual_quantised(big_endian=True)
    return out


def _gpu(name, options=None, residuals=False):
    c = cr.CASES[name]
    from iterative_cleaner_amd import _native
    with _native.GpuSession(c["nsub"], c["nchan"], c["nbin"], options=options, **_session_kw(name)) as s:
        _upload(s, name)
        return _details(s, s.run(), residuals)


def _same_hotbins(got, want, what):
    for key in ("count", "bins", "offsets"):
        assert bits_equal(got[key], want[key]), "%s: hotbins %s" % (what, key)
    assert got["total"] == want["total"], what


def _same_quantised(got, residual, big_endian, what):
    """(q, scl, offs) of the GPU against psrfits.quantise of the yardstick's residual."""
    from iterative_cleaner_amd import psrfits
    q, scl, offs = psrfits.quantise(residual[:, None])
    assert got[0].dtype == np.dtype(">i2" if big_endian else np.int16), what
    assert bits_equal(got[0], q[:, 0].astype(got[0].dtype)), "%s: int16 samples" % what
    assert bits_equal(got[1], scl[:, 0]) and bits_equal(got[2], offs[:, 0]), "%s: scales and offsets" % what


def _check(out, ref, name, tol, what=None):
    """One GPU run against the yardstick, output by output."""
    what = what or name
    if "hotbins" in ref:
        _same_hotbins(out["hotbins"], ref["hotbins"], what)
    else:
        assert "hotbins" not in out, what
    if "std_alignment" in ref:
        assert out["std_alignment"] == ref["std_alignment"], "%s: alignment %s != %s" % (
            what, out["std_alignment"], ref["std_alignment"])
    else:
        assert "std_alignment" not in out, what
    assert out["loops"] == ref["loops"] and out["n_iter"] == ref["n_iter"], "%s: loops %d/%d, n_iter %d/%d" % (
        what, out["loops"], ref["loops"], out["n_iter"], ref["n_iter"])
    assert np.array_equal(out["changed"], ref["changed"]) and np.array_equal(out["nzero"], ref["nzero"]), what
    assert bits_equal(out["weights"], ref["weights"]), "%s: %d weights differ" % (
        what, int((out["weights"] != ref["weights"]).sum()))
    t, u = out["test"], ref["test"]
    with np.errstate(invalid="ignore"):
        near = (t == u) | (np.abs(t - u) <= tol) | (np.isnan(t) & np.isnan(u))
    print("%s: largest |test - yardstick| %.3g (tolerance %.3g)" % (what, float(np.nanmax(np.abs(t - u))), tol))
    assert np.all(near), "%s: test values differ by up to %.3g > %.3g" % (what, float(np.nanmax(np.abs(t - u))), tol)
    if "T" in out:
        assert bits_equal(out["T"], ref["T"]), "%s: template" % what
        assert bits_equal(out["amp"], ref["amp"]), "%s: %d amplitudes differ" % (
            what, int((out["amp"] != ref["amp"]).sum()))
        assert bits_equal(out["info"], ref["info"]), "%s: fit status" % what
        for key in ("std", "mean", "ptp"):
            assert bits_equal_nan(out[key], ref[key]), "%s: %s" % (what, key)
        g, f = out["fft"], ref["fft"]
        with np.errstate(invalid="ignore"):
            assert np.all((g == f) | (np.abs(g - f) <= 1e-9 * np.abs(f)) | (np.isnan(g) & np.isnan(f))), \
                "%s: fftmax" % what
    if "residual" in out:
        assert bits_equal(out["residual"], ref["residual"]), "%s: residual (%d samples differ)" % (
            what, int((out["residual"] != ref["residual"]).sum()))
        _same_quantised(out["residual_q"], ref["residual"], False, what)
        _same_quantised(out["residual_q_be"], ref["residual"], True, what)


# ---------------------------------------------------------------- a - e. sessions against the yardstick

# e: the fused k_residual_q (integer shifts), the rotate-then-encode path (delays) and the long rows
RESIDUALS = ("a-int-128-int", "a-int-128-frac", "a-chan-128-int", "a-chan-128-frac", "a-prof-1024-int",
             "a-prof-1024-frac", "a-int-2048-int", "a-int-2048-frac")


@pytest.mark.parametrize("name", [n for n in sorted(cr.CASES) if n[0] in "abcd"])
def test_session_equals_the_yardstick(name):
    """a: hot bins, standard (int and frac) and detrend (1, 2) in one session of
    max_iter 5, at every statistics kernel's length and in every dedispersion
    mode; b: the variants at 128 bins (closed fit, data_f64, a pulse region over
    the hot-bin window, quantised and full-polarisation uploads, pieces at 6 x
    32); c: pairs without a standard over three iterations, every iteration's
    counts and the last iteration in full; d: standard, detrending and pieces
    without hot bins; e (RESIDUALS): the residuals under the modes."""
    assert set(RESIDUALS) <= set(cr.CASES)
    out = _gpu(name, residuals=name in RESIDUALS)
    _check(out, cr.reference(name), name, cr.tolerance(name))


@pytest.mark.parametrize("options", [{"fit_tiled": 0}, {"fit_tiled": 1}, {"grid_cap": 1}],
                         ids=lambda o: "%s=%d" % next(iter(o.items())))
def test_schedule_options_keep_the_yardstick(options):
    """b: fit_tiled 0 and 1, and grid_cap = 1 (one block walks every grid-stride
    loop of the chain), residuals included."""
    name = "a-int-128-frac"
    out = _gpu(name, options=options, residuals=True)
    _check(out, cr.reference(name), name, cr.tolerance(name), "%s, %s" % (name, options))


@pytest.mark.parametrize("lanes", [1, 2])
def test_batch_residuals_equal_the_yardstick(lanes):
    """e: clean_batch(hotbins=, std_template=, detrend=, residuals=True) over
    three archives, one without spikes: each item's residual_q, weights,
    hotbins and std_alignment are the yardstick's for that archive."""
    from iterative_cleaner_amd import batch
    arcs = cr.batch_archives()
    n = 0
    for out, (raw, w0, shift, ref) in zip(
            batch.clean_batch([a[:3] for a in arcs], (6, 16, 128), lanes=lanes, hotbins=cr.hot_window(128),
                              std_template=(cr.standard(128), cr.BATCH_STD), detrend=cr.DETREND, residuals=True),
            arcs):
        what = "archive %d, %d lanes" % (n, lanes)
        _same_quantised(tuple(np.array(a) for a in out["residual_q"]), ref["residual"], True, what)
        assert bits_equal(out["weights"], ref["weights"]) and out["loops"] == ref["loops"], what
        _same_hotbins(out["hotbins"], ref["hotbins"], what)
        assert out["std_alignment"] == ref["std_alignment"], what
        n += 1
    assert n == 3
    assert arcs[1][3]["hotbins"]["total"] < arcs[0][3]["hotbins"]["total"]     # the archive without spikes


# ---------------------------------------------------------------- f. session life cycle

def _launches(s):
    return {k: v["launches"] for k, v in s.kernel_times().items()}


def test_second_run_repeats_and_repairs_nothing_again():
    from iterative_cleaner_amd import _native
    name = "a-int-128-frac"
    c, ref = cr.CASES[name], cr.reference(name)
    with _native.GpuSession(c["nsub"], c["nchan"], c["nbin"], **_session_kw(name)) as s:
        s.set_timing(True)
        _upload(s, name)
        first = _details(s, s.run(), residuals=True)
        assert _launches(s)["k_hotbins"] == 1
        second = _details(s, s.run(), residuals=True)
        assert _launches(s)["k_hotbins"] == 1, "the second run repaired the repaired cube again"
    for out, what in ((first, "first run"), (second, "second run")):
        _check(out, ref, name, cr.tolerance(name), what)
    for key in ("test", "fft"):
        assert bits_equal_nan(first[key], second[key]), key


def test_queued_uploads_get_their_own_repair_and_alignment():
    """Two archives queued with upload_async on one FFT session, the second
    bringing per-profile delays of its own: each run equals the yardstick of
    its archive (its own hit list, its own alignment, its own residual)."""
    from iterative_cleaner_amd import _native
    first, second = "a-chan-128-frac", "a-prof-128-frac"
    a, b = cr.case_inputs(first), cr.case_inputs(second, cr.QUEUED_SEED)
    assert a["delay"].ndim == 1 and b["delay"].ndim == 2
    ra, rb = cr.reference(first), cr.reference(second, cr.QUEUED_SEED)
    assert ra["std_alignment"] != rb["std_alignment"] and not bits_equal(ra["hotbins"]["bins"], rb["hotbins"]["bins"])
    kw = _session_kw(first)
    with _native.GpuSession(6, 16, 128, **kw) as s:
        s.upload_async(a["raw"], a["w0"], a["shift"])
        s.upload_async(b["raw"], b["w0"], b["shift"], delay=b["delay"])
        _check(_details(s, s.run(), residuals=True), ra, first, cr.tolerance(first))
        _check(_details(s, s.run(), residuals=True), rb, second, cr.tolerance(second))


def test_set_then_cleared_is_never_set():
    """All three modes (and pieces) set and then cleared: the bits and the
    per-kernel launch counts of a session that never set them."""
    from iterative_cleaner_amd import _native
    name = "a-int-128-frac"
    inp = cr.case_inputs(name)

    def run(cleared):
        with _native.GpuSession(6, 16, 128, device=0) as s:
            if cleared:
                s.set_hotbins(*inp["hot"])
                s.set_std_template(inp["S"], "frac")
                s.set_detrend(*cr.DETREND)
                s.set_detrend_pieces(None, "w8")
                s.clear_hotbins()
                s.clear_std_template()
                s.set_detrend_pieces(None, None)
                s.set_detrend(0, 0)
            s.set_timing(True)
            s.upload(inp["raw"], inp["w0"], inp["shift"])
            out = _details(s, s.run(), residuals=True)
            out["launches"] = _launches(s)
        return out

    never, cleared = run(False), run(True)
    assert never["launches"] == cleared["launches"] and never["launches"]["k_hotbins"] == 0
    assert "hotbins" not in cleared and "std_alignment" not in cleared
    assert never["loops"] == cleared["loops"] and never["n_iter"] == cleared["n_iter"]
    for key in ("weights", "test", "changed", "nzero", "T", "amp", "info", "std", "mean", "ptp", "fft", "residual"):
        assert bits_equal_nan(never[key], cleared[key]), key
    for k in range(3):
        assert bits_equal(never["residual_q"][k], cleared["residual_q"][k])
    # and that session is the plain loop of the yardstick
    _check(never, cr.reference(name, hotbins=None, std=None, detrend=None), name, cr.TOL_PLAIN, "never set")


# ---------------------------------------------------------------- g. shards

def test_shards_equal_one_session_that_equals_the_yardstick():
    """An in-process group of two channel shards at 4 x 512 x 64 with hot bins,
    the standard (int), detrend (1, 2) under shard_detrend and subint pieces
    equals one session bit for bit: weights, the merged hit list
    (hotbins.merge_shards), the alignment and the trends.  The one session is
    held to the yardstick at 4 x 64 x 64 (case g-4x64x64, an archive of its
    own): the Python side of the yardstick at 512 channels is left out as too
    slow for a test, so shards are not pinned to the yardstick at the shards'
    own shape."""
    from iterative_cleaner_amd import _native, sharded
    name = "g-4x64x64"
    _check(_gpu(name), cr.reference(name), name, cr.tolerance(name))
    raw, w0, shift, _ = cr.shard_archive(512)
    kw = dict(hotbins=cr.hot_window(64), std_template=(cr.standard(64), "int"), detrend=cr.DETREND,
              detrend_pieces=(None, "w16"))
    with _native.GpuSession(4, 512, 64, device=0, **kw) as s:
        s.upload(raw, w0, shift)
        one = _details(s, s.run())
        one["trend_chan"], one["trend_subint"] = s.trends()
    assert one["hotbins"]["total"] > 100 and one["std_alignment"]["lag"] != 0
    assert (one["weights"][w0 != 0] == 0).any() and (one["weights"] != 0).any()
    out = sharded.clean_cube_local(raw, w0, shift, 2, want_details=True, shard_detrend=True, **kw)
    assert out["loops"] == one["loops"] and out["n_iter"] == one["n_iter"]
    assert out["std_alignment"] == one["std_alignment"]
    _same_hotbins(out["hotbins"], one["hotbins"], "shards")
    for key in ("weights", "test", "T", "amp", "info", "std", "mean", "ptp", "fft", "trend_chan", "trend_subint"):
        assert bits_equal_nan(out[key], one[key]), key


# ---------------------------------------------------------------- h. end to end

def test_cli_clean_with_the_three_switches(tmp_path, monkeypatch, capsys):
    """clean() on a PSRFITS stand-in archive with IC_HOTBINS, IC_STD_TEMPLATE (a
    .npy written here) and IC_DETREND set, -u -p: the output archive's weights
    are the yardstick's, its samples are patched at the yardstick's bins, and
    the residual it writes is the yardstick's residual."""
    from iterative_cleaner_amd import archive as ica
    from iterative_cleaner_amd import cleaner, psrfits
    name = "a-int-128-int"
    inp = cr.case_inputs(name)
    monkeypatch.chdir(tmp_path)
    half = (inp["raw"] * np.float32(0.5)).astype(np.float32)
    data = np.ascontiguousarray(np.stack([half, (inp["raw"] - half).astype(np.float32)], axis=1))
    ica.Archive(data, inp["w0"].copy(), inp["shift"].astype(np.int64), filename="obs.sf").unload("obs.sf")
    src = ica.Archive_load("obs.sf")
    dec = src.get_data()
    cube = (dec[:, 0] + dec[:, 1]).astype(np.float32)          # archive.py pscrunch
    thr, a, b = inp["hot"]
    ref = cr.clean(cube, src.get_weights(), src.get_dm_shift(), hotbins=inp["hot"], std=(inp["S"], "int"),
                   detrend=cr.DETREND)
    assert ref["hotbins"]["total"] > 0 and ref["std_alignment"]["lag"] != 0
    assert np.min(np.abs(ref["test"][np.isfinite(ref["test"])] - 1.0)) > 100 * cr.TOL_DETREND
    np.save("std.npy", inp["S"])
    monkeypatch.setenv("IC_HOTBINS", "%r,%d,%d" % (thr, a, b))
    monkeypatch.setenv("IC_STD_TEMPLATE", "std.npy,int")
    monkeypatch.setenv("IC_DETREND", "%d,%d" % cr.DETREND)
    cleaner.main(cleaner.parse_arguments(["-l", "-q", "-u", "-p", "obs.sf"]))
    capsys.readouterr()
    res = ica.Archive_load("obs_cleaned.ar")
    assert bits_equal(res.get_weights(), ref["weights"])
    assert res.get_npol() == 1
    got = res.get_data()[:, 0]
    # the samples are the repaired cube's, re-quantised on unload: within half a step (a little more, for the
    # rounding of the f32 scale) of it everywhere, and at the repaired bins far from what the archive held
    q, scl, offs = psrfits.quantise(ref["cube"][:, None])
    assert np.all(np.abs(got - ref["cube"]) <= 0.51 * scl[:, 0][:, :, None])
    hot = np.zeros(cube.shape, bool)
    rows = ref["hotbins"]["offsets"]
    for k in np.nonzero(ref["hotbins"]["count"].reshape(-1) > 0)[0]:
        hot[k // 16, k % 16, ref["hotbins"]["bins"][rows[k]:rows[k + 1]]] = True
    assert hot.sum() == ref["hotbins"]["total"] and np.all(np.abs(got[hot] - cube[hot]) > 10.0)
    assert np.all(np.abs(got[~hot] - cube[~hot]) <= 1.02 * scl[:, 0][:, :, None].repeat(128, axis=2)[~hot])
    resid = [p for p in os.listdir(".") if "_residual_" in p]
    assert resid == ["obs.sf_residual_%d.ar" % ref["loops"]]
    r = psrfits.load_quantised(resid[0])
    want = psrfits.quantise(ref["residual"][:, None])
    assert bits_equal(np.asarray(r[0]).astype(np.int16), want[0]) and bits_equal(np.asarray(r[1]), want[1])
    assert bits_equal(np.asarray(r[2]), want[2])
