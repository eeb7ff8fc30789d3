"""The dynamic spectrum's written definition (iterative_cleaner_amd/dynspec.py)
on the host: against numpy's least squares, the calibration of its error, the
order of its sums, its rules, the switch, the text file, the shard merge and
clean()'s file with the native layer stubbed."""
import inspect
import os
import re

import numpy as np
import pytest

import dynspec_cases as dc
from helpers import bits_equal, bits_equal_nan
from iterative_cleaner_amd import dynspec as ds

F = np.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LSTSQ_NBINS = (16, 64, 100, 256, 1024)
AMP_DEV, BASE_DEV = 5.1e-15, 7.9e-15      # measured (docstring below)


def test_against_numpy_lstsq():
    """dynspec.profiles against numpy.linalg.lstsq on [1, T] in f64, 64 seeded
    profiles at each of 16, 64, 100, 256 and 1024 bins.  The largest relative
    deviations measured on the CPU over these inputs are 5.01e-15 (amp) and
    7.85e-15 (base); 16 x that is allowed: it is the rounding noise of two
    different orders of summation (sum64 against LAPACK's), nothing else."""
    worst_a = worst_b = 0.0
    for nbin in LSTSQ_NBINS:
        T, X, w, _, _ = dc.profiles(nbin, 64)
        got = ds.profiles(T, X, w)
        A = np.stack([np.ones(nbin), T.astype(np.float64)], axis=1)
        sol = np.linalg.lstsq(A, X.astype(np.float64).T, rcond=None)[0]
        worst_a = max(worst_a, float(np.max(np.abs(got["amp"] - sol[1]) / np.abs(sol[1]))))
        worst_b = max(worst_b, float(np.max(np.abs(got["base"] - sol[0]) / np.abs(sol[0]))))
    print("largest relative deviation from lstsq: amp %.3g, base %.3g" % (worst_a, worst_b))
    assert worst_a <= 16 * AMP_DEV and worst_b <= 16 * BASE_DEV


def test_err_is_calibrated():
    """4096 profiles of 256 bins, x = g T + b + N(0, 1) with a Gaussian-pulse T,
    fixed seed: the pulls (amp - g) / err have a mean within +-0.1 and a
    standard deviation within 0.9 .. 1.1 (measured here: 0.025 and 1.002; the
    sampling error of the standard deviation is 0.011).  A wrong nbin - 2 or a
    missing sqrt(Stt) fails it."""
    rng = np.random.default_rng(20261021)
    nbin, n = 256, 4096
    i = np.arange(nbin)
    T = np.exp(-0.5 * ((i - 0.3 * nbin) / 8.0) ** 2).astype(F)
    g = rng.uniform(0.5, 4.0, n)
    b = rng.uniform(-5.0, 5.0, n)
    X = (g[:, None] * T.astype(np.float64) + b[:, None] + rng.standard_normal((n, nbin))).astype(F)
    r = ds.profiles(T, X, np.ones(n))
    pull = (r["amp"] - g) / r["err"]
    print("pulls: mean %.4f, std %.4f" % (pull.mean(), pull.std()))
    assert abs(pull.mean()) <= 0.1 and 0.9 <= pull.std() <= 1.1
    assert np.all(np.abs(r["base"] - b) < 1.0)


def test_sum64_order():
    """Chain 0 cancels 1e16 - 1e16 before it meets its 1.0; a plain ascending sum
    loses the first 1.0 and numpy's pairwise sum both."""
    v = np.zeros(130)
    v[0], v[1], v[64], v[65], v[128] = 1e16, 1.0, -1e16, 1.0, 1.0
    assert ds.sum64(v) == 3.0
    assert sum(v.tolist()) == 2.0 and float(np.add.reduce(v)) != 3.0
    # the tree: c[l] + c[l + 32] first.  Chains 0 and 32 cancel before anything else is added
    u = np.zeros(64)
    u[0], u[32], u[1] = 1e16, -1e16, 1.0
    assert ds.sum64(u) == 1.0 and sum(u.tolist()) == 0.0
    # ... and not neighbours first: (1e16 + 1) + (-1e16 + 0) would lose the 1.0.
    # Lanes 0 and 2 meet at h = 2 and cancel; lane 1 joins at h = 1
    t = np.zeros(64)
    t[0], t[1], t[2] = 1e16, 1.0, -1e16
    assert ds.sum64(t) == 1.0 and sum(t.tolist()) == 0.0
    # fewer values than chains, a partly filled last round, several axes
    assert ds.sum64(np.array([1.0, 2.0, 3.0, 4.0])) == 10.0
    w = np.arange(2 * 3 * 100, dtype=np.float64).reshape(2, 3, 100)
    assert np.array_equal(ds.sum64(w), w.sum(axis=-1)) and ds.sum64(w).shape == (2, 3)
    # a chain that starts at +0.0 never yields -0.0
    assert np.signbit(ds.sum64(np.full(70, -0.0))) == False  # noqa: E712


def test_terms_follow_the_definition():
    """profiles() against a literal per-profile transcription of the formulas."""
    T, X, w, _, _ = dc.profiles(100, 5)
    got = ds.profiles(T, X, w)
    mT, t, Stt = ds.template_terms(T)
    assert mT == ds.sum64(T.astype(np.float64)) / 100.0 and bits_equal(t, T.astype(np.float64) - mT)
    for k in range(5):
        x = X[k].astype(np.float64)
        mx = ds.sum64(x) / 100.0
        a = ds.sum64(t * x) / Stt
        r = (x - mx) - a * t
        e = np.sqrt(ds.sum64(r * r) / 98.0) / np.sqrt(Stt)
        assert (got["amp"][k], got["err"][k], got["base"][k]) == (a, e, mx - a * mT)


def test_mask_rule_and_ieee_cases():
    T, X, w = dc.edge_profiles()
    got = ds.profiles(T, X, w)
    for key in ("amp", "err", "base"):
        assert got[key][1] == 0 and got[key][4] == 0 and not np.signbit(got[key][1])   # w == 0: +0.0, NaN row unread
        assert not np.isfinite(got[key][2])                                            # the Inf is not special-cased
        assert np.all(np.isfinite(got[key][[0, 3]]))
    # a constant template: Stt == 0 -> 0 / 0
    flat = ds.profiles(np.full(64, 2.5, F), X[:1, :64], [1.0])
    assert np.isnan(flat["amp"][0]) and np.isnan(flat["err"][0]) and np.isnan(flat["base"][0])
    # all masked: zeros, whatever the template
    z = ds.profiles(np.full(64, 2.5, F), np.full((3, 64), np.nan, F), np.zeros(3))
    assert all(bits_equal(z[k], np.zeros(3)) for k in ("amp", "err", "base"))


def test_refusals():
    T, X, w, _, _ = dc.profiles(16, 3)
    with pytest.raises(ValueError, match="below 4"):
        ds.profiles(T[:3], X[:, :3], w)
    with pytest.raises(ValueError, match="nprof, 16"):
        ds.profiles(T, X[:, :15], w)
    with pytest.raises(ValueError, match="nprof, 16"):
        ds.profiles(T, X[0], w)
    with pytest.raises(ValueError, match="weights"):
        ds.profiles(T, X, w[:2])
    with pytest.raises(ValueError, match="template must be"):
        ds.profiles(T[None], X, w)
    cube = X.reshape(1, 3, 16)
    with pytest.raises(ValueError, match="weights must be"):
        ds.cube(cube, T, np.ones((3, 1)))
    with pytest.raises(ValueError, match="template of"):
        ds.cube(cube, dc.template(32), np.ones((1, 3)))
    with pytest.raises(ValueError, match="nsub, nchan, nbin"):
        ds.cube(X, T, np.ones((1, 3)))
    with pytest.raises(ValueError, match="delays must be"):
        ds.cube(np.zeros((1, 3, 64), F), dc.template(64), np.ones((1, 3)), delay=np.zeros(2))
    assert ds.profiles(T[:4], X[:, :4], w)["amp"].shape == (3,)       # 4 bins: the fewest


def test_cube_forms():
    """cube(): integer shifts gather at the dedispersed index, a stored-
    dedispersed cube is read as it is, fractional delays go through
    phase_rotation.rotate."""
    from iterative_cleaner_amd import phase_rotation as pr
    rng = np.random.default_rng(4)
    nsub, nchan, nbin = 2, 3, 64
    raw = rng.standard_normal((nsub, nchan, nbin)).astype(F)
    T = dc.template(nbin)
    w = np.ones((nsub, nchan), F)
    w[1, 2] = 0
    shift = np.array([0, 5, 64 + 63])
    got = ds.cube(raw, T, w, shift=shift)
    xd = np.stack([np.roll(raw[:, c], -int(shift[c]) % nbin, axis=-1) for c in range(nchan)], axis=1)
    assert xd[0, 1, 0] == raw[0, 1, 5]
    want = ds.profiles(T, xd.reshape(-1, nbin), w.reshape(-1))
    assert dc.same(got, {k: v.reshape(nsub, nchan) for k, v in want.items()}) and got["amp"][1, 2] == 0
    asis = ds.cube(raw, T, w, shift=shift, delay=np.ones(nchan), input_dedispersed=True)
    assert dc.same(asis, ds.cube(raw, T, w))
    for delay in (np.array([0.25, 3.5, -7.125]), rng.uniform(-9, 9, (nsub, nchan))):
        rot = pr.rotate(raw, pr.phasors(nbin, delay), +1)
        assert dc.same(ds.cube(raw, T, w, delay=delay), ds.cube(rot, T, w))
    assert not bits_equal(ds.cube(raw, T, w, delay=np.array([0.25, 3.5, -7.125]))["amp"], got["amp"])


def test_normalise_and_env(monkeypatch):
    assert ds.parse_env(None) is None and ds.parse_env("") is None and ds.parse_env(" 0 ") is None
    assert ds.parse_env("1") is True and ds.parse_env("out/x.dynspec") == "out/x.dynspec"
    assert ds.normalise(False) is None and ds.normalise(0) is None and ds.normalise("") is None
    assert ds.normalise(True) is True and ds.normalise(1) is True and ds.normalise("1") is True
    assert ds.normalise("a.txt") == "a.txt" and ds.normalise(type("P", (), {"__fspath__": lambda s: "p.txt"})()) == "p.txt"
    for bad in (2, 1.5, ("a",)):
        with pytest.raises(ValueError, match="switch or a path"):
            ds.normalise(bad)
    monkeypatch.delenv("IC_DYNSPEC", raising=False)
    assert ds.normalise(None) is None
    for text, want in (("", None), ("0", None), ("1", True), ("/tmp/d.txt", "/tmp/d.txt")):
        monkeypatch.setenv("IC_DYNSPEC", text)
        assert ds.normalise(None) == want
    monkeypatch.setenv("IC_DYNSPEC", "1")
    assert ds.normalise(False) is None                         # an argument overrides the switch


def test_save_load_round_trip(tmp_path):
    rng = np.random.default_rng(6)
    nsub, nchan = 3, 5
    res = dict(amp=rng.standard_normal((nsub, nchan)) * 1e-3, err=np.abs(rng.standard_normal((nsub, nchan))) * 1e5,
               base=rng.standard_normal((nsub, nchan)))
    res["amp"][0, 0], res["amp"][0, 1], res["err"][0, 1] = -0.0, np.nan, np.inf
    res["amp"][2, 4] = np.nextafter(1.0, 2.0)
    mw = np.ones((nsub, nchan))
    mw[1, :] = 0
    mw[2, 3] = 0
    freq = 120.0 + rng.uniform(0, 1, (nsub, nchan))
    tmin = np.array([0.5, 1.5, 2.5]) / 3.0
    path = str(tmp_path / "a.dynspec")
    ds.save(path, res, mw, dict(archive="obs.ar", nbin=64, template="standard", freq_MHz=freq, time_min=tmin))
    text = open(path).read().splitlines()
    head = [ln for ln in text if ln.startswith("#")]
    assert head[0] == "# dynspec 1" and "# archive: obs.ar" in head and "# shape: 3 5 64" in head
    assert "# template: standard" in head and "# masked: 6" in head
    assert len(text) - len(head) == nsub * nchan and text[len(head)].split()[:2] == ["0", "0"]
    assert text[len(head) + 5].split()[:4] == ["1", "0", "0", "0"]              # masked: zeros
    back = ds.load(path)
    live = mw != 0
    for key in ("amp", "err"):
        assert bits_equal_nan(back[key][live], res[key][live]), key
        assert bits_equal(back[key][~live], np.zeros(6))
    assert np.signbit(back["amp"][0, 0]) and back["err"][0, 1] == np.inf
    assert bits_equal(back["freq_MHz"], freq) and bits_equal(back["time_min"], tmin)
    assert (back["archive"], back["nbin"], back["template"], back["masked"]) == ("obs.ar", 64, "standard", 6)
    # no axes: NaN columns; and a second save of what was loaded gives the same bytes
    ds.save(path, res, mw, dict(archive="obs.ar", nbin=64))
    bare = ds.load(path)
    assert np.all(np.isnan(bare["freq_MHz"])) and np.all(np.isnan(bare["time_min"])) and bare["template"] == "cleaner"
    first = open(path).read()
    ds.save(path, bare, mw, dict(archive="obs.ar", nbin=64))
    assert open(path).read() == first
    with pytest.raises(ValueError, match="mask weights"):
        ds.save(path, res, mw[:2])
    (tmp_path / "junk").write_text("hello\n")
    with pytest.raises(ValueError, match="not a dynamic-spectrum file"):
        ds.load(str(tmp_path / "junk"))


def test_merge_shards():
    rng = np.random.default_rng(7)
    whole = {k: rng.standard_normal((4, 7)) for k in ("amp", "err", "base")}
    parts = [{k: v[:, a:b] for k, v in whole.items()} for a, b in ((0, 2), (2, 3), (3, 7))]
    assert dc.same(ds.merge_shards(parts), whole)
    assert ds.merge_shards(parts)["amp"].flags.c_contiguous
    with pytest.raises(ValueError, match="no shard"):
        ds.merge_shards([])


def _stub_loop(seen, result):
    def run_loop(cube, w0, shift, args, **kw):
        seen.append(kw)
        nsub, nchan = np.shape(w0)
        test = np.zeros((nsub, nchan))
        test[2, 1] = 1.5                                   # the loop zaps one profile
        out = dict(n_iter=1, converged=True, loops=1, changed=np.array([1]), nzero=np.array([1]),
                   bad_fits=np.array([0]), test=test, weights=np.asarray(w0, F))
        if kw.get("dynspec"):
            out["dynspec"] = result
        return out
    return run_loop


def _stand_in(tmp_path, name="obs.ar"):
    from iterative_cleaner_amd import archive as ica
    from iterative_cleaner_amd import synth
    data, w0, shift = synth.make_cube(4, 6, 32, 3, 0.0, dead_frac=0.0)
    w0[:, 4] = 0                                           # a channel dead on arrival
    w0[0, 4] = 1
    ica.Archive(data, w0, shift, filename=name).unload(str(tmp_path / name))
    return w0


def test_clean_writes_the_file(tmp_path, monkeypatch):
    """clean() on a stand-in archive with run_loop stubbed: off, no file and no
    dynspec request; on, the file is masked with the output archive's final
    weights, after set_weights_archive and find_bad_parts (--bad_chan removes
    the channel that arrived three quarters dead), not with the loop's."""
    from iterative_cleaner_amd import archive as ica
    from iterative_cleaner_amd import cleaner
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("IC_DYNSPEC", raising=False)
    w0 = _stand_in(tmp_path)
    rng = np.random.default_rng(11)
    result = {k: rng.standard_normal((4, 6)) + 3.0 for k in ("amp", "err", "base")}
    argv = ["-l", "-q", "--bad_chan", "0.7", "obs.ar"]
    seen = []
    monkeypatch.setattr(cleaner, "run_loop", _stub_loop(seen, result))
    cleaner.clean(ica.Archive_load("obs.ar"), cleaner.parse_arguments(argv), "obs.ar")
    assert seen[-1]["dynspec"] is False and not os.path.exists("obs.ar.dynspec")
    out = cleaner.clean(ica.Archive_load("obs.ar"), cleaner.parse_arguments(argv), "obs.ar", dynspec=True)
    assert seen[-1]["dynspec"] is True
    final = out.get_weights()
    assert final[0, 4] == 0 and w0[0, 4] == 1 and final[2, 1] == 0     # find_bad_parts, set_weights_archive
    back = ds.load("obs.ar.dynspec")
    masked = final == 0
    assert back["masked"] == int(masked.sum()) == 5 and (back["archive"], back["nbin"]) == ("obs.ar", 32)
    for key in ("amp", "err"):
        assert bits_equal(back[key][~masked], result[key][~masked]) and np.all(back[key][masked] == 0), key
    assert back["amp"][0, 4] == 0 and result["amp"][0, 4] != 0
    assert back["template"] == "cleaner"
    assert np.all(np.isnan(back["freq_MHz"])) and np.all(np.isnan(back["time_min"]))   # the stand-in offers neither
    # the switch: "1" is the default name, anything else the path; an argument wins
    os.remove("obs.ar.dynspec")
    monkeypatch.setenv("IC_DYNSPEC", "1")
    cleaner.clean(ica.Archive_load("obs.ar"), cleaner.parse_arguments(argv), "obs.ar")
    first = open("obs.ar.dynspec").read()
    os.remove("obs.ar.dynspec")
    monkeypatch.setenv("IC_DYNSPEC", "elsewhere.txt")
    cleaner.clean(ica.Archive_load("obs.ar"), cleaner.parse_arguments(argv), "obs.ar")
    assert open("elsewhere.txt").read() == first and not os.path.exists("obs.ar.dynspec")
    os.remove("elsewhere.txt")
    cleaner.clean(ica.Archive_load("obs.ar"), cleaner.parse_arguments(argv), "obs.ar", dynspec=False)
    assert not os.path.exists("elsewhere.txt") and seen[-1]["dynspec"] is False


def test_archive_axes_when_offered():
    """An archive object with psrchive's per-Integration frequency and epoch
    gets its columns; one without keeps NaN."""
    class Epoch:
        def __init__(self, d):
            self.d = d

        def in_days(self):
            return self.d

    class Integ:
        def __init__(self, s):
            self.s = s

        def get_centre_frequency(self, c):
            return 100.0 + c + 0.5 * self.s

        def get_epoch(self):
            return Epoch(59000.0 + (self.s + 0.5) / 1440.0)

    class Ar:
        def get_nsubint(self): return 2
        def get_nchan(self): return 3
        def get_Integration(self, s): return Integ(s)
        def start_time(self): return Epoch(59000.0)

    freq, tmin = ds.archive_axes(Ar())
    assert np.array_equal(freq, [[100.0, 101.0, 102.0], [100.5, 101.5, 102.5]])
    assert np.allclose(tmin, [0.5, 1.5], atol=1e-6)


def test_c_abi_surface():
    """The two calls are declared, exported by name in the binding, the ABI
    version did not move, the kernel has its unit and its name, and the
    keyword runs through every layer."""
    from iterative_cleaner_amd import _native, batch, cleaner, sharded
    text = open(os.path.join(REPO, "include", "iterative_cleaner.h")).read()
    for name in ("ic_get_dynspec", "ic_dynspec_profiles"):
        assert re.search(r"\bint %s\(" % name, text) and name in _native.EXPORTS
    assert re.search(r"#define IC_ABI_VERSION 9\b", text) and _native.ABI_VERSION == 9
    csrc = os.path.join(REPO, "iterative_cleaner_amd", "csrc")
    assert "ic_dynspec.hip" in open(os.path.join(csrc, "Makefile")).read()
    names = re.search(r"kKernelNames\[K_COUNT\] = \{(.*?)\};", open(os.path.join(csrc, "ic_session.hip")).read(), re.S)
    assert names.group(1).split(",")[-1].strip() == '"k_dynspec"'           # appended: the other ids did not move
    for fn in (cleaner.run_loop, cleaner.clean, batch.pipeline, batch.run_lanes, batch.clean_batch):
        assert "dynspec" in inspect.signature(fn).parameters
    assert hasattr(_native.GpuSession, "dynspec") and hasattr(_native, "dynspec_profiles")
    assert "dynspec" not in sharded._loop_kwargs(dict(dynspec=True), (2, 4), 64)   # acted on after the run
