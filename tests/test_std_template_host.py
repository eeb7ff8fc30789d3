"""The written definition of the standard template (std_template.py): the
alignment rules, their failure cases, the validation, the IC_STD_TEMPLATE
switch and the loaders.  No GPU."""
import os

import numpy as np
import pytest

from iterative_cleaner_amd import std_template as st
from std_template_cases import delayed, pulse

NBINS = (64, 100, 1024)


@pytest.mark.parametrize("nbin", NBINS)
def test_integer_rolls_are_recovered_exactly(nbin):
    """S = roll(A, -k): lag == k, |delta| <= 1e-9, and mode int returns A bit
    for bit.  Measured with this module: |delta| <= 1.6e-12 (8.9e-16 at 64
    bins, 0 at 100, 1.6e-12 at 1024)."""
    A = pulse(nbin)
    for k in (0, 1, nbin // 2, nbin - 1):
        S = np.roll(A, -k)
        r = st.align(S, A, "int")
        print("nbin %d roll %d: lag %d delta %.3g" % (nbin, k, r["lag"], r["shift"] - k))
        assert r["aligned"] == 1 and r["lag"] == k
        assert abs(r["shift"] - k) <= 1e-9
        assert r["template"].dtype == np.float32 and r["template"].tobytes() == A.tobytes()
        # the peak rule alone
        assert st.peak(st.ccf(S, A)) == (1, k, r["shift"])


@pytest.mark.parametrize("nbin,cap", [(64, 0.02), (1024, 1e-4)])
def test_fractional_delays_are_recovered(nbin, cap):
    """S = rotate(A, +d): the shift is within 0.02 bin of d at 64 bins and
    within 1e-4 bin at 1024.  Measured with this module: at 64 bins 6.4e-3
    (d = 0.25), 4.4e-8 (3.5), 5.8e-3 (17.37); at 1024 bins 2.5e-5, 7.5e-7,
    2.1e-5.  The parabola is exact for a half-bin delay of a symmetric peak and
    worst near a quarter bin."""
    A = pulse(nbin)
    for d in (0.25, 3.5, 17.37):
        r = st.align(delayed(A, d), A, "frac")
        print("nbin %d delay %g: lag %d shift %.9g error %.3g" % (nbin, d, r["lag"], r["shift"], r["shift"] - d))
        assert r["aligned"] == 1
        assert abs(r["shift"] - d) <= cap
        # the aligned template is the standard rotated back onto A
        assert np.max(np.abs(r["template"].astype(np.float64) - A)) <= 2.5e-3 * float(A.max())


def test_ccf_is_the_written_sum():
    """c[k] = sum_i a[i] * s[(i - k) mod n], every product rounded on its own
    and added in ascending i, against a plain Python loop."""
    rng = np.random.default_rng(5)
    n = 12
    S = (rng.standard_normal(n) * 100).astype(np.float32)
    A = (rng.standard_normal(n) * 100).astype(np.float32)
    m = 0.0
    for v in S:
        m = m + float(v)
    m = m / n
    want = []
    for k in range(n):
        acc = 0.0
        for i in range(n):
            acc = acc + float(A[i]) * (float(S[(i - k) % n]) - m)
        want.append(acc)
    assert st.ccf(S, A).tobytes() == np.array(want, np.float64).tobytes()


def test_peak_rules():
    # the first of equal maxima; the parabola only where it opens downwards
    assert st.peak([1.0, 3.0, 3.0, 0.0]) == (1, 1, 1.0 + 0.5 * (1.0 - 3.0) / ((1.0 - 3.0) + (3.0 - 3.0)))
    assert st.peak([2.0, 2.0, 2.0, 2.0]) == (1, 0, 0.0)          # den == 0: no sub-bin part
    assert st.peak([5.0, 1.0, 0.0, 2.0]) == (1, 0, 0.0 + 0.5 * (2.0 - 1.0) / ((2.0 - 5.0) + (1.0 - 5.0)))
    # failures: no positive peak, a trough deeper than the peak, a non-finite value anywhere
    assert st.peak([1.0, -3.0, 0.5, 0.25]) == (0, 0, 0.0)
    assert st.peak([3.0, -3.0, 0.5, 0.25])[:2] == (1, 0)
    assert st.peak([-1.0, -2.0, -0.5, -3.0]) == (0, 0, 0.0)
    assert st.peak([0.0, 0.0, 0.0, 0.0]) == (0, 0, 0.0)
    assert st.peak([1.0, np.nan, 9.0, 2.0]) == (0, 0, 0.0)
    assert st.peak([1.0, np.inf, 9.0, 2.0]) == (0, 0, 0.0)


@pytest.mark.parametrize("mode", ["int", "frac"])
def test_failed_alignment_uses_the_standard_as_given(mode):
    A = pulse(64)
    S = np.roll(A, -9)
    bad = A.copy()
    bad[7] = np.nan
    for against in (bad, -S):
        r = st.align(S, against, mode)
        assert (r["aligned"], r["lag"], r["shift"]) == (0, 0, 0.0)
        assert r["template"].tobytes() == S.tobytes()


def test_mode_none_measures_nothing():
    A = pulse(64)
    S = np.roll(A, -9)
    r = st.align(S, A, "none")
    assert (r["aligned"], r["lag"], r["shift"], r["mode"]) == (0, 0, 0.0, st.ALIGN_NONE)
    assert r["template"].tobytes() == S.tobytes()


def test_check():
    A = pulse(64)
    out = st.check(A.astype(np.float64), 64)
    assert out.dtype == np.float32 and out.flags.c_contiguous and out.tobytes() == A.tobytes()
    assert st.check(list(range(8)), 8).tobytes() == np.arange(8, dtype=np.float32).tobytes()
    for bad, nbin, word in ((A[None, :], 64, "1-D"), (A, 128, "not rebinned"), (np.ones(64, np.float32), 64, "constant"),
                            (np.arange(3.0), 3, "nbin=3"), (np.array([1.0, 2.0, np.nan, 4.0]), 4, "non-finite"),
                            (np.array([1.0, 2.0, np.inf, 4.0]), 4, "non-finite"),
                            (np.array([1.0, 2.0, 1e300, 4.0]), 4, "non-finite"),     # overflows f32
                            (np.array([1 + 2j, 0, 0, 0]), 4, "real")):
        with pytest.raises(ValueError, match=word):
            st.check(bad, nbin)


def test_auto_resolves_by_length():
    assert st.resolve_align("auto", 1024) == st.ALIGN_FRAC      # a power of two
    assert st.resolve_align(None, 1000) == st.ALIGN_FRAC        # mixed radix
    assert st.resolve_align("auto", 100) == st.ALIGN_INT        # neither
    assert st.resolve_align("AUTO", 8192) == st.ALIGN_FRAC
    assert st.resolve_align("auto", 16384) == st.ALIGN_INT
    assert st.resolve_align("none", 100) == st.ALIGN_NONE
    assert st.resolve_align(st.ALIGN_INT, 100) == st.ALIGN_INT
    with pytest.raises(ValueError, match="use 'int'"):
        st.resolve_align("frac", 100)
    with pytest.raises(ValueError, match="one of auto"):
        st.resolve_align("nearest", 128)
    with pytest.raises(ValueError, match="one of auto"):
        st.resolve_align(7, 128)
    assert st.align(np.roll(pulse(100), -3), pulse(100))["mode"] == st.ALIGN_INT
    assert st.align(np.roll(pulse(64), -3), pulse(64))["mode"] == st.ALIGN_FRAC


def test_switch_parser(monkeypatch):
    assert st.parse("") is None and st.parse(None) is None and st.parse("   ") is None
    assert st.parse("/data/J0437.std.npy") == ("/data/J0437.std.npy", "auto")
    assert st.parse(" std.npy , INT ") == ("std.npy", "int")
    assert st.parse("a,b.npy,none") == ("a,b.npy", "none")
    assert st.parse("std.ar,frac") == ("std.ar", "frac")
    for bad in ("std.npy,nearest", ",int", "std.npy,"):
        with pytest.raises(ValueError, match="IC_STD_TEMPLATE"):
            st.parse(bad)
    monkeypatch.delenv(st.ENV, raising=False)
    assert st.env_std_template() is None and st.normalise(None, 64) is None
    monkeypatch.setenv(st.ENV, "")
    assert st.normalise(None, 64) is None
    monkeypatch.setenv(st.ENV, "x.npy,int")
    assert st.env_std_template() == ("x.npy", "int")


def test_load_npy_and_normalise(tmp_path, monkeypatch):
    A = pulse(100)
    path = str(tmp_path / "std.npy")
    np.save(path, A.astype(np.float64))
    assert st.load(path, 100).tobytes() == A.tobytes()
    with pytest.raises(ValueError, match="not rebinned"):
        st.load(path, 128)
    np.save(str(tmp_path / "two.npy"), np.zeros((2, 100)))
    with pytest.raises(ValueError, match="1-D"):
        st.load(str(tmp_path / "two.npy"), 100)
    S, mode = st.normalise(path, 100)
    assert S.tobytes() == A.tobytes() and mode == st.ALIGN_INT          # auto at 100 bins
    S, mode = st.normalise((path, "none"), 100)
    assert mode == st.ALIGN_NONE
    S, mode = st.normalise((A, "int"), 100)
    assert S.tobytes() == A.tobytes() and mode == st.ALIGN_INT
    assert st.normalise((S, mode), 100)[1] == st.ALIGN_INT              # a normalised pair again
    assert st.normalise(pulse(64), 64)[1] == st.ALIGN_FRAC
    monkeypatch.setenv(st.ENV, path + ",int")
    S, mode = st.normalise(None, 100)
    assert S.tobytes() == A.tobytes() and mode == st.ALIGN_INT
    monkeypatch.setenv(st.ENV, path + ",frac")
    with pytest.raises(ValueError, match="use 'int'"):
        st.normalise(None, 100)


def test_load_from_a_stand_in_archive(tmp_path):
    """An archive path goes through archive_backend(): pscrunch,
    remove_baseline, dedisperse, fscrunch, tscrunch, profile (0, 0, 0)."""
    from iterative_cleaner_amd import archive as ica
    from iterative_cleaner_amd import synth
    data, w0, shift = synth.make_cube(4, 16, 64, 3, 0.0, npol=2)
    path = str(tmp_path / "std.ar")
    ica.Archive(data, w0, shift, filename=path).unload(path)
    S = st.load(path, 64, backend=ica)
    ar = ica.Archive_load(path)
    for step in ("pscrunch", "remove_baseline", "dedisperse", "fscrunch", "tscrunch"):
        getattr(ar, step)()
    want = np.asarray(ar.get_Profile(0, 0, 0).get_amps(), np.float32)
    assert S.dtype == np.float32 and S.shape == (64,) and S.tobytes() == want.tobytes()
    assert st.load(path, 64).tobytes() == want.tobytes()      # the default backend (no psrchive here: the stand-in)
    with pytest.raises(ValueError, match="not rebinned"):
        st.load(path, 128, backend=ica)


def test_load_uses_the_backend_in_the_written_order():
    calls = []

    class Prof:
        def get_amps(self):
            calls.append("get_amps")
            return pulse(64)

    class Ar:
        def __getattr__(self, name):
            if name in ("pscrunch", "remove_baseline", "dedisperse", "fscrunch", "tscrunch"):
                return lambda: calls.append(name)
            raise AttributeError(name)

        def get_Profile(self, *idx):
            calls.append("get_Profile%s" % (idx,))
            return Prof()

    class Backend:
        @staticmethod
        def Archive_load(path):
            calls.append("load " + path)
            return Ar()

    S = st.load("J0000.std", 64, backend=Backend)
    assert S.tobytes() == pulse(64).tobytes()
    assert calls == ["load J0000.std", "pscrunch", "remove_baseline", "dedisperse", "fscrunch", "tscrunch",
                     "get_Profile(0, 0, 0)", "get_amps"]


def test_warn_failed_goes_to_stderr_only(capsys):
    st.warn_failed(None, st.ALIGN_INT)
    st.warn_failed(dict(aligned=1, lag=3, shift=3.1), st.ALIGN_INT)
    st.warn_failed(dict(aligned=0, lag=0, shift=0.0), st.ALIGN_NONE)
    assert capsys.readouterr() == ("", "")
    st.warn_failed(dict(aligned=0, lag=0, shift=0.0), st.ALIGN_FRAC)
    out, err = capsys.readouterr()
    assert out == "" and "alignment" in err and err.count("\n") == 1


def test_python_layers_take_std_template():
    """The parameter is on every layer the issue names (the GPU tests run them)."""
    import inspect

    from iterative_cleaner_amd import _native, batch, cleaner, sharded
    for fn in (cleaner.run_loop, cleaner.clean, batch.clean_batch, batch.pipeline, batch.run_lanes,
               _native.GpuSession.__init__):
        assert inspect.signature(fn).parameters["std_template"].default is None, fn
    assert "std_template" in sharded._LOOP_KEYS
    for name in ("ic_set_std_template", "ic_get_std_alignment", "ic_align_template"):
        assert name in _native.EXPORTS
    header = open(os.path.join(os.path.dirname(os.path.abspath(_native.__file__)), "..", "include",
                               "iterative_cleaner.h")).read()
    for name, value in (("IC_ALIGN_NONE", st.ALIGN_NONE), ("IC_ALIGN_INT", st.ALIGN_INT),
                        ("IC_ALIGN_FRAC", st.ALIGN_FRAC)):
        assert "#define %s %d" % (name, value) in header
