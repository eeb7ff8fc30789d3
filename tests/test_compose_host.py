"""The composed yardstick (compose_ref.clean) is right, on the CPU: it is the
oracle's loop when no option is set, it reproduces the reference's own outputs,
one option at a time it is what that option's own tests state, and the composed
cases of test_compose_gpu.py mean something (the conditions on their inputs, and
the measured tolerance on detrended test values)."""
import os

import numpy as np
import pytest

import compose_ref as cr
from helpers import GOLDEN, bits_equal, bits_equal_nan, case_kwargs, load_clean_case


def _cube(nsub, nchan, nbin, seed=3, rfi=0.2):
    from iterative_cleaner_amd import synth
    data, w0, shift = synth.make_cube(nsub, nchan, nbin, seed, rfi)
    return np.ascontiguousarray(data[:, 0]), w0, shift


def _same_as_loop(got, ref, what):
    """Every output of compose_ref.clean against oracle.lib.clean_loop's, bit for
    bit (a NaN matches any NaN)."""
    n = got["n_iter"]
    assert got["loops"] == ref["loops"], what
    assert np.array_equal(got["changed"], ref["changed"][:n]) and np.array_equal(got["nzero"], ref["nzero"][:n]), what
    if n < len(ref["changed"]):
        assert not ref["changed"][n:].any() and not ref["nzero"][n:].any(), what   # the oracle ran no further
    for k in range(n):
        assert bits_equal_nan(got["T_all"][k], ref["T"][k]), "%s: template of iteration %d" % (what, k + 1)
    for key in ("weights", "test", "amp", "info", "std", "mean", "ptp", "fft", "residual"):
        assert bits_equal_nan(got[key], ref[key]), "%s: %s" % (what, key)


PLAIN = {
    "integer shifts": ((12, 48, 128), dict()),
    "delays per channel": ((6, 16, 128), dict(delay="chan")),
    "delays per profile": ((6, 16, 128), dict(delay="prof")),
    "input dedispersed": ((6, 16, 128), dict(delay="ded", input_dedispersed=True)),
    "closed fit": ((12, 48, 128), dict(fit_mode=1)),
    "closed fit, delays per channel": ((6, 16, 128), dict(fit_mode=1, delay="chan")),
    "data_f64": ((12, 48, 128), dict(data_f64=True)),
    "data_f64, delays per profile": ((6, 16, 128), dict(data_f64=True, delay="prof")),
    "pulse region": ((12, 48, 128), dict(pulse_region=(0.5, 30, 48))),
}


@pytest.mark.parametrize("name", sorted(PLAIN))
def test_no_options_is_the_oracle_loop(name, oracle_lib):
    """max_iter = 5, every output, every iteration's template and counts."""
    shape, kw = PLAIN[name]
    kw = dict(kw)
    raw, w0, shift = _cube(*shape)
    if "delay" in kw:
        kw["delay"] = cr.delays(kw["delay"], shift, shape[2], shape[0])
    got = cr.clean(raw, w0, shift, **kw)
    ref = oracle_lib.clean_loop(raw, w0, shift, want_details=True, want_residual=True, **kw)
    assert got["n_iter"] >= 2, name     # the loop rule is exercised
    _same_as_loop(got, ref, name)


@pytest.mark.parametrize("name", ["s12x48x128", "s12x40x128_pr", "s12x48x128_f64", "s12x48x128_fft"])
def test_reproduces_the_reference_fixtures(name, prefix="clean_"):
    """The outputs the reference itself wrote (tests/golden), by the measure
    test_oracle_golden.py holds the oracle to."""
    z, meta, raw, w0, shift, args = load_clean_case(os.path.join(GOLDEN, "%s%s.npz" % (prefix, name)))
    kw = case_kwargs(z, meta)
    out = cr.clean(raw, w0, shift, delay=kw["delay"], input_dedispersed=kw["input_dedispersed"],
                   chanthresh=args["chanthresh"], subintthresh=args["subintthresh"], max_iter=args["max_iter"],
                   pulse_region=None if args["pulse_region"] == [0, 0, 1] else args["pulse_region"],
                   data_f64=meta.get("data_f64", False))
    nit = int(z["n_iter"])
    assert out["loops"] == int(z["loops"]) and out["n_iter"] == nit
    for k in range(1, nit + 1):
        assert bits_equal_nan(out["T_all"][k - 1], z["T_%d" % k]), "template of loop %d" % k
    assert bits_equal(out["amp"].ravel(), z["amp_%d" % nit])
    assert bits_equal(out["info"].ravel(), z["info_%d" % nit])
    assert bits_equal(out["weights"], z["weights_%d" % nit])
    assert bits_equal_nan(out["std"], z["diag_std_%d" % nit])
    assert bits_equal_nan(out["mean"], z["diag_mean_%d" % nit])
    assert bits_equal_nan(out["ptp"], z["diag_ptp_%d" % nit])
    ref = z["test_%d" % nit]
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(out["test"]), np.isnan(ref))
    assert np.all(np.abs(out["test"][fin] - ref[fin]) <= 1e-9 * np.maximum(1, np.abs(ref[fin])))


def test_reproduces_a_mixed_radix_reference_fixture():
    """1000 bins with fractional delays: the C oracle's rotation is written for
    powers of two (oracle.lib refuses other lengths), so compose_ref.rotate
    takes the written definition there; the reference's own outputs pin it."""
    test_reproduces_the_reference_fixtures("s4x16x1000_fft_pr", prefix="mr_clean_")
    with pytest.raises(ValueError, match="power-of-two"):
        from oracle import lib
        lib.rotate(np.zeros((1, 2, 1000), np.float32), np.zeros(2))


@pytest.mark.parametrize("mode", ["int", "chan", "prof", "ded"])
def test_hotbins_alone_is_the_loop_on_the_repaired_cube(mode, oracle_lib):
    from iterative_cleaner_amd import hotbins as hb
    raw, w0, shift, delay = cr.archive(128, 2, mode)
    hot = cr.hot_window(128)
    fixed, want = hb.repair_cube(raw, w0, hot, shift=shift, delay=delay, input_dedispersed=mode == "ded")
    assert want["total"] > 0 and not bits_equal(fixed, raw)
    got = cr.clean(raw, w0, shift, delay=delay, input_dedispersed=mode == "ded", hotbins=hot)
    ref = oracle_lib.clean_loop(fixed, w0, shift, delay=delay, input_dedispersed=mode == "ded", want_details=True,
                                want_residual=True)
    _same_as_loop(got, ref, mode)
    assert bits_equal(got["cube"], fixed)
    for key in ("count", "bins", "offsets"):
        assert bits_equal(got["hotbins"][key], want[key]), key


@pytest.mark.parametrize("mode", ["int", "prof"])
def test_detrend_of_order_zero_is_the_plain_loop(mode, oracle_lib):
    raw, w0, shift, delay = cr.archive(128, 2, mode)
    got = cr.clean(raw, w0, shift, delay=delay, detrend=(0, 0))
    ref = oracle_lib.clean_loop(raw, w0, shift, delay=delay, want_details=True, want_residual=True)
    _same_as_loop(got, ref, mode)
    assert not got["chan_coef"].any() and not got["subint_coef"].any()


def test_standard_alone_is_one_pass_with_the_aligned_template(oracle_lib):
    """With only std=: the template is std_template.align of the standard against
    the oracle's first template, and the fit, diagnostics and test values are
    the oracle's pieces on it; the reported second iteration repeats the first."""
    from iterative_cleaner_amd import std_template as st
    raw, w0, shift, _ = cr.archive(128, 2, "int")
    S = cr.standard(128)
    got = cr.clean(raw, w0, shift, std=(S, "int"))
    A = oracle_lib.template(raw, w0, shift)
    al = st.align(S, A, "int")
    assert bits_equal(got["A"], A) and bits_equal(got["T"], al["template"]) and len(got["T_all"]) == 1
    assert got["std_alignment"] == dict(aligned=1, lag=al["lag"], shift=al["shift"]) and al["lag"] == 128 - 5
    amp, info, Rd = oracle_lib.fit_residual(oracle_lib.fit_cube(raw, w0, shift), al["template"])
    assert bits_equal(got["amp"].ravel(), amp) and bits_equal(got["info"].ravel(), info)
    assert got["loops"] == 2 and got["n_iter"] == 2 and got["changed"][1] == 0 and got["nzero"][0] == got["nzero"][1]
    assert got["changed"][0] == got["nzero"][0] - int((w0 == 0).sum()) > 0
    one = cr.clean(raw, w0, shift, std=(S, "int"), max_iter=1)
    assert one["loops"] == 1 and one["n_iter"] == 1 and bits_equal(one["weights"], got["weights"])
    # a standard that fails to align (anti-correlated) is used as given
    neg = cr.clean(raw, w0, shift, std=(-S, "int"))
    assert neg["std_alignment"] == dict(aligned=0, lag=0, shift=0.0) and bits_equal(neg["T"], -S)


# ---------------------------------------------------------------- the composed cases

@pytest.mark.parametrize("name", sorted(cr.CASES))
def test_composed_case_means_something(name):
    """The conditions on the inputs that test_compose_gpu.py relies on: hot bins
    found (and a capped profile where the case plants one), a non-zero lag that
    the un-repaired cube's template would not give, profiles zapped and kept,
    weights that change when any one option is removed, and no test value within
    100 tolerances of the threshold."""
    assert cr.conditions(name, cr.tolerance(name)) == []


def test_queued_second_archive_means_something():
    """The archive test_compose_gpu.py queues behind case a-chan-128-frac (the
    per-profile case's, from another seed): the same conditions, and another
    hit list and alignment than the first archive's."""
    name, seed = "a-prof-128-frac", cr.QUEUED_SEED
    assert cr.conditions(name, cr.tolerance(name), seed) == []
    d, same = cr.perturbed(name, seed)
    assert same and d <= cr.DELTA
    first, second = cr.reference("a-chan-128-frac"), cr.reference(name, seed)
    assert first["std_alignment"] != second["std_alignment"]
    assert not bits_equal(first["hotbins"]["bins"], second["hotbins"]["bins"])


def test_batch_archives_mean_something():
    """The batch test's three archives: profiles zapped and kept, an alignment
    with a lag, test values clear of the threshold; the one without spikes has
    fewer hot bins than the others."""
    arcs = cr.batch_archives()
    for raw, w0, shift, ref in arcs:
        assert ref["std_alignment"]["aligned"] and ref["std_alignment"]["lag"] != 0
        assert (ref["weights"][w0 != 0] == 0).any() and (ref["weights"] != 0).any()
        t = ref["test"][np.isfinite(ref["test"])]
        assert np.min(np.abs(t - 1.0)) > 100.0 * cr.TOL_DETREND
    assert arcs[1][3]["hotbins"]["total"] < min(arcs[0][3]["hotbins"]["total"], arcs[2][3]["hotbins"]["total"])
    assert not bits_equal(arcs[0][3]["weights"], arcs[2][3]["weights"])


def test_the_start_list_changes_the_test_values():
    a, b = cr.reference("b-pieces-w8"), cr.reference("b-pieces-starts")
    assert not np.array_equal(a["test"], b["test"], equal_nan=True)


def test_tolerance_on_detrended_test_values_is_the_measured_one():
    """Every fftmax scaled by 1 +- 1e-9 (alternating by profile index): the
    weights of every detrended case stay, and the largest change of a test value
    over the cases is DELTA (compose_ref.py; the constant is that figure rounded
    up, so at least 0.9 of it is reached)."""
    detrended = [n for n in sorted(cr.CASES) if cr.CASES[n]["detrend"]]
    assert len(detrended) == len(cr.CASES)     # (every composed case detrends; the plain 1e-9 has no user yet)
    worst = 0.0
    for name in detrended:
        d, same = cr.perturbed(name)
        assert same, "%s: the perturbation changes the weights" % name
        assert d <= cr.DELTA, "%s: |change of a test value| %.3g > DELTA" % (name, d)
        worst = max(worst, d)
    print("largest |change of a test value| %.3g (DELTA %.3g)" % (worst, cr.DELTA))
    assert worst >= 0.9 * cr.DELTA
    assert cr.TOL_DETREND == max(1e-9, 4.0 * cr.DELTA)
