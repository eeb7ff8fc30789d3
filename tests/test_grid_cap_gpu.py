"""Every grid-stride kernel loop past its first trip, at small sizes.

The launchers cap their grids (4096 blocks for k_diag_p2 / k_diag_cl, 8192 for
k_diag, 16384 waves for k_rotate / k_base / k_residual, 65536 for k_fit_tail),
so a wave group takes a second profile only on archives of tens of thousands
of profiles, and k_diag_cl refills its 64-slot window only past 2 M profiles.
Session option grid_cap (IC_OPT_GRID_CAP) caps every such grid: with grid_cap
= 1 one block walks the whole archive, and the state the loops carry from one
profile to the next (the prefetched row and scalars of k_diag_p2, the slot
window of k_diag_cl, the wave-private LDS of k_diag, k_rotate's block-uniform
`continue`) is exercised hundreds of times by a few-hundred-profile archive.

Every case compares a grid_cap in {1, 3} run with the C oracle's clean_loop,
as test_gpu_parity.test_loop_matches_c_oracle does (loops, changed, nzero
equal; weights, amp, info, std, mean, ptp, template and residual bit-equal;
fftmax within 1e-9 relative, test values within 1e-9), and with the grid_cap
= 0 run of the same session bit for bit (a profile's arithmetic does not
depend on the group that computes it).

Shapes: (7, 152, nbin) for nbin <= 1024, where 8 one-wave groups per block
take 133 profiles each (two full windows of k_diag_cl and a ragged third; 1064
is no multiple of 8 x 64), and (5, 53, nbin) for 2048 / 4096, one group per
block, 265 profiles.  RFI fraction 0.25; the synthetic cube has zero-weight
channels, and the middle subint is all zero.  The two-shard cases need two
256-channel super-blocks: (3, 300, nbin).

k_fit_tail under a cap of one block fits the whole archive a few profiles at a
time (about a second per run at 1024 bins), so only
test_integer_shifts_exact_fit, one schedule per case, hands the fit to it; the
other tests fit by rounds, which is also what reaches the fork round.

Which kernel instantiation each case is for:

  test_integer_shifts_exact_fit      k_diag_p2<64..512, EXACT>, k_diag (100,
                                     1000), k_diag_cl<1024..4096, EXACT>; with
                                     the fork their list and skip passes,
                                     k_mark_list, k_fit_tail's slot loop;
                                     k_base, k_residual, k_combine everywhere
  test_row_layout_at_chain_sizes     k_diag_p2<1024>, multi-wave
                                     k_diag_p2<2048 / 4096> (diag_chain = 0,
                                     and the pulse region)
  test_f64_data                      k_diag<D64> (100), k_diag_p2<128 / 1024 /
                                     2048, EXACT, D64>
  test_closed_form                   k_diag (100), k_diag_p2<256, CLOSED>,
                                     k_diag_cl<1024 / 4096, CLOSED>,
                                     k_diag_p2<1024, CLOSED> (diag_chain = 0)
  test_fft_dedispersion              k_rotate<64..4096, per channel / per
                                     profile> with flags, late and list item
                                     orders, k_diag_p2<N, STATS>,
                                     k_diag_cl<N, STATS>, k_rotate<1024, *,
                                     stats>
  test_fft_dedispersion_variants     pulse region, k_diag_p2<N, STATS, D64>,
                                     k_rotate_identity, k_diag_p2<128 / 1024,
                                     FIT> (the early `continue`)
  test_uploads_under_the_cap         k_pscrunch, k_decode_q, k_decode_q_scalar
  test_shards_under_the_cap          k_pack_rows, k_assemble_rows and the
                                     shard sessions' launches
"""
import numpy as np
import pytest

from helpers import bits_equal

pytestmark = pytest.mark.gpu

FFT_RTOL = 1e-9     # the project's bounds (test_gpu_parity)
TEST_ATOL = 1e-9
CAPS = (1, 3)
TAIL_ONLY = 1 << 40
TAIL_MIXED = 256     # below every archive's profile count: the tail takes over after the first rounds
RFI = 0.25
PULSE = [0.25, 40, 90]

_ARCHIVES = {}
_ORACLE = {}


def _shape(nbin):
    return (7, 152, nbin) if nbin <= 1024 else (5, 53, nbin)


def _archive(nbin):
    """(raw, w0, shift) of the size's archive: read-only, shared by the tests."""
    if nbin not in _ARCHIVES:
        _ARCHIVES[nbin] = _make_archive(_shape(nbin))
    return _ARCHIVES[nbin]


def _make_archive(shape):
    from iterative_cleaner_amd import synth
    nsub, nchan, nbin = shape
    data, w0, shift = synth.make_cube(nsub, nchan, nbin, 700 + nbin, RFI)
    raw = np.ascontiguousarray(data[:, 0])
    raw[nsub // 2] = 0.0                               # a subint of zeros
    assert (w0 == 0).all(axis=0).any() and (w0 != 0).any()   # zero-weight channels
    for a in (raw, w0, shift):
        a.setflags(write=False)
    return raw, w0, shift


def _delay(nbin, kind):
    from iterative_cleaner_amd import synth
    nsub = _shape(nbin)[0]
    shift = _archive(nbin)[2]
    if kind is None:
        return None
    return synth.per_profile_delays(shift, nbin, nsub) if kind == "pp" else synth.fractional_delays(shift, nbin)


def _oracle(oracle_lib, nbin, fit_mode=0, data_f64=False, delay=None, pulse=False, input_dedispersed=False):
    """The C oracle's loop on the size's archive, computed once per configuration."""
    key = (nbin, fit_mode, data_f64, delay, pulse, input_dedispersed)
    if key not in _ORACLE:
        from iterative_cleaner_amd import _native
        raw, w0, shift = _archive(nbin)
        pr = None
        if pulse:
            _, fac, a, b = _native.normalise_pulse_region(PULSE, nbin)
            pr = (fac, a, b)
        ref = oracle_lib.clean_loop(raw, w0, shift, 5.0, 5.0, 5, pr, want_residual=True, want_details=True,
                                    fit_mode=fit_mode, data_f64=data_f64, delay=_delay(nbin, delay),
                                    input_dedispersed=input_dedispersed)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _ORACLE[key] = ref
    return _ORACLE[key]


def _session(nbin, fit_mode=0, data_f64=False, delay=None, pulse=False, input_dedispersed=False, options=None):
    from iterative_cleaner_amd import _native
    nsub, nchan, _ = _shape(nbin)
    return _native.GpuSession(nsub, nchan, nbin, 5, 5.0, 5.0, PULSE if pulse else (0, 0, 1), device=0,
                              fit_mode=fit_mode, data_f64=data_f64, delay=_delay(nbin, delay),
                              input_dedispersed=input_dedispersed, options=options)


def _upload(s, nbin, fft, other=False):
    """The size's archive, or (other) a different cube of the same shape."""
    raw, w0, shift = _archive(nbin)
    if other:
        raw = raw * np.float32(3.0) + np.float32(1.0)
    s.upload(raw, w0, np.zeros_like(shift) if fft else shift)


def _results(s):
    out = s.run()
    out["amp"], out["info"] = s.fit()
    out["std"], out["mean"], out["ptp"], out["fft"] = s.diagnostics()
    out["T"] = s.template()
    out["residual"] = s.residual()
    out["stats"] = s.run_stats()
    return out


def _capped_results(s, nbin, fft, cap):
    """The results under grid_cap = cap.  A loop that left profiles out would
    leave their outputs as the previous run wrote them, which after a run on
    the same archive are the right values: a run on another cube comes first."""
    s.set_option("grid_cap", 0)
    _upload(s, nbin, fft, other=True)
    s.run(fetch=False)
    _upload(s, nbin, fft)
    s.set_option("grid_cap", cap)
    assert s.get_option("grid_cap") == cap
    return _results(s)


def _close_fft(a, b):
    both_nan = np.isnan(a) & np.isnan(b)
    return bool((both_nan | (np.abs(a - b) <= FFT_RTOL * np.maximum(np.abs(b), 1e-300)) | (a == b)).all())


def _close_test(a, b):
    both_nan = np.isnan(a) & np.isnan(b)
    same_inf = np.isinf(a) & np.isinf(b) & (np.sign(a) == np.sign(b))
    fin = np.isfinite(a) & np.isfinite(b)
    return bool((both_nan | same_inf | (fin & (np.abs(a - b) <= TEST_ATOL * np.maximum(1.0, np.abs(b))))).all())


def _check_oracle(got, ref, what):
    k = got["n_iter"]
    assert got["loops"] == ref["loops"], what
    assert np.array_equal(got["changed"], ref["changed"][:k]), what
    assert np.array_equal(got["nzero"], ref["nzero"][:k]), what
    assert bits_equal(got["weights"], ref["weights"]), (what, "weights")
    assert bits_equal(got["T"], ref["T"][k - 1]), (what, "template")
    for name in ("amp", "info", "std", "mean", "ptp"):
        assert bits_equal(got[name], ref[name]), (what, name, int((got[name] != ref[name]).sum()))
    assert _close_fft(got["fft"], ref["fft"]), (what, "fftmax")
    assert _close_test(got["test"], ref["test"]), (what, "test")
    with np.errstate(invalid="ignore"):
        assert np.array_equal(got["test"] >= 1.0, ref["test"] >= 1.0), (what, "zap decisions")
    assert bits_equal(got["residual"], ref["residual"]), (what, "residual")


def _check_same(got, base, what):
    """Bit for bit the run with the launchers' own grids, fftmax and test values included."""
    assert got["loops"] == base["loops"] and got["n_iter"] == base["n_iter"], what
    assert np.array_equal(got["changed"], base["changed"]) and np.array_equal(got["nzero"], base["nzero"]), what
    for name in ("weights", "test", "T", "amp", "info", "std", "mean", "ptp", "fft", "residual"):
        assert bits_equal(got[name], base[name]), (what, name)


def _sweep(s, nbin, fft, ref, schedules, exact=True):
    """Every schedule (a dict of options, `fit_tail`: the tail threshold or None
    for the session's default) with grid_cap 0, 1 and 3 on the size's archive."""
    default_tail = s.get_option("fit_tail")
    for sched in schedules:
        opts = dict(sched)
        tail = opts.pop("fit_tail", None)
        s.set_fit_tail(default_tail if tail is None else tail)
        for name, value in opts.items():
            s.set_option(name, value)
        runs = {}
        for cap in (0,) + CAPS:
            runs[cap] = _capped_results(s, nbin, fft, cap)
        for cap in CAPS:
            what = (sched, "grid_cap=%d" % cap)
            _check_oracle(runs[cap], ref, what)
            _check_same(runs[cap], runs[0], what)
            st = runs[cap]["stats"]
            if exact and tail == 0:          # rounds only
                assert st["fit_tail_sweeps"] == 0 and st["fit_profile_sweeps"] > 0, what
            elif exact and tail == TAIL_ONLY:
                assert st["fit_profile_sweeps"] == 0 and st["fit_tail_sweeps"] > 0, what
            elif exact and tail == TAIL_MIXED:   # rounds, then the tail on the survivors' list
                assert st["fit_profile_sweeps"] > 0 and st["fit_tail_sweeps"] > 0, what


def _fork_schedules(forks=(0, 3), tails=(0,), **more):
    """Rounds only by default, so that the fork round is reached: k_fit_tail
    under a cap of one block fits the archive's profiles a few at a time, a
    second per run (test_integer_shifts_exact_fit covers its loop at every size)."""
    return [dict(diag_fork=f, fit_tail=t, **more) for f in forks for t in tails]


TAILS = {"rounds": 0, "tail": TAIL_ONLY, "default": None, "mixed": TAIL_MIXED}
SCHEDULES = [(f, t) for f in (0, 1, 3) for t in ("rounds", "tail", "default")] + [(1, "mixed")]


@pytest.mark.parametrize("fork,tail", SCHEDULES, ids=lambda v: str(v))
@pytest.mark.parametrize("nbin", [64, 128, 256, 512, 100, 1000, 1024, 2048, 4096])
def test_integer_shifts_exact_fit(nbin, fork, tail, oracle_lib):
    """Integer shifts, exact fit, f32 data: every fork round with the rounds-only,
    tail-only and default schedules (archives this small go to the tail at once
    by default).  "mixed": a hand-over to the tail after the fork round, which
    puts k_fit_tail on a survivor list and, with tail_split (both settings at
    2048), runs k_mark_list and the skip pass beside it."""
    ref = _oracle(oracle_lib, nbin)
    splits = (0, 1) if tail == "mixed" and nbin == 2048 else (2,)
    with _session(nbin) as s:
        _sweep(s, nbin, False, ref, [dict(diag_fork=fork, fit_tail=TAILS[tail], tail_split=sp) for sp in splits])


@pytest.mark.parametrize("pulse", [False, True], ids=["chain0", "pulse"])
@pytest.mark.parametrize("nbin", [1024, 2048, 4096])
def test_row_layout_at_chain_sizes(nbin, pulse, oracle_lib):
    """diag_chain = 0, or a pulse region, sends 1024 / 2048 / 4096 to k_diag_p2."""
    ref = _oracle(oracle_lib, nbin, pulse=pulse)
    with _session(nbin, pulse=pulse, options=None if pulse else {"diag_chain": 0}) as s:
        _sweep(s, nbin, False, ref, _fork_schedules())


@pytest.mark.parametrize("nbin", [100, 128, 1024, 2048])
def test_f64_data(nbin, oracle_lib):
    ref = _oracle(oracle_lib, nbin, data_f64=True)
    with _session(nbin, data_f64=True) as s:
        _sweep(s, nbin, False, ref, _fork_schedules())


@pytest.mark.parametrize("nbin,chain", [(100, 1), (256, 1), (1024, 1), (4096, 1), (1024, 0)])
def test_closed_form(nbin, chain, oracle_lib):
    from iterative_cleaner_amd import _native
    ref = _oracle(oracle_lib, nbin, fit_mode=1)
    with _session(nbin, fit_mode=_native.FIT_CLOSED, options={"diag_chain": chain}) as s:
        with pytest.raises(_native.NativeError, match="DIAG_FORK"):   # the fork serves the exact fit only
            s.set_option("diag_fork", 3)
        _sweep(s, nbin, False, ref, [dict(diag_fork=0)], exact=False)


@pytest.mark.parametrize("kind", ["chan", "pp"])
@pytest.mark.parametrize("nbin", [64, 128, 256, 512, 1024, 2048, 4096])
def test_fft_dedispersion(nbin, kind, oracle_lib):
    """FFT dedispersion, exact fit: k_rotate's item loop in both item orders
    (the late flags of a channel's phasor table, the survivor list of
    per-profile delays) and the statistics of the rotated residual; at 1024
    the rotation that measures its rows against rotation + k_diag_cl<STATS>."""
    ref = _oracle(oracle_lib, nbin, delay=kind)
    scheds = []
    for rs in ((0, 1) if nbin == 1024 else (1,)):
        scheds += _fork_schedules(rot_stats=rs)
    with _session(nbin, delay=kind) as s:
        _sweep(s, nbin, True, ref, scheds)


FFT_VARIANTS = {
    "pulse-256": (256, dict(delay="chan", pulse=True)),
    "pulse-2048": (2048, dict(delay="pp", pulse=True)),
    "f64-128": (128, dict(delay="chan", data_f64=True)),
    "f64-1024": (1024, dict(delay="pp", data_f64=True)),
    "stored-dedispersed-512": (512, dict(delay="chan", input_dedispersed=True)),
    "stored-dedispersed-1024": (1024, dict(delay="pp", input_dedispersed=True)),
    "closed-128": (128, dict(delay="chan", fit_mode=1)),
    "closed-1024": (1024, dict(delay="pp", fit_mode=1)),
}


@pytest.mark.parametrize("name", sorted(FFT_VARIANTS))
def test_fft_dedispersion_variants(name, oracle_lib):
    nbin, kw = FFT_VARIANTS[name]
    ref = _oracle(oracle_lib, nbin, **kw)
    closed = kw.get("fit_mode", 0) == 1
    scheds = [dict(diag_fork=0)] if closed else _fork_schedules()
    with _session(nbin, **kw) as s:
        _sweep(s, nbin, True, ref, scheds, exact=not closed)


def _pols(nbin, npol):
    """(data (nsub, npol, nchan, nbin), w0, shift) with pol 1 perturbed, so that
    pol 0 + pol 1 rounds (synth splits the cube into two halves that sum exactly)."""
    from iterative_cleaner_amd import synth
    nsub, nchan, _ = _shape(nbin)
    data, w0, shift = synth.make_cube(nsub, nchan, nbin, 900 + nbin, RFI, npol=npol)
    rng = np.random.default_rng(901 + nbin)
    data[:, 1] += (0.37 * rng.standard_normal(data[:, 1].shape)).astype(np.float32)
    return data, w0, shift


@pytest.mark.parametrize("nbin", [128, 100])
def test_uploads_under_the_cap(nbin):
    """upload_pols (k_pscrunch) and upload_quantised (k_decode_q at nbin % 8 == 0,
    k_decode_q_scalar otherwise; native and FITS byte order; one and two summed
    polarisations) under grid_cap 1 and 3: every result, the residual cube
    included (every sample of the cube enters it), equals the plain session's
    on the host-prepared f32 cube."""
    from iterative_cleaner_amd import _native, psrfits
    nsub, nchan, _ = _shape(nbin)
    for npol in (2, 4):
        data, w0, shift = _pols(nbin, npol)
        q, scl, offs = psrfits.quantise(data)
        dec = psrfits.decode(q, scl, offs)
        hosts = {"pols": np.ascontiguousarray((data[:, 0] + data[:, 1]).astype(np.float32)),
                 1: np.ascontiguousarray(dec[:, 0]),
                 2: np.ascontiguousarray((dec[:, 0] + dec[:, 1]).astype(np.float32))}
        other = hosts["pols"] * np.float32(3.0) + np.float32(1.0)
        refs = {}
        with _native.GpuSession(nsub, nchan, nbin, device=0) as s:
            for key, cube in hosts.items():
                s.upload(cube, w0, shift)
                refs[key] = _results(s)
        assert not bits_equal(refs[1]["residual"], refs[2]["residual"])
        for cap in CAPS:
            with _native.GpuSession(nsub, nchan, nbin, device=0, options={"grid_cap": cap}) as s:
                s.upload(other, w0, shift)
                s.upload_pols(data, w0, shift)
                _check_same(_results(s), refs["pols"], (npol, cap, "upload_pols"))
                for nsum in (1, 2):
                    for samples in (q, q.astype(">i2")):
                        s.upload(other, w0, shift)   # a decode that left samples out would show them
                        s.upload_quantised(samples, scl, offs, w0, shift, nsum)
                        _check_same(_results(s), refs[nsum], (npol, cap, nsum, samples.dtype.str))


SHARD_SHAPE = (3, 300)   # two 256-channel super-blocks: the fewest channels two shards can split


@pytest.mark.parametrize("nbin,fft", [(256, False), (1024, True)], ids=["256", "1024-fft"])
def test_shards_under_the_cap(nbin, fft, oracle_lib):
    """World 2, in process, every shard under grid_cap 1 (the exact fit by
    rounds, k_fit_tail's loop is test_integer_shifts_exact_fit's): the merged
    result is the unsharded session's and the oracle's."""
    from iterative_cleaner_amd import _native, sharded, synth
    nsub, nchan = SHARD_SHAPE
    raw, w0, shift = _make_archive(SHARD_SHAPE + (nbin,))
    delay = synth.fractional_delays(shift, nbin) if fft else None
    ref = oracle_lib.clean_loop(raw, w0, shift, want_details=True, delay=delay)
    sh = np.zeros_like(shift) if fft else shift
    with _native.GpuSession(nsub, nchan, nbin, device=0, delay=delay) as s:
        s.upload(raw, w0, sh)
        one = _results(s)
    kw = {"delay": delay} if fft else {}
    out = sharded.clean_cube_local(raw, w0, sh, 2, want_details=True, fit_tail=0, options={"grid_cap": 1}, **kw)
    assert out["loops"] == one["loops"] == ref["loops"]
    assert np.array_equal(out["changed"], one["changed"]) and np.array_equal(out["nzero"], one["nzero"])
    for name in ("weights", "test", "T", "amp", "info", "std", "mean", "ptp", "fft"):
        assert bits_equal(out[name], one[name]), name
    for name in ("weights", "amp", "info", "std", "mean", "ptp"):
        assert bits_equal(out[name], ref[name]), name
    assert _close_fft(out["fft"], ref["fft"]) and _close_test(out["test"], ref["test"])
