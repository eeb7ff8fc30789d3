"""The detrend tests' own yardstick and inputs (no test in here).

combine(): the detrended comprehensive_stats from given diagnostics, stated
with iterative_cleaner_amd.detrend (the definition) and oracle/restated.py's
scalers: every line is detrended (detrend.line_trend / detrended), scaled by
restated.scale_line_masked / scale_line_plain, then restated's max / sort /
NaN rule (restated.comprehensive_stats, lines 156-174) as written there.
"""
import numpy as np

from iterative_cleaner_amd import detrend as dt
from iterative_cleaner_amd import synth
from oracle import restated

PLANTED = ((2, 90), (5, 93), (8, 88), (10, 95))   # (subint, channel) of the 12 x 96 cube: the low-gain end


def combine(diags, valid, chanthresh, subintthresh, detrend=None):
    """diags = (std f64, mean f64, ptp f32 or f64, fftmax f64), each (nsub, nchan);
    valid (nsub, nchan) bool.  Returns (test, chan_coef (4, nchan, 4), subint_coef
    (4, nsub, 4), rounds_used list).  detrend None: zero trends."""
    co, so, rounds, clip = (0, 0, dt.DEFAULT_ROUNDS, dt.DEFAULT_CLIP) if detrend is None else dt.check_params(*detrend)
    valid = np.asarray(valid, dtype=bool)
    nsub, nchan = valid.shape
    scaled = []
    cc = np.zeros((4, nchan, 4), np.float64)
    sc = np.zeros((4, nsub, 4), np.float64)
    used = []
    for q, (D, masked) in enumerate(zip(diags, (True, True, True, False))):
        D = np.asarray(D)
        v = valid if masked else np.ones_like(valid)
        Dc, Ds, cc[q], sc[q], u = dt.detrend_cube(D, v, co, so, rounds, clip)
        used += u
        ch = np.empty((nsub, nchan), np.float64)
        sb = np.empty((nsub, nchan), np.float64)
        for c in range(nchan):
            ch[:, c] = (restated.scale_line_masked(Dc[:, c], valid[:, c], chanthresh) if masked
                        else restated.scale_line_plain(Dc[:, c], chanthresh))
        for s in range(nsub):
            sb[s, :] = (restated.scale_line_masked(Ds[s, :], valid[s, :], subintthresh) if masked
                        else restated.scale_line_plain(Ds[s, :], subintthresh))
        scaled.append(np.maximum(ch, sb))
    st = np.stack(scaled)                                    # (4, nsub, nchan)
    with np.errstate(all="ignore"):
        srt = np.sort(st, axis=0)                            # NaN last
        test = (np.float64(0.0) + srt[1] + srt[2]) / 2.0
        test = np.where(np.isnan(st).any(axis=0), np.nan, test)
    return test, cc, sc, used


def sloped_cube(nsub, nchan, nbin, seed, seed2, planted=PLANTED, slope=3.0, extra=1.5):
    """synth.make_cube with a `slope` x gain slope across the band (gain `slope`
    at channel 0 falling linearly to 1 at the last), and `extra` sigma of further
    noise on the `planted` profiles (the channel's own noise sigma = its gain).
    Returns (raw f32 (nsub, nchan, nbin), w0, shift), read-only."""
    data, w0, shift = synth.make_cube(nsub, nchan, nbin, seed, 0.05)
    gain = np.linspace(slope, 1.0, nchan)
    raw = (data[:, 0].astype(np.float64) * gain[None, :, None])
    rng = np.random.default_rng(seed2)
    for s, c in planted:
        w0[s, c] = 1.0
        raw[s, c] += extra * gain[c] * rng.standard_normal(nbin)
    raw = np.ascontiguousarray(raw.astype(np.float32))
    for a in (raw, w0, shift):
        a.setflags(write=False)
    return raw, w0, shift


def hard_cube(nsub, nchan, nbin, seed):
    """The one-shot tests' cube: a bandpass slope, zero-weight profiles, a whole
    dead channel, a NaN and an Inf sample, a constant channel.  Returns (data
    f32, weights f32)."""
    rng = np.random.default_rng(seed)
    data = rng.standard_normal((nsub, nchan, nbin)).astype(np.float32)
    data *= np.linspace(3.0, 1.0, nchan, dtype=np.float32)[None, :, None]
    data += (0.3 * np.arange(nsub, dtype=np.float32) / max(nsub - 1, 1))[:, None, None]
    w = np.ones((nsub, nchan), np.float32)
    w[rng.random((nsub, nchan)) < 0.1] = 0.0
    if nchan >= 3:
        w[:, 1] = 0.0                      # a dead channel
        data[:, 2, :] = 1.25               # a constant channel
        w[:, 2] = 1.0
    if nchan >= 5:
        data[nsub // 2, 4, 7] = np.nan
        w[nsub // 2, 4] = 1.0
        data[0, 3, 5] = np.inf
        w[0, 3] = 1.0
    return data, w
