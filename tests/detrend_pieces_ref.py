"""The piecewise-detrend tests' own yardstick and inputs (no test in here).

combine(): detrend_ref.combine with pieces: every line is detrended in pieces
(detrend.line_trend_pieces / detrended_pieces, the definition), scaled by
oracle/restated.py's scale_line_masked / scale_line_plain, then restated's max /
sort / NaN rule as detrend_ref.combine writes it.
"""
import numpy as np

from iterative_cleaner_amd import detrend as dt
from iterative_cleaner_amd import synth
from oracle import restated

PERIOD = 16                                            # channels per subband of the teeth cube
PLANTED = ((2, 32), (5, 47), (8, 64), (10, 79))        # (subint, channel) of the 12 x 96 cube: subband edges


def combine(diags, valid, chanthresh, subintthresh, detrend, chan_starts=None, subint_starts=None):
    """diags = (std f64, mean f64, ptp f32 or f64, fftmax f64), each (nsub, nchan);
    valid (nsub, nchan) bool; detrend the (chan, subint[, rounds, clip]) tuple;
    chan_starts / subint_starts: the pieces of a channel line (over the subints)
    and of a subint line (over the channels), None = one piece.  Returns (test,
    chan_coef (4, nchan, mc, 4), subint_coef (4, nsub, ms, 4))."""
    co, so, rounds, clip = dt.check_params(*detrend)
    valid = np.asarray(valid, dtype=bool)
    nsub, nchan = valid.shape
    cb = [0] if chan_starts is None else list(chan_starts)
    sb = [0] if subint_starts is None else list(subint_starts)
    scaled = []
    cc = np.zeros((4, nchan, len(cb), 4), np.float64)
    sc = np.zeros((4, nsub, len(sb), 4), np.float64)
    for q, (D, masked) in enumerate(zip(diags, (True, True, True, False))):
        D = np.asarray(D)
        v = valid if masked else np.ones_like(valid)
        Dc, Ds, cc[q], sc[q], _ = dt.detrend_cube_pieces(D, v, co, so, cb, sb, rounds, clip)
        ch = np.empty((nsub, nchan), np.float64)
        sbv = np.empty((nsub, nchan), np.float64)
        for c in range(nchan):
            ch[:, c] = (restated.scale_line_masked(Dc[:, c], valid[:, c], chanthresh) if masked
                        else restated.scale_line_plain(Dc[:, c], chanthresh))
        for s in range(nsub):
            sbv[s, :] = (restated.scale_line_masked(Ds[s, :], valid[s, :], subintthresh) if masked
                         else restated.scale_line_plain(Ds[s, :], subintthresh))
        scaled.append(np.maximum(ch, sbv))
    st = np.stack(scaled)                                    # (4, nsub, nchan)
    with np.errstate(all="ignore"):
        srt = np.sort(st, axis=0)                            # NaN last
        test = (np.float64(0.0) + srt[1] + srt[2]) / 2.0
        test = np.where(np.isnan(st).any(axis=0), np.nan, test)
    return test, cc, sc


def tooth_gain(nchan, period=PERIOD, top=3.0):
    """The polyphase-like bandpass: a parabola per subband of `period` channels,
    gain 1 at its two edge channels and `top` in the middle."""
    u = (np.arange(nchan) % period) / float(period - 1)      # 0 .. 1 across a subband
    return 1.0 + (top - 1.0) * (1.0 - (2.0 * u - 1.0) ** 2)


def teeth_cube(nsub, nchan, nbin, seed, seed2, planted=PLANTED, extra=1.0):
    """synth.make_cube under tooth_gain, with `extra` sigma of further noise on
    the `planted` profiles (the channel's own noise sigma = its gain).  Returns
    (raw f32 (nsub, nchan, nbin), w0, shift), read-only."""
    data, w0, shift = synth.make_cube(nsub, nchan, nbin, seed, 0.05)
    gain = tooth_gain(nchan)
    raw = data[:, 0].astype(np.float64) * gain[None, :, None]
    rng = np.random.default_rng(seed2)
    for s, c in planted:
        w0[s, c] = 1.0
        raw[s, c] += extra * gain[c] * rng.standard_normal(nbin)
    raw = np.ascontiguousarray(raw.astype(np.float32))
    for a in (raw, w0, shift):
        a.setflags(write=False)
    return raw, w0, shift
