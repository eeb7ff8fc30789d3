"""Opt-in hot-bin repair: the written definition (NumPy) that the kernels of
csrc/ic_hotbins.hip follow bit for bit.

An impulsive interferer that spoils two or three phase bins of a profile drives
up that profile's peak-to-peak and fftmax, and the surgical loop then zaps the
whole profile.  This pass repairs the few bad off-pulse bins first and lets the
loop judge what is left.  It works on the pscrunched f32 cube in the frame the
archive stores it in, once per upload, before the loop reads the cube; every
profile is handled on its own.

How this differs from coast_guard's ``hotbins`` cleaner, which it is modelled
on: coast_guard peels bins off a profile while a normality statistic of the
rest improves, and fills them with random noise.  Here the bins are found by
MAD clipping and filled with the median of the bins that stay, so that the
result is deterministic and can be pinned bit for bit.  Parity with coast_guard
is not pinned by any test.

Parameters
  threshold   finite, > 0: a bin is hot when it lies more than ``threshold``
              scaled MADs from the median
  on_start, on_end   the on-pulse window [on_start, on_end) in the dedispersed
              frame, 0 <= on_start < nbin, 0 <= on_end <= nbin; its length is
              L = (on_end - on_start) mod nbin, so on_end <= on_start wraps
              around and L = 0 means no window (equal ends, and also (0, nbin):
              never the whole profile)
  rounds      1..8 clipping rounds, default 4

Off-pulse set.  Stored bin j of profile (s, c) is on-pulse iff (j - o) mod nbin
lies in the window; o = shift[c] with integer shifts (ded[i] = raw[(i + shift)
% nbin]), 0 for a cube stored dedispersed, and rint(delay[s][c]) (round half
even) mod nbin with fractional delays, where the window is also widened by one
bin on each side (a window of L = 0 stays empty).  O is every other bin;
|O| < 8 is refused.

Skip rule.  A profile with w0 == 0, or with a non-finite sample in O, is left
untouched and has count 0.

Rounds, over the live set V (initially O):
  m    = median of f64(x_j), j in V; an even count gives (a + b) * 0.5 in f64.
         The order is the total order of the bit patterns (-0.0 before +0.0).
  mad  = median of fabs(f64(x_j) - m), by the same rule
  lim  = threshold * (1.4826 * mad)        (two f64 multiplies, no fused form)
  bin j in V is hot iff fabs(f64(x_j) - m) > lim
  stop when mad == 0, when no bin is hot, or after ``rounds``; hot bins leave V.
  (The rounds also stop once more than |O| // 4 bins are flagged: the cap below
  then decides the profile, and V can never run empty.)

Cap.  More than |O| // 4 bins flagged in total: the profile is left untouched
and its count is -1 (it belongs to the surgical cleaner).

Repair.  Otherwise every hot bin becomes f32(m_final), m_final the median of
the surviving V recomputed after the last removal.  On-pulse bins are never
read for the statistics and never written.

The hit list is CSR: the positive counts are the row lengths, profiles in
(s, c) order, bins ascending within a profile.
"""
from __future__ import annotations

import os

import numpy as np

__all__ = ["MIN_OFF", "MAX_ROUNDS", "MAX_NBIN", "SCALE", "normalise", "parse_env", "window", "check_window",
           "on_pulse", "profile_offsets", "repair_profile", "repair_profiles", "repair_cube", "csr_offsets",
           "patch_amps", "patch_pols", "result_dict", "merge_shards"]

MIN_OFF = 8          # fewer off-pulse bins are refused
MAX_ROUNDS = 8
MAX_NBIN = 8192      # k_hotbins holds a profile in one block's registers
SCALE = 1.4826       # MAD -> sigma of a normal distribution
ENV = "IC_HOTBINS"


def parse_env(text):
    """IC_HOTBINS="thr,start,end[,rounds]" -> (thr, start, end, rounds), or None
    for an unset, empty or "0" switch."""
    text = (text or "").strip()
    if text in ("", "0"):
        return None
    parts = [t.strip() for t in text.split(",")]
    if len(parts) not in (3, 4):
        raise ValueError('%s="%s": expected "threshold,on_start,on_end[,rounds]"' % (ENV, text))
    try:
        thr = float(parts[0])
        ints = [int(t) for t in parts[1:]]
    except ValueError:
        raise ValueError('%s="%s": expected "threshold,on_start,on_end[,rounds]" (a number, then integers)'
                         % (ENV, text)) from None
    return normalise((thr,) + tuple(ints))


def normalise(hotbins):
    """A hotbins argument -> (threshold, on_start, on_end, rounds) or None (off).
    None reads the switch IC_HOTBINS; False, 0, () or a threshold <= 0 is off."""
    if hotbins is None:
        return parse_env(os.environ.get(ENV, ""))
    if hotbins is False or (np.isscalar(hotbins) and not hotbins):
        return None
    t = tuple(hotbins)
    if len(t) == 0:
        return None
    if len(t) not in (3, 4):
        raise ValueError("hotbins must be (threshold, on_start, on_end[, rounds]), got %r" % (hotbins,))
    thr = float(t[0])
    for v in t[1:]:
        if isinstance(v, (bool, np.bool_)) or int(v) != v:
            raise ValueError("hotbins: on_start, on_end and rounds must be integers, got %r" % (hotbins,))
    if np.isnan(thr) or np.isinf(thr):
        raise ValueError("hotbins: threshold must be finite, got %r" % thr)
    if thr <= 0:
        return None
    rounds = int(t[3]) if len(t) == 4 else 4
    if rounds < 1 or rounds > MAX_ROUNDS:
        raise ValueError("hotbins: rounds=%d outside 1..%d" % (rounds, MAX_ROUNDS))
    return thr, int(t[1]), int(t[2]), rounds


def window(nbin, on_start, on_end, widen=False):
    """(start, length) of the on-pulse window in the dedispersed frame, widened
    by one bin on each side when asked (never beyond nbin, never from nothing)."""
    length = (int(on_end) - int(on_start)) % nbin
    start = int(on_start)
    if widen and length > 0:
        start = (start - 1) % nbin
        length = min(length + 2, nbin)
    return start, length


def check_window(nbin, on_start, on_end, widen=False):
    """The refusals of ic_set_hotbins that depend on the shape; returns window()."""
    if nbin > MAX_NBIN:
        raise ValueError("hotbins: nbin=%d above %d" % (nbin, MAX_NBIN))
    if not 0 <= on_start < nbin:
        raise ValueError("hotbins: on_start=%d outside [0, %d)" % (on_start, nbin))
    if not 0 <= on_end <= nbin:
        raise ValueError("hotbins: on_end=%d outside [0, %d]" % (on_end, nbin))
    start, length = window(nbin, on_start, on_end, widen)
    if nbin - length < MIN_OFF:
        raise ValueError("hotbins: %d off-pulse bins left of %d (fewer than %d)" % (nbin - length, nbin, MIN_OFF))
    return start, length


def on_pulse(nbin, o, start, length):
    """bool [nbin]: stored bin j is on-pulse iff ((j - o) mod nbin - start) mod
    nbin < length."""
    j = np.arange(nbin, dtype=np.int64)
    return ((j - int(o)) % nbin - start) % nbin < length


def profile_offsets(nsub, nchan, nbin, shift=None, delay=None, input_dedispersed=False):
    """(offsets int64 (nsub, nchan), widen): o of every profile.  delay: the
    fractional delays in bins, (nchan,) or (nsub, nchan) (the window is then
    widened); else shift: the integer shifts (nchan,); a cube stored
    dedispersed has o = 0 and the window as given, whatever its delays."""
    if input_dedispersed:
        return np.zeros((nsub, nchan), np.int64), False
    if delay is not None:
        d = np.asarray(delay, dtype=np.float64)
        d = np.broadcast_to(d if d.ndim == 2 else d[None, :], (nsub, nchan))
        return np.rint(d).astype(np.int64) % nbin, True
    sh = np.mod(np.asarray(shift, dtype=np.int64).reshape(nchan), nbin)
    return np.broadcast_to(sh[None, :], (nsub, nchan)).copy(), False


def _median(v):
    """Median of the f64 values v (no NaN) in the total order of the bit
    patterns; an even count gives (a + b) * 0.5."""
    u = np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)
    top = np.uint64(1) << np.uint64(63)
    key = np.sort(np.where(u & top, ~u, u | top))
    s = np.where(key & top, key & ~top, ~key).view(np.float64)
    n = s.shape[0]
    if n % 2:
        return np.float64(s[n // 2])
    return np.float64((s[n // 2 - 1] + s[n // 2]) * np.float64(0.5))


def repair_profile(x, w, o, start, length, threshold, rounds=4):
    """One profile x [nbin] f32 with weight w and offset o, the window as
    window() gives it -> (repaired copy, count, ascending hot bins)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    nbin = x.shape[0]
    out = x.copy()
    none = np.zeros(0, np.int32)
    off = ~on_pulse(nbin, o, start, length)
    if np.float32(w) == 0:
        return out, 0, none
    x64 = x.astype(np.float64)
    if not np.all(np.isfinite(x64[off])):
        return out, 0, none
    cap = int(off.sum()) // 4
    live = off.copy()
    flagged = np.zeros(nbin, bool)
    thr = np.float64(threshold)
    for _ in range(int(rounds)):
        m = _median(x64[live])
        dev = np.zeros(nbin, np.float64)
        dev[live] = np.fabs(x64[live] - m)
        mad = _median(dev[live])
        if mad == 0:
            break
        lim = thr * (np.float64(SCALE) * mad)
        hot = live & (dev > lim)
        if not hot.any():
            break
        live &= ~hot
        flagged |= hot
        if int(flagged.sum()) > cap:
            break
    n = int(flagged.sum())
    if n > cap:
        return out, -1, none
    if n == 0:
        return out, 0, none
    out[flagged] = np.float32(_median(x64[live]))
    return out, n, np.nonzero(flagged)[0].astype(np.int32)


def csr_offsets(count):
    """int64 [P + 1]: the row starts of the hit list (the positive counts are
    the row lengths)."""
    c = np.asarray(count).reshape(-1).astype(np.int64)
    off = np.zeros(c.shape[0] + 1, np.int64)
    np.cumsum(np.where(c > 0, c, 0), out=off[1:])
    return off


def repair_profiles(profiles, w, offsets, widen, threshold, on_start, on_end, rounds=4):
    """The one-shot ic_hotbins_profiles states: profiles (nprof, nbin) f32, w
    (nprof,), offsets (nprof,) integers (None: 0) -> (out, count int32, bins
    int32 CSR)."""
    p = np.ascontiguousarray(profiles, dtype=np.float32)
    nprof, nbin = p.shape
    start, length = check_window(nbin, on_start, on_end, widen)
    w = np.asarray(w, dtype=np.float32).reshape(nprof)
    offsets = np.zeros(nprof, np.int64) if offsets is None else np.asarray(offsets).reshape(nprof)
    out = np.empty_like(p)
    count = np.zeros(nprof, np.int32)
    bins = []
    for k in range(nprof):
        out[k], count[k], b = repair_profile(p[k], w[k], int(offsets[k]) % nbin, start, length, threshold, rounds)
        bins.append(b)
    return out, count, (np.concatenate(bins) if bins else np.zeros(0, np.int32)).astype(np.int32)


def result_dict(count, bins):
    """The ``hotbins`` entry of a result: count (nsub, nchan) int32, total,
    offsets int64 [P + 1] (CSR row starts), bins int32 [total]."""
    count = np.asarray(count, dtype=np.int32)
    off = csr_offsets(count)
    return dict(count=count, total=int(off[-1]), offsets=off, bins=np.asarray(bins, dtype=np.int32))


def merge_shards(parts):
    """The results of the channel shards of one archive, in rank order (each
    count (nsub, nchan_r)) -> the whole archive's result_dict."""
    count = np.concatenate([np.asarray(p["count"]) for p in parts], axis=1)
    nsub = count.shape[0]
    rows = []
    for s in range(nsub):
        for p in parts:
            nc = np.asarray(p["count"]).shape[1]
            off = np.asarray(p["offsets"])
            rows.append(np.asarray(p["bins"])[off[s * nc]:off[(s + 1) * nc]])
    bins = np.concatenate(rows) if rows else np.zeros(0, np.int32)
    return result_dict(count, bins)


def repair_cube(cube, w0, hotbins, shift=None, delay=None, input_dedispersed=False):
    """What a session with ``hotbins`` set makes of an uploaded cube (nsub,
    nchan, nbin) f32: (repaired cube, result_dict)."""
    cube = np.ascontiguousarray(cube, dtype=np.float32)
    nsub, nchan, nbin = cube.shape
    thr, a, b, rounds = normalise(hotbins)
    offs, widen = profile_offsets(nsub, nchan, nbin, shift, delay, input_dedispersed)
    out, count, bins = repair_profiles(cube.reshape(-1, nbin), np.asarray(w0).reshape(-1), offs.reshape(-1), widen,
                                       thr, a, b, rounds)
    return out.reshape(cube.shape), result_dict(count.reshape(nsub, nchan), bins)


def patch_amps(amps, hot, o, start, length):
    """One polarisation of one listed profile, in place: the bins `hot` of the
    writable f32 amplitudes take the median (the rule above, in f64, stored as
    f32) of the profile's surviving off-pulse bins, O (offset o, the window as
    window() gives it) without `hot`."""
    live = ~on_pulse(amps.shape[0], o, start, length)
    live[hot] = False
    amps[hot] = np.float32(_median(np.asarray(amps[live], dtype=np.float64)))


def patch_pols(data, result, hotbins, shift=None, delay=None, input_dedispersed=False):
    """The full-polarisation host patch: data (nsub, npol, nchan, nbin) f32 is
    patched in place at the bins of the hit list.  For each polarisation the
    listed bins of a profile get that polarisation's own median over the
    profile's surviving off-pulse bins (patch_amps).  Sparse: only listed
    profiles are touched.  Returns the number of profiles patched."""
    nsub, npol, nchan, nbin = data.shape
    thr, a, b, _ = normalise(hotbins)
    offs, widen = profile_offsets(nsub, nchan, nbin, shift, delay, input_dedispersed)
    start, length = check_window(nbin, a, b, widen)
    count = np.asarray(result["count"]).reshape(nsub, nchan)
    rows, bins = np.asarray(result["offsets"]), np.asarray(result["bins"])
    done = 0
    for s, c in np.argwhere(count > 0):
        k = int(s) * nchan + int(c)
        for p in range(npol):
            patch_amps(data[s, p, c], bins[rows[k]:rows[k + 1]], offs[s, c], start, length)
        done += 1
    return done
