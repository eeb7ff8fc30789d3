"""Opt-in dynamic spectrum: the written definition (NumPy) that the kernels of
csrc/ic_dynspec.hip follow bit for bit.

The dynamic spectrum is the pulsar's flux and its uncertainty per (subint,
channel), with the zapped profiles masked: what scintillation studies take from
a cleaned archive.  When a cleaning run returns, the session still holds the
cube, the final template, the final weights and the dedispersion, so one more
pass over the resident cube gives it (ic_get_dynspec; GpuSession.dynspec()).

It is modelled on psrchive's ``psrflux``, which fits a template with a free
baseline to every profile.  Parity with psrchive is not pinned by any test: the
template here is the cleaner's own (or the aligned standard), the sums are
ordered as below, and no flux calibration is applied.

Inputs, per profile (s, c)
  xd   the dedispersed f32 samples of the cube the last run consumed (pscrunched,
       and hot-bin-repaired where that mode is on), nbin of them: with integer
       shifts xd[i] = raw[(i + shift[c]) % nbin]; with fractional delays the
       rotated view rot(raw) (phase_rotation.rotate, sign +1, no baseline); a
       cube stored dedispersed as it is.
  T    the template, f32 [nbin], as ic_get_template returns it after that run
  w    the last iteration's weight of the profile
No baseline is removed first, and the pulse region plays no part.

One summation rule for every sum, sum64(v): 64 chains; chain l starts at +0.0
and adds v[l], v[l + 64], ... in ascending order; then the halving tree c[l] =
c[l] + c[l + h] for l < h, h = 32, 16, 8, 4, 2, 1; the result is c[0].
Everything is f64, every product is rounded on its own (no fused multiply-add),
and / and sqrt are the IEEE operations.

Once per template
  mT  = sum64(f64(T)) / nbin
  t_i = f64(T_i) - mT
  Stt = sum64(t_i * t_i)

Per profile with w != 0
  x_i = f64(xd_i)
  mx  = sum64(x) / nbin
  amp = sum64(t_i * x_i) / Stt       free-baseline least squares (sum t = 0
                                     decouples the baseline)
  base = mx - amp * mT
  r_i = (x_i - mx) - amp * t_i
  err = sqrt(sum64(r_i * r_i) / (nbin - 2)) / sqrt(Stt)

Rules.  A profile with w == 0 has amp = err = base = +0.0 and its samples are
never read (a NaN in a zapped row does not reach the output).  Non-finite
samples and a constant template (Stt == 0) are not special-cased: whatever IEEE
gives is the answer.  nbin < 4 is refused.
"""
from __future__ import annotations

import os

import numpy as np

__all__ = ["MIN_NBIN", "LANES", "ENV", "sum64", "template_terms", "profiles", "dedispersed", "cube", "normalise",
           "parse_env", "merge_shards", "final_weights", "archive_axes", "save", "load"]

MIN_NBIN = 4
LANES = 64           # the chains of sum64: one per lane of a wave
ENV = "IC_DYNSPEC"
KEYS = ("amp", "err", "base")


def sum64(v):
    """sum64 over the last axis of the f64 values v (..., n) -> (...)."""
    v = np.asarray(v, dtype=np.float64)
    n = v.shape[-1]
    c = np.zeros(v.shape[:-1] + (LANES,), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(0, n, LANES):
            m = min(LANES, n - j)
            c[..., :m] = c[..., :m] + v[..., j:j + m]
        h = LANES // 2
        while h >= 1:
            c = c[..., :h] + c[..., h:2 * h]
            h //= 2
    return c[..., 0]


def _check_template(T):
    T = np.ascontiguousarray(T, dtype=np.float32)
    if T.ndim != 1:
        raise ValueError("dynspec: the template must be (nbin,), got shape %s" % (T.shape,))
    if T.shape[0] < MIN_NBIN:
        raise ValueError("dynspec: nbin=%d below %d" % (T.shape[0], MIN_NBIN))
    return T


def template_terms(T):
    """(mT, t f64 [nbin], Stt) of the template T f32 [nbin]."""
    T = _check_template(T)
    nbin = T.shape[0]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        mT = sum64(T.astype(np.float64)) / np.float64(nbin)
        t = T.astype(np.float64) - mT
        Stt = sum64(t * t)
    return np.float64(mT), t, np.float64(Stt)


def profiles(T, xd, w):
    """The one-shot ic_dynspec_profiles states: T (nbin,) f32, xd (nprof, nbin)
    f32 dedispersed profiles, w (nprof,) -> dict(amp, err, base), f64 (nprof,)."""
    T = _check_template(T)
    nbin = T.shape[0]
    xd = np.asarray(xd)
    if xd.ndim != 2 or xd.shape[1] != nbin:
        raise ValueError("dynspec: profiles must be (nprof, %d), got shape %s" % (nbin, xd.shape))
    nprof = xd.shape[0]
    w = np.asarray(w, dtype=np.float32)
    if w.size != nprof:
        raise ValueError("dynspec: %d weights for %d profiles" % (w.size, nprof))
    live = w.reshape(nprof) != 0
    out = {k: np.zeros(nprof, np.float64) for k in KEYS}
    if not live.any():
        return out
    mT, t, Stt = template_terms(T)
    n = np.float64(nbin)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        x = np.asarray(xd[live], dtype=np.float32).astype(np.float64)   # zapped rows are never read
        mx = sum64(x) / n
        a = sum64(t * x) / Stt
        b = mx - a * mT
        r = (x - mx[:, None]) - a[:, None] * t
        e = np.sqrt(sum64(r * r) / np.float64(nbin - 2)) / np.sqrt(Stt)
    out["amp"][live], out["err"][live], out["base"][live] = a, e, b
    return out


def dedispersed(cube, shift=None, delay=None, input_dedispersed=False, any_length=None):
    """The dedispersed view xd (nsub, nchan, nbin) f32 of a cube as a session
    holds it: gathered by the integer shifts (nchan,), rotated by the fractional
    delays (nchan,) or (nsub, nchan) (phase_rotation.rotate; any_length as
    there), or as it is when stored dedispersed."""
    cube = np.asarray(cube, dtype=np.float32)
    if cube.ndim != 3:
        raise ValueError("dynspec: the cube must be (nsub, nchan, nbin), got shape %s" % (cube.shape,))
    nsub, nchan, nbin = cube.shape
    if input_dedispersed:
        return cube
    if delay is not None:
        from . import phase_rotation as pr
        d = np.asarray(delay, dtype=np.float64)
        if d.shape not in ((nchan,), (nsub, nchan)):
            raise ValueError("dynspec: delays must be (%d,) or (%d, %d), got shape %s" % (nchan, nsub, nchan, d.shape))
        return np.ascontiguousarray(pr.rotate(cube, pr.phasors(nbin, d), +1, any_length=any_length), dtype=np.float32)
    if shift is None:
        return cube
    sh = np.mod(np.asarray(shift, dtype=np.int64).reshape(nchan), nbin)
    idx = (np.arange(nbin, dtype=np.int64)[None, :] + sh[:, None]) % nbin
    return np.take_along_axis(cube, np.broadcast_to(idx[None], cube.shape), axis=2)


def cube(cube, T, w, shift=None, delay=None, input_dedispersed=False, any_length=None):
    """What a session returns (ic_get_dynspec) for a cube (nsub, nchan, nbin)
    f32, the template T and the weights w (nsub, nchan): dict(amp, err, base),
    f64 (nsub, nchan).  shift / delay / input_dedispersed: dedispersed()'s."""
    cube = np.asarray(cube, dtype=np.float32)
    if cube.ndim != 3:
        raise ValueError("dynspec: the cube must be (nsub, nchan, nbin), got shape %s" % (cube.shape,))
    nsub, nchan, nbin = cube.shape
    w = np.asarray(w, dtype=np.float32)
    if w.shape != (nsub, nchan):
        raise ValueError("dynspec: weights must be (%d, %d), got shape %s" % (nsub, nchan, w.shape))
    T = _check_template(T)
    if T.shape[0] != nbin:
        raise ValueError("dynspec: a template of %d bins for profiles of %d" % (T.shape[0], nbin))
    xd = dedispersed(cube, shift, delay, input_dedispersed, any_length)
    res = profiles(T, xd.reshape(-1, nbin), w.reshape(-1))
    return {k: v.reshape(nsub, nchan) for k, v in res.items()}


def parse_env(text):
    """IC_DYNSPEC -> None (off: unset, empty or "0"), True ("1": the default
    file name "<ar_name>.dynspec") or the path."""
    text = (text or "").strip()
    if text in ("", "0"):
        return None
    return True if text == "1" else text


def normalise(dynspec):
    """A dynspec argument -> None (off), True (on; clean() writes
    "<ar_name>.dynspec") or a path (str).  None reads the switch IC_DYNSPEC;
    False, 0 and "" are off."""
    if dynspec is None:
        return parse_env(os.environ.get(ENV, ""))
    if isinstance(dynspec, (bool, np.bool_)):
        return True if dynspec else None
    if isinstance(dynspec, (int, np.integer)):
        if dynspec in (0, 1):
            return True if dynspec else None
        raise ValueError("dynspec must be a switch or a path, got %r" % (dynspec,))
    if isinstance(dynspec, os.PathLike):
        dynspec = os.fspath(dynspec)
    if isinstance(dynspec, str):
        return parse_env(dynspec)
    raise ValueError("dynspec must be a switch or a path, got %r" % (dynspec,))


def merge_shards(parts):
    """The results of the channel shards of one archive, in rank order (each
    (nsub, nchan_r)) -> the whole archive's dict(amp, err, base)."""
    parts = list(parts)
    if not parts:
        raise ValueError("dynspec: no shard results to merge")
    return {k: np.ascontiguousarray(np.concatenate([np.asarray(p[k], dtype=np.float64) for p in parts], axis=1))
            for k in KEYS}


def final_weights(ar):
    """The (nsub, nchan) weights of an archive object as they stand."""
    return np.asarray(ar.get_weights(), dtype=np.float64)


def archive_axes(ar):
    """(freq_MHz (nsub, nchan), time_min (nsub,)) of an archive object: the
    centre frequency of every channel and the subints' mid times in minutes
    since the archive's start, where the object offers them (psrchive's
    Integration.get_centre_frequency(ichan), get_epoch() and start_time()); NaN
    where it does not."""
    nsub, nchan = int(ar.get_nsubint()), int(ar.get_nchan())
    freq = np.full((nsub, nchan), np.nan)
    tmin = np.full(nsub, np.nan)
    try:
        t0 = ar.start_time().in_days()
    except Exception:
        t0 = None
    for s in range(nsub):
        integ = ar.get_Integration(s)
        if hasattr(integ, "get_centre_frequency"):
            try:
                freq[s] = [float(integ.get_centre_frequency(c)) for c in range(nchan)]
            except Exception:
                freq[s] = np.nan
        if t0 is not None and hasattr(integ, "get_epoch"):
            try:
                tmin[s] = (float(integ.get_epoch().in_days()) - float(t0)) * 1440.0
            except Exception:
                tmin[s] = np.nan
    return freq, tmin


MAGIC = "# dynspec 1"
COLUMNS = "isub ichan amp err freq_MHz time_min"


def _g(v):
    return "%.17g" % v


def save(path, result, mask_weights, meta=None):
    """Write the dynamic spectrum as text.  result: dict(amp, err[, base]) of
    (nsub, nchan); mask_weights (nsub, nchan): a profile whose weight is 0 is
    written as zeros; meta: dict with any of archive (name), nbin, template
    (where the template came from), freq_MHz (nsub, nchan) or (nchan,),
    time_min (nsub,).  '#' header lines (archive name, shape, template source,
    number of masked profiles, columns), then one line per profile: isub ichan
    amp err freq_MHz time_min, the numbers in %.17g (a NaN is written as nan)."""
    meta = dict(meta or {})
    amp = np.asarray(result["amp"], dtype=np.float64)
    err = np.asarray(result["err"], dtype=np.float64)
    if amp.ndim != 2 or err.shape != amp.shape:
        raise ValueError("dynspec.save: amp and err must be (nsub, nchan), got %s and %s" % (amp.shape, err.shape))
    nsub, nchan = amp.shape
    mw = np.asarray(mask_weights)
    if mw.shape != (nsub, nchan):
        raise ValueError("dynspec.save: mask weights must be (%d, %d), got %s" % (nsub, nchan, mw.shape))
    masked = mw == 0
    amp = np.where(masked, 0.0, amp)
    err = np.where(masked, 0.0, err)
    freq = meta.get("freq_MHz")
    freq = np.full((nsub, nchan), np.nan) if freq is None else np.broadcast_to(
        np.asarray(freq, dtype=np.float64), (nsub, nchan))
    tmin = meta.get("time_min")
    tmin = np.full(nsub, np.nan) if tmin is None else np.asarray(tmin, dtype=np.float64).reshape(nsub)
    lines = [MAGIC,
             "# archive: %s" % str(meta.get("archive", "")).replace("\n", " "),
             "# shape: %d %d %d" % (nsub, nchan, int(meta.get("nbin", 0))),
             "# template: %s" % str(meta.get("template", "cleaner")).replace("\n", " "),
             "# masked: %d" % int(masked.sum()),
             "# columns: %s" % COLUMNS]
    for s in range(nsub):
        for c in range(nchan):
            lines.append("%d %d %s %s %s %s" % (s, c, _g(amp[s, c]), _g(err[s, c]), _g(freq[s, c]), _g(tmin[s])))
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def load(path):
    """Read a file save() wrote: dict(amp, err, freq_MHz (nsub, nchan), time_min
    (nsub,), and the header's archive, nbin, template, masked).  Finite numbers
    come back bit for bit; a NaN comes back as a NaN."""
    head = {}
    rows = []
    with open(path) as fh:
        first = fh.readline().rstrip("\n")
        if first != MAGIC:
            raise ValueError("%s: not a dynamic-spectrum file (first line %r)" % (path, first))
        for line in fh:
            line = line.rstrip("\n")
            if line.startswith("#"):
                key, _, val = line[1:].partition(":")
                head[key.strip()] = val.strip()
            elif line.strip():
                rows.append(line.split())
    try:
        nsub, nchan, nbin = (int(v) for v in head["shape"].split())
    except (KeyError, ValueError):
        raise ValueError("%s: no shape line in the header" % path) from None
    if len(rows) != nsub * nchan:
        raise ValueError("%s: %d profile lines for a shape of %d x %d" % (path, len(rows), nsub, nchan))
    amp = np.zeros((nsub, nchan), np.float64)
    err = np.zeros((nsub, nchan), np.float64)
    freq = np.full((nsub, nchan), np.nan)
    tmin = np.full(nsub, np.nan)
    for f in rows:
        if len(f) != 6:
            raise ValueError("%s: expected 6 columns (%s), got %r" % (path, COLUMNS, " ".join(f)))
        s, c = int(f[0]), int(f[1])
        amp[s, c], err[s, c], freq[s, c], tmin[s] = float(f[2]), float(f[3]), float(f[4]), float(f[5])
    return dict(amp=amp, err=err, freq_MHz=freq, time_min=tmin, archive=head.get("archive", ""), nbin=nbin,
                template=head.get("template", ""), masked=int(head.get("masked", 0)))
