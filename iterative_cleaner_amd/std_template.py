"""Cleaning against a supplied standard profile (opt-in): the written
definition that the GPU kernels k_std_ccf, k_std_peak and k_std_install
(csrc/ic_stdtemplate.hip) follow bit for bit.

The reference builds its template from the archive itself, once per iteration
(iterative_cleaner.py:88-94).  Its ancestor, coast_guard's surgical cleaner,
can instead be handed a standard profile of the pulsar; this module states
what this build does with one.  Parity with psrchive / coast_guard is
unpinned, as elsewhere: the rules below are this project's.

Inputs: ``S``, the standard (f32, nbin long), and ``A``, the archive's own
first template (f32, nbin long: what iteration 1's template stage leaves).

Cross-correlation, all in f64::

    a = f64(A)
    s = f64(S) - m,   m = (sequential ascending-index sum of f64(S)) / nbin
    c[k] = sum_i a[i] * s[(i - k) mod nbin],   k = 0 .. nbin-1

every product rounded on its own and added in ascending i (no FMA).

Lag: ``k*`` is the smallest k at which c is largest.  If any c[k] is not
finite, or c[k*] <= 0, or -min_k c[k] > c[k*], the alignment FAILS: lag = 0,
shift = 0.0, the standard is used as given and aligned = 0 is reported.  That
is not an error of the run (an archive with a NaN sample has a NaN A; the
default loop runs on too).  The third condition is what catches a standard
that anti-correlates with the archive (A = -S): s has zero mean, so sum_k c[k]
= (sum a)(sum s) is zero up to rounding and the largest c[k] of ANY non-trivial
pair is positive; c[k*] <= 0 alone only catches a zero A.  A standard that
matches has c[k*] = sum s^2 at the peak against side lobes of the order of
m sum a.

Sub-bin part (the parabola through the peak's neighbours, the rule of
psrchive's ParIntShiftFit)::

    cm = c[(k*-1) mod nbin], c0 = c[k*], cp = c[(k*+1) mod nbin]
    den = (cm - c0) + (cp - c0)
    delta = 0.5 * (cm - cp) / den  if den < 0  else 0
    shift = k* + delta

Aligned template, by mode:

``none``  S as given.  No cross-correlation is made: aligned = 0, lag = 0,
          shift = 0.0 are reported.
``int``   out[i] = S[(i - k*) mod nbin]: the original f32 samples, exact.
``frac``  phase_rotation.rotate(S[None, :], phase_rotation.phasors(nbin,
          [shift]), -1)[0]: the written f32 rotation k_rotate / k_rotate_mr
          follow, so only where dedispersion.fft_supported(nbin) holds.
``auto``  ``frac`` where it is available, else ``int``.

The standard is used as given, in f32: no x10000 and no normalisation, the
fit's amplitude absorbs the scale.  With a fixed template nothing in an
iteration depends on the previous mask, so the loop is one pass (DESIGN.md,
"Standard template").

The switch is ``IC_STD_TEMPLATE="<path>[,<align>]"`` (read by the Python
layer, never by the library).
"""
from __future__ import annotations

import os
import sys

import numpy as np

from . import phase_rotation
from .dedispersion import fft_supported

__all__ = ["ALIGN_NONE", "ALIGN_INT", "ALIGN_FRAC", "ALIGN_NAMES", "ENV", "check", "resolve_align", "ccf", "peak",
           "align", "parse", "env_std_template", "load", "normalise", "warn_failed"]

ALIGN_NONE, ALIGN_INT, ALIGN_FRAC = 0, 1, 2    # IC_ALIGN_* (include/iterative_cleaner.h)
ALIGN_NAMES = {"none": ALIGN_NONE, "int": ALIGN_INT, "frac": ALIGN_FRAC}
ENV = "IC_STD_TEMPLATE"
MIN_NBIN = 4


def check(S, nbin: int) -> np.ndarray:
    """The standard as the loop takes it: 1-D, nbin long (no rebinning), every
    value finite, not constant, nbin >= 4; returned as a C-contiguous f32 array.
    Anything else is a ValueError."""
    nbin = int(nbin)
    if nbin < MIN_NBIN:
        raise ValueError("std_template: nbin=%d < %d" % (nbin, MIN_NBIN))
    S = np.asarray(S)
    if S.ndim != 1:
        raise ValueError("std_template: the standard must be 1-D, got shape %s" % (S.shape,))
    if S.shape[0] != nbin:
        raise ValueError("std_template: the standard has %d bins, the archive %d (a standard of another length "
                         "is not rebinned)" % (S.shape[0], nbin))
    if S.dtype.kind not in "fiu":
        raise ValueError("std_template: the standard must be real numbers, got dtype %s" % S.dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        S = np.ascontiguousarray(S, dtype=np.float32)
    if not np.all(np.isfinite(S)):
        raise ValueError("std_template: the standard holds a non-finite value")
    if np.all(S == S[0]):
        raise ValueError("std_template: the standard is constant")
    return S


def resolve_align(align, nbin: int) -> int:
    """An alignment mode ("auto", "none", "int", "frac" or an IC_ALIGN_* value)
    -> IC_ALIGN_*.  ``frac`` at a length the rotation does not serve is
    refused; ``auto`` there is ``int``."""
    if align is None:
        align = "auto"
    if isinstance(align, str):
        name = align.strip().lower()
        if name == "auto":
            return ALIGN_FRAC if fft_supported(int(nbin)) else ALIGN_INT
        if name not in ALIGN_NAMES:
            raise ValueError("std_template: align=%r (one of auto, none, int, frac)" % (align,))
        mode = ALIGN_NAMES[name]
    else:
        mode = int(align)
        if mode not in (ALIGN_NONE, ALIGN_INT, ALIGN_FRAC):
            raise ValueError("std_template: align=%r (one of auto, none, int, frac)" % (align,))
    if mode == ALIGN_FRAC and not fft_supported(int(nbin)):
        raise ValueError("std_template: align 'frac' %s (nbin=%d); use 'int'"
                         % (phase_rotation.UNSUPPORTED, int(nbin)))
    return mode


def ccf(S, A) -> np.ndarray:
    """c[k] of the module docstring, f64 (nbin,)."""
    S = np.asarray(S, dtype=np.float32)
    A = np.asarray(A, dtype=np.float32)
    n = S.shape[0]
    a = A.astype(np.float64)
    s64 = S.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.cumsum(s64)[-1] / np.float64(n)    # cumsum adds in ascending index
        s = s64 - m
        # s2[n - k + i] = s[(i - k) mod n] for 0 <= i, k < n (k = 0: s2[n + i])
        s2 = np.concatenate([s, s, s[:1]])
        k = np.arange(n)
        c = np.zeros(n, np.float64)
        for i in range(n):
            c = c + a[i] * s2[n - k + i]
    return c


def peak(c):
    """(aligned, lag, shift) from the cross-correlation (module docstring)."""
    c = np.asarray(c, dtype=np.float64)
    n = c.shape[0]
    if not np.all(np.isfinite(c)):
        return 0, 0, 0.0
    ks = int(np.argmax(c))     # the first of equal maxima
    c0 = c[ks]
    if not c0 > 0.0 or -np.min(c) > c0:
        return 0, 0, 0.0
    cm, cp = c[(ks - 1) % n], c[(ks + 1) % n]
    den = (cm - c0) + (cp - c0)
    delta = np.float64(0.5) * (cm - cp) / den if den < 0.0 else np.float64(0.0)
    return 1, ks, float(np.float64(ks) + delta)


def align(S, A, mode="auto") -> dict:
    """The template the loop installs for the standard S and the archive's
    first template A: dict(aligned, lag, shift, template, mode)."""
    S = check(S, np.shape(S)[0] if np.ndim(S) == 1 else MIN_NBIN)
    n = S.shape[0]
    mode = resolve_align(mode, n)
    if mode == ALIGN_NONE:
        return dict(aligned=0, lag=0, shift=0.0, template=S.copy(), mode=mode)
    A = np.ascontiguousarray(A, dtype=np.float32).reshape(n)
    aligned, lag, shift = peak(ccf(S, A))
    if not aligned:
        T = S.copy()
    elif mode == ALIGN_INT:
        T = S[(np.arange(n) - lag) % n].copy()
    else:
        T = phase_rotation.rotate(S[None, :], phase_rotation.phasors(n, [shift]), -1, any_length=False)[0]
    return dict(aligned=aligned, lag=lag, shift=shift, template=np.ascontiguousarray(T, dtype=np.float32),
                mode=mode)


# ---------------------------------------------------------------- switch, loading

def parse(text):
    """"<path>[,<align>]" -> (path, align name), or None when the text is empty.
    The align name is the text after the LAST comma: one of auto, none, int,
    frac (ValueError otherwise); without a comma it is auto."""
    text = (text or "").strip()
    if text == "":
        return None
    path, alg = text, "auto"
    if "," in text:
        head, tail = text.rsplit(",", 1)
        path, alg = head.strip(), tail.strip().lower()
        if alg not in ("auto",) + tuple(ALIGN_NAMES):
            raise ValueError("%s=%r: align %r (one of auto, none, int, frac)" % (ENV, text, tail.strip()))
    if path == "":
        raise ValueError("%s=%r: no path" % (ENV, text))
    return path, alg


def env_std_template():
    """The IC_STD_TEMPLATE switch: None (unset or empty) or (path, align)."""
    return parse(os.environ.get(ENV, ""))


def load(path, nbin: int, backend=None) -> np.ndarray:
    """The standard of `path`, checked for nbin: a ``.npy`` file holding a 1-D
    array, or an archive (backend = cleaner.archive_backend() when None) brought
    to one profile: pscrunch, remove_baseline, dedisperse, fscrunch, tscrunch,
    then get_Profile(0, 0, 0).get_amps()."""
    path = os.fspath(path)
    if path.lower().endswith(".npy"):
        return check(np.load(path, allow_pickle=False), nbin)
    if backend is None:
        from .cleaner import archive_backend
        backend = archive_backend()
    ar = backend.Archive_load(path)
    ar.pscrunch()
    ar.remove_baseline()
    ar.dedisperse()
    ar.fscrunch()
    ar.tscrunch()
    return check(np.asarray(ar.get_Profile(0, 0, 0).get_amps()), nbin)


def normalise(std_template, nbin: int, backend=None):
    """A std_template argument -> None (off) or (S f32 checked, IC_ALIGN_*).
    None reads the IC_STD_TEMPLATE switch; otherwise an array (align auto), a
    path, or a pair (array or path, align)."""
    alg = "auto"
    if std_template is None:
        sw = env_std_template()
        if sw is None:
            return None
        std_template, alg = sw
    elif isinstance(std_template, (tuple, list)) and len(std_template) == 2 and (
            isinstance(std_template[1], (str, int, np.integer)) and not isinstance(std_template[0], (int, float))):
        std_template, alg = std_template
    if isinstance(std_template, (str, os.PathLike)):
        S = load(std_template, nbin, backend)
    else:
        S = check(std_template, nbin)
    return S, resolve_align(alg, nbin)


def warn_failed(alignment, mode, what="the archive"):
    """One line on stderr when an alignment that was measured (mode not
    ``none``) failed (stdout stays the reference's)."""
    if alignment is not None and mode != ALIGN_NONE and not alignment["aligned"]:
        sys.stderr.write("std_template: the alignment against %s failed (a non-finite correlation, no positive peak, "
                         "or a trough deeper than the peak); the standard is used as given\n" % what)
