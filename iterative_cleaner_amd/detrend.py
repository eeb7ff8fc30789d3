"""Detrended scaling: the written definition (numpy), opt-in.

Before a diagnostic (std, mean, ptp, fftmax) is scaled by the median and MAD of
its channel (a line over the subints) or of its subint (a line over the
channels), a low-order polynomial trend of that line can be removed, so that
a bandpass slope or a gain drift does not inflate the line's MAD.  The
reference cleaner has no such step (its README: "The detrending algorithm was
removed"); the surgical cleaner it descends from, coast_guard, has one
(``iterative_detrend``).  coast_guard is not available here: this module is
MODELLED ON its iterative_detrend, NOT PINNED to it, and parity with it is
UNPINNED.  This statement is the pin: the HIP kernels (k_linetrend,
k_combine_dt in csrc/ic_linestats.hip) follow it operation by operation, and
the GPU tests compare bit for bit.

Parameters: chan_order, subint_order in 0..3 (0: that direction is not
detrended; both 0: off), rounds in 1..8 (default 4), clip a finite f64 > 0
(default 5.0).

One line: d[0..n) in the diagnostic's dtype (f64; f32 for ptp of f32 data), a
membership mask valid (w0 != 0 for std / mean / ptp, everything for fftmax),
an order k.

1. The trend is ZERO (four coefficients +0.0) when k == 0, when no entry is
   valid, or when any valid value is NaN or +-Inf.
2. x_j = f64(2 j - (n - 1)) / f64(n - 1)  (n == 1: x_0 = 0);  y_j = f64(d_j).
3. use = valid.  For r = 1 .. rounds:
     |use| <= k: the trend is zero, stop.
     S_p = sum_{j in use} x_j^p, p = 0..2k;  B_p = sum_{j in use} x_j^p * y_j,
     p = 0..k.  x^0 = 1.0, x^p = x^(p-1) * x; the term of B_p is the one
     product (x^p) * y.  Every sum runs as 64 chains: chain l adds the terms of
     the j in use with j = l (mod 64), in ascending j, starting from +0.0; the
     chains are combined by the halving tree t[l] = t[l] + t[l + h], l < h,
     for h = 32, 16, 8, 4, 2, 1; the sum is t[0].  (A term left out and a term
     +0.0 give the same bits: a chain that starts at +0.0 is never -0.0.)
     Solve G a = B, G_pq = S_{p+q}, by elimination without pivoting:
         for i = 0..k:   piv = G[i][i]; unless piv > 0 and finite: zero trend, stop
             for r' = i+1..k:  f = G[r'][i] / piv
                 for c = i+1..k:  G[r'][c] = G[r'][c] - f * G[i][c]
                 B[r'] = B[r'] - f * B[i]
         for i = k..0:   s = B[i];  for c = i+1..k: s = s - G[i][c] * a[c]
             a[i] = s / G[i][i]
     every product, difference and quotient its own IEEE f64 operation.
     a (a_{k+1..3} = +0.0) is now the line's trend.  r == rounds: stop.
     e_j = y_j - p(x_j), p by Horner from a_k: t = a_k; t = t * x + a_i for
     i = k-1..0, every * and + rounded separately.
     Any e_j, j in use, not finite: stop (the trend stays a).
     med = median of e over use, mad = median of |e - med| over use, in f64 with
     the scalers' median arithmetic (odd count: 0 + mid; even: ((0 + lo) + hi) / 2).
     mad == 0: stop.
     new_use = valid and |e_j - med| <= clip * mad (e_j evaluated for every
     valid j).  new_use == use: stop; else use = new_use.
4. d'_j = dtype(f64(d_j) - p(x_j)) for valid j, d'_j = d_j for invalid j.
   (A zero trend gives p = +0.0 and d' = d, bit for bit.)

The scaler then runs on d' exactly as it runs on d without detrending: the
median, the MAD, the quotient, the MAD == 0 rule and the masked |d| rule.  A
channel's scaled value uses the channel direction's d' (chan_order), a
subint's the subint direction's d' (subint_order).

No sum above depends on a schedule option: the GPU forms the chains in a wave's
64 lanes whatever the number of waves per line.

Piecewise detrending (opt-in on top of the above; k_linetrend_pw, k_combine_pw)
----------------------------------------------------------------------------
coast_guard's detrend also takes breakpoints (``bp``) and ``numpieces`` and fits
every piece of a line on its own; its surgical cleaner exposes both per direction
(chan_breakpoints, chan_numpieces, subint_breakpoints, subint_numpieces).  That
is stated from memory: this part too is MODELLED ON it and UNPINNED.  It is what
a band made of polyphase-filtered subbands needs (the filter's bandpass shape
repeats once per subband along a subint's line), and bands with gaps, and a
gain step in time.

A direction's pieces are a strictly ascending list of starts b_0 = 0 < b_1 < ..
< b_{m-1} < n, 1 <= m <= 512; piece q is [b_q, b_{q+1}), the last one ends at
n.  All lines and diagnostics of a direction share them.  The piecewise rule is
the rule above except where stated here:

1'. (unchanged, whole line) every piece's trend is zero when k == 0, when no
    entry of the line is valid, or when any valid value of the line is NaN or
    +-Inf.
2'. Each piece has its own abscissa: for entry j of piece q of length L,
    i = j - b_q and x = f64(2 i - (L - 1)) / f64(L - 1)  (L == 1: x = 0).
3'. use = valid (per line).  For r = 1 .. rounds:
      every piece that is not retired is fitted on its own: S_p, B_p over the
      piece's members of use, as 64 chains by i mod 64 in ascending i from
      +0.0, then the halving tree; the elimination above.  A piece with
      <= k members, or that meets a refused pivot, is RETIRED: its
      coefficients are +0.0 in this round and in every later one.  Retiring a
      piece does not stop the line.
      r == rounds, or use is empty: stop.
      e_j = y_j - p_q(x) by Horner at the direction's order k with the
      coefficients of j's piece (a retired piece: p = +0.0, e = y).
      The stop rules are the line's, as above: stop if an e in use is not
      finite; med and mad of e over ALL of use; stop if mad == 0; new_use =
      valid and |e - med| <= clip * mad; stop if it is unchanged.  Membership
      is per line (as in coast_guard's iterative_detrend); only the fit is per
      piece.
4'. d'_j = dtype(f64(d_j) - p_q(x)) for valid j with its own piece's
    coefficients, d'_j = d_j otherwise.

One piece ([0]): every coefficient, median, MAD and d' equals the whole-line
statement's bit for bit.  The two differ in one place that reaches no output:
where the whole-line rule says "zero trend, stop" (|use| <= k, a refused pivot)
the piecewise rule retires the piece and goes on clipping, so the final
membership may differ, and with it nothing else: the coefficients stay +0.0.

A consequence: the entries of a retired piece meet the scaler undetrended,
beside neighbours that lost their level, so a subband with <= k live channels
is likely to be zapped.  No lower order is tried for such a piece.

The switch IC_DETREND_PIECES="<chan>;<subint>": each side empty (one piece),
"N" (N pieces, starts (q n) // N), "wN" (a piece every N entries) or a comma
list of starts beginning with 0.  As everywhere here "chan" means the channel
lines (over the subints, n = nsub) and "subint" the subint lines (over the
channels, n = nchan).  Pieces of a direction without a detrend order are
ignored.
"""
from __future__ import annotations

import math
import os

import numpy as np

__all__ = ["DEFAULT_ROUNDS", "DEFAULT_CLIP", "check_params", "parse_detrend", "env_detrend", "abscissa",
           "chain_sum", "line_trend", "line_fit", "normalise", "poly_eval", "detrended", "detrend_cube",
           "MAX_PIECES", "check_pieces", "pieces_from_count", "pieces_every", "piece_spec", "resolve_pieces",
           "parse_pieces", "env_pieces", "normalise_pieces", "piece_abscissa", "line_fit_pieces", "line_trend_pieces",
           "detrended_pieces", "detrend_cube_pieces"]

DEFAULT_ROUNDS = 4
DEFAULT_CLIP = 5.0
MAX_ORDER = 3
MAX_ROUNDS = 8
MAX_PIECES = 512


def check_params(chan_order, subint_order, rounds=DEFAULT_ROUNDS, clip=DEFAULT_CLIP):
    """(chan_order, subint_order, rounds, clip) validated, or ValueError."""
    for name, v in (("chan_order", chan_order), ("subint_order", subint_order), ("rounds", rounds)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError("detrend: %s=%r is not an integer" % (name, v))
    co, so, rd = int(chan_order), int(subint_order), int(rounds)
    for name, v in (("chan_order", co), ("subint_order", so)):
        if v < 0 or v > MAX_ORDER:
            raise ValueError("detrend: %s=%d outside 0..%d" % (name, v, MAX_ORDER))
    if rd < 1 or rd > MAX_ROUNDS:
        raise ValueError("detrend: rounds=%d outside 1..%d" % (rd, MAX_ROUNDS))
    cl = float(clip)
    if not (math.isfinite(cl) and cl > 0.0):
        raise ValueError("detrend: clip=%r must be finite and > 0" % (clip,))
    return co, so, rd, cl


def parse_detrend(text):
    """"chan,subint[,rounds,clip]" -> (chan, subint, rounds, clip), or None when
    the text is empty or "0", or when both orders are 0 (off)."""
    text = (text or "").strip()
    if text in ("", "0"):
        return None
    parts = [t.strip() for t in text.split(",")]
    if len(parts) < 2 or len(parts) > 4:
        raise ValueError("IC_DETREND=%r: expected chan,subint[,rounds,clip]" % text)
    try:
        vals = [int(parts[0]), int(parts[1])]
        vals.append(int(parts[2]) if len(parts) > 2 else DEFAULT_ROUNDS)
        vals.append(float(parts[3]) if len(parts) > 3 else DEFAULT_CLIP)
    except ValueError:
        raise ValueError("IC_DETREND=%r: expected chan,subint[,rounds,clip]" % text) from None
    out = check_params(*vals)
    return None if out[0] == 0 and out[1] == 0 else out


def env_detrend():
    """The IC_DETREND switch: None (unset, empty, "0", orders 0,0) or the
    validated (chan_order, subint_order, rounds, clip)."""
    return parse_detrend(os.environ.get("IC_DETREND", ""))


def shards_enabled() -> bool:
    """The opt-in switch of detrending under channel sharding: the environment
    variable IC_DETREND_SHARDS (unset, empty or ``0`` = off), read at every call.
    torchrun hands the environment to every rank, which is how the ranks of a
    group agree (ic_shard_enable_detrend must be called on all of them)."""
    return os.environ.get("IC_DETREND_SHARDS", "") not in ("", "0")


def normalise(detrend):
    """A detrend argument (None = the IC_DETREND switch; a tuple (chan, subint[,
    rounds, clip])) -> None (off) or the validated four."""
    if detrend is None:
        return env_detrend()
    t = tuple(detrend)
    if len(t) < 2 or len(t) > 4:
        raise ValueError("detrend=%r: expected (chan, subint[, rounds, clip])" % (detrend,))
    out = check_params(*t)
    return None if out[0] == 0 and out[1] == 0 else out


def abscissa(n: int) -> np.ndarray:
    if n == 1:
        return np.zeros(1, np.float64)
    j = np.arange(n, dtype=np.int64)
    return (2 * j - (n - 1)).astype(np.float64) / np.float64(n - 1)


def chain_sum(terms: np.ndarray) -> np.ndarray:
    """The statement's sum over the last axis of terms (..., n) f64 (left-out
    terms given as +0.0): 64 chains in ascending j, then the halving tree."""
    n = terms.shape[-1]
    rows = (n + 63) // 64
    pad = np.zeros(terms.shape[:-1] + (rows * 64,), np.float64)
    pad[..., :n] = terms
    pad = pad.reshape(terms.shape[:-1] + (rows, 64))
    t = np.zeros(terms.shape[:-1] + (64,), np.float64)
    for q in range(rows):
        t = t + pad[..., q, :]
    h = 32
    while h >= 1:
        t = t[..., :h] + t[..., h:2 * h]
        h //= 2
    return t[..., 0]


def _solve(S, B, k):
    """The statement's elimination; S, B Python floats.  None: zero trend."""
    G = [[S[p + q] for q in range(k + 1)] for p in range(k + 1)]
    B = list(B)
    for i in range(k + 1):
        piv = G[i][i]
        if not (piv > 0.0 and math.isfinite(piv)):
            return None
        for r in range(i + 1, k + 1):
            f = G[r][i] / piv
            for c in range(i + 1, k + 1):
                G[r][c] = G[r][c] - f * G[i][c]
            B[r] = B[r] - f * B[i]
    a = [0.0] * (k + 1)
    for i in range(k, -1, -1):
        s = B[i]
        for c in range(i + 1, k + 1):
            s = s - G[i][c] * a[c]
        a[i] = s / G[i][i]
    return a


def poly_eval(x: np.ndarray, coef, order: int) -> np.ndarray:
    """p(x) by Horner from coef[order]."""
    with np.errstate(all="ignore"):
        t = np.full(x.shape, np.float64(coef[order]), np.float64)
        for i in range(order - 1, -1, -1):
            t = t * x + np.float64(coef[i])
    return t


def _median64(v: np.ndarray) -> np.float64:
    s = np.sort(v)
    idx, odd = divmod(s.shape[0], 2)
    if odd:
        return np.float64(0.0) + s[idx]
    return ((np.float64(0.0) + s[idx - 1]) + s[idx]) / np.float64(2.0)


def line_trend(d, valid, order, rounds=DEFAULT_ROUNDS, clip=DEFAULT_CLIP):
    """(coef f64[4], rounds_used) of one line; rounds_used counts the fits made
    (0 for a trend that is zero by rule 1)."""
    coef, used, _ = line_fit(d, valid, order, rounds, clip)
    return coef, used


def line_fit(d, valid, order, rounds=DEFAULT_ROUNDS, clip=DEFAULT_CLIP):
    """line_trend plus the final membership: (coef, rounds_used, use)."""
    d = np.asarray(d)
    valid = np.asarray(valid, dtype=bool)
    n = d.shape[0]
    k = int(order)
    zero = np.zeros(4, np.float64)
    if k == 0 or not valid.any():
        return zero, 0, valid.copy()
    y = d.astype(np.float64)
    if not np.isfinite(y[valid]).all():
        return zero, 0, valid.copy()
    x = abscissa(n)
    xp = [np.ones(n, np.float64)]
    for _ in range(2 * k):
        xp.append(xp[-1] * x)
    clip = np.float64(clip)
    use = valid.copy()
    coef = zero
    used = 0
    ysafe = np.where(valid, y, 0.0)
    with np.errstate(all="ignore"):
        for r in range(1, int(rounds) + 1):
            if int(use.sum()) <= k:
                return zero, used, use
            terms = [np.where(use, xp[p], 0.0) for p in range(2 * k + 1)]
            terms += [np.where(use, xp[p] * ysafe, 0.0) for p in range(k + 1)]
            sums = chain_sum(np.stack(terms))
            a = _solve([float(v) for v in sums[:2 * k + 1]], [float(v) for v in sums[2 * k + 1:]], k)
            used = r
            if a is None:
                return zero, used, use
            coef = np.zeros(4, np.float64)
            coef[:k + 1] = a
            if r == int(rounds):
                break
            e = ysafe - poly_eval(x, coef, k)
            if not np.isfinite(e[use]).all():
                break
            med = _median64(e[use])
            dev = np.abs(e - med)
            mad = _median64(dev[use])
            if mad == 0.0:
                break
            new_use = valid & (dev <= clip * mad)
            if np.array_equal(new_use, use):
                break
            use = new_use
    return coef, used, use


def detrended(d, valid, coef, order=None):
    """d' of the statement (step 4) in d's dtype.  order: the line's order
    (None: the highest non-zero coefficient's; a zero trend then returns d)."""
    d = np.asarray(d)
    valid = np.asarray(valid, dtype=bool)
    coef = np.asarray(coef, np.float64)
    if order is None:
        nz = np.nonzero(coef)[0]
        if nz.size == 0:
            return d
        order = int(nz[-1])
    if order == 0 and coef[0] == 0.0 and not np.signbit(coef[0]):
        return d
    with np.errstate(all="ignore"):
        p = poly_eval(abscissa(d.shape[0]), coef, int(order))
        out = d.copy()
        out[valid] = (d.astype(np.float64) - p).astype(d.dtype)[valid]
    return out


def detrend_cube(D, valid, chan_order, subint_order, rounds=DEFAULT_ROUNDS, clip=DEFAULT_CLIP):
    """Both directions of one diagnostic D (nsub, nchan): (Dc, Ds, chan_coef
    (nchan, 4), subint_coef (nsub, 4), rounds_used list) - Dc[:, c] is channel
    c's d', Ds[s, :] subint s's."""
    D = np.asarray(D)
    nsub, nchan = D.shape
    Dc, Ds = D.copy(), D.copy()
    cc = np.zeros((nchan, 4), np.float64)
    sc = np.zeros((nsub, 4), np.float64)
    used = []
    for c in range(nchan):
        cc[c], u = line_trend(D[:, c], valid[:, c], chan_order, rounds, clip)
        used.append(u)
        if chan_order:
            Dc[:, c] = detrended(D[:, c], valid[:, c], cc[c], chan_order)
    for s in range(nsub):
        sc[s], u = line_trend(D[s, :], valid[s, :], subint_order, rounds, clip)
        used.append(u)
        if subint_order:
            Ds[s, :] = detrended(D[s, :], valid[s, :], sc[s], subint_order)
    return Dc, Ds, cc, sc, used


# ---------------------------------------------------------------- pieces


def check_pieces(starts, n):
    """The validated starts of a line of n entries as a list of ints, or
    ValueError: first 0, strictly ascending, all < n, at most MAX_PIECES."""
    try:
        b = [int(v) for v in starts]
        if any(isinstance(v, bool) or int(v) != v for v in starts):
            raise TypeError
    except (TypeError, ValueError):
        raise ValueError("detrend pieces: starts %r are not integers" % (starts,)) from None
    if len(b) < 1 or len(b) > MAX_PIECES:
        raise ValueError("detrend pieces: %d pieces outside 1..%d" % (len(b), MAX_PIECES))
    if b[0] != 0:
        raise ValueError("detrend pieces: the first start is %d, not 0" % b[0])
    if any(v <= u for u, v in zip(b, b[1:])):
        raise ValueError("detrend pieces: starts are not strictly ascending")
    if b[-1] >= int(n):
        raise ValueError("detrend pieces: start %d at or past the line's %d entries" % (b[-1], int(n)))
    return b


def pieces_from_count(n, m):
    """m pieces of a line of n entries: starts (q n) // m; ValueError when two
    coincide (m > n) or m is outside 1..MAX_PIECES."""
    n, m = int(n), int(m)
    if m < 1 or m > MAX_PIECES:
        raise ValueError("detrend pieces: %d pieces outside 1..%d" % (m, MAX_PIECES))
    b = [(q * n) // m for q in range(m)]
    if any(v == u for u, v in zip(b, b[1:])):
        raise ValueError("detrend pieces: %d pieces of %d entries: starts coincide" % (m, n))
    return check_pieces(b, n)


def pieces_every(n, width):
    """A piece every `width` entries (the last one may be shorter)."""
    n, width = int(n), int(width)
    if width < 1:
        raise ValueError("detrend pieces: width %d < 1" % width)
    return check_pieces(list(range(0, n, width)), n)


def piece_spec(v, what):
    """One direction's pieces before the shape is known: None (one piece), an
    int count, "wN", or a tuple of starts."""
    if v is None:
        return None
    if isinstance(v, str):
        t = v.strip()
        if t == "":
            return None
        try:
            if t[0] in "wW":
                w = int(t[1:])
                if w < 1:
                    raise ValueError
                return "w%d" % w
            if "," in t:
                return tuple(int(p) for p in t.split(","))
            return int(t)
        except ValueError:
            raise ValueError("%s: %r is not empty, N, wN or a list of starts" % (what, v)) from None
    if isinstance(v, bool):
        raise ValueError("%s: %r is not a piece count or a list of starts" % (what, v))
    if isinstance(v, (int, np.integer)):
        return int(v)
    return tuple(v)


def resolve_pieces(spec, n):
    """A direction's spec (see piece_spec) on lines of n entries -> the validated
    starts, or None for one piece."""
    spec = piece_spec(spec, "detrend pieces")
    if spec is None:
        return None
    if isinstance(spec, str):
        return pieces_every(n, int(spec[1:]))
    if isinstance(spec, int):
        return pieces_from_count(n, spec)
    return check_pieces(spec, n)


def parse_pieces(text):
    """"<chan>;<subint>" -> (chan spec, subint spec), or None when the text is
    empty or both sides are.  The specs are resolved with a shape by
    normalise_pieces; the forms are checked here."""
    text = (text or "").strip()
    if text == "":
        return None
    parts = text.split(";")
    if len(parts) != 2:
        raise ValueError("IC_DETREND_PIECES=%r: expected <chan>;<subint>" % text)
    out = tuple(piece_spec(p, "IC_DETREND_PIECES=%r" % text) for p in parts)
    for sp in out:
        if isinstance(sp, int) and (sp < 1 or sp > MAX_PIECES):
            raise ValueError("IC_DETREND_PIECES=%r: %d pieces outside 1..%d" % (text, sp, MAX_PIECES))
        if isinstance(sp, tuple):
            check_pieces(sp, sp[-1] + 1 if sp else 1)
    return None if out == (None, None) else out


def env_pieces():
    """The IC_DETREND_PIECES switch: None or (chan spec, subint spec)."""
    return parse_pieces(os.environ.get("IC_DETREND_PIECES", ""))


def normalise_pieces(pieces, nsub, nchan, detrend=False):
    """A detrend_pieces argument (None = the IC_DETREND_PIECES switch; a pair
    (chan, subint), each None, a count, "wN" or a sequence of starts) on a
    (nsub, nchan) archive -> None (no pieces) or (chan starts or None, subint
    starts or None).  detrend: the validated detrend four, or None for "off"
    (then no pieces); given, the pieces of a direction whose order is 0 are
    ignored.  The default (False) keeps both directions."""
    if pieces is None:
        pieces = env_pieces()
        if pieces is None:
            return None
    t = tuple(pieces)
    if len(t) != 2:
        raise ValueError("detrend_pieces=%r: expected (chan, subint)" % (pieces,))
    if detrend is None:
        return None
    orders = (1, 1) if detrend is False else detrend[:2]
    out = tuple(resolve_pieces(sp, n) if k else None for sp, n, k in zip(t, (nsub, nchan), orders))
    return None if out == (None, None) else out


def piece_abscissa(starts, n) -> np.ndarray:
    """x of every entry of a line of n entries on its piece's own abscissa."""
    ends = list(starts[1:]) + [n]
    return np.concatenate([abscissa(e - b) for b, e in zip(starts, ends)])


def _poly_pieces(x, coef, order, starts, n):
    """p_q(x_j) for every entry j of the line."""
    ends = list(starts[1:]) + [n]
    p = np.empty(n, np.float64)
    for q, (b, e) in enumerate(zip(starts, ends)):
        p[b:e] = poly_eval(x[b:e], coef[q], order)
    return p


def line_fit_pieces(d, valid, order, starts, rounds=DEFAULT_ROUNDS, clip=DEFAULT_CLIP):
    """The piecewise line_fit: (coef f64 (npieces, 4), rounds entered, use)."""
    d = np.asarray(d)
    valid = np.asarray(valid, dtype=bool)
    n = d.shape[0]
    k = int(order)
    b = check_pieces(starts, n)
    ends = b[1:] + [n]
    m = len(b)
    coef = np.zeros((m, 4), np.float64)
    if k == 0 or not valid.any():
        return coef, 0, valid.copy()
    y = d.astype(np.float64)
    if not np.isfinite(y[valid]).all():
        return coef, 0, valid.copy()
    x = piece_abscissa(b, n)
    xp = [np.ones(n, np.float64)]
    for _ in range(2 * k):
        xp.append(xp[-1] * x)
    clip = np.float64(clip)
    use = valid.copy()
    used = 0
    retired = [False] * m
    ysafe = np.where(valid, y, 0.0)
    with np.errstate(all="ignore"):
        for r in range(1, int(rounds) + 1):
            coef = np.zeros((m, 4), np.float64)
            for q in range(m):
                if retired[q]:
                    continue
                sl = slice(b[q], ends[q])
                u = use[sl]
                a = None
                if int(u.sum()) > k:
                    terms = [np.where(u, xp[p][sl], 0.0) for p in range(2 * k + 1)]
                    terms += [np.where(u, xp[p][sl] * ysafe[sl], 0.0) for p in range(k + 1)]
                    sums = chain_sum(np.stack(terms))
                    a = _solve([float(v) for v in sums[:2 * k + 1]], [float(v) for v in sums[2 * k + 1:]], k)
                if a is None:
                    retired[q] = True
                else:
                    coef[q, :k + 1] = a
            used = r
            if r == int(rounds) or not use.any():
                break
            e = ysafe - _poly_pieces(x, coef, k, b, n)
            if not np.isfinite(e[use]).all():
                break
            med = _median64(e[use])
            dev = np.abs(e - med)
            mad = _median64(dev[use])
            if mad == 0.0:
                break
            new_use = valid & (dev <= clip * mad)
            if np.array_equal(new_use, use):
                break
            use = new_use
    return coef, used, use


def line_trend_pieces(d, valid, order, starts, rounds=DEFAULT_ROUNDS, clip=DEFAULT_CLIP):
    """(coef f64 (npieces, 4), rounds entered) of one line in pieces."""
    coef, used, _ = line_fit_pieces(d, valid, order, starts, rounds, clip)
    return coef, used


def detrended_pieces(d, valid, coef, order, starts):
    """d' of the piecewise statement (step 4') in d's dtype; coef (npieces, 4),
    order the direction's (0: d itself)."""
    d = np.asarray(d)
    valid = np.asarray(valid, dtype=bool)
    coef = np.asarray(coef, np.float64)
    if int(order) == 0:
        return d
    n = d.shape[0]
    b = check_pieces(starts, n)
    with np.errstate(all="ignore"):
        p = _poly_pieces(piece_abscissa(b, n), coef, int(order), b, n)
        out = d.copy()
        out[valid] = (d.astype(np.float64) - p).astype(d.dtype)[valid]
    return out


def detrend_cube_pieces(D, valid, chan_order, subint_order, chan_starts=None, subint_starts=None,
                        rounds=DEFAULT_ROUNDS, clip=DEFAULT_CLIP):
    """detrend_cube in pieces (None: one piece): (Dc, Ds, chan_coef (nchan, mc,
    4), subint_coef (nsub, ms, 4), rounds list)."""
    D = np.asarray(D)
    nsub, nchan = D.shape
    cb = [0] if chan_starts is None else check_pieces(chan_starts, nsub)
    sb = [0] if subint_starts is None else check_pieces(subint_starts, nchan)
    Dc, Ds = D.copy(), D.copy()
    cc = np.zeros((nchan, len(cb), 4), np.float64)
    sc = np.zeros((nsub, len(sb), 4), np.float64)
    used = []
    for c in range(nchan):
        cc[c], u = line_trend_pieces(D[:, c], valid[:, c], chan_order, cb, rounds, clip)
        used.append(u)
        if chan_order:
            Dc[:, c] = detrended_pieces(D[:, c], valid[:, c], cc[c], chan_order, cb)
    for s in range(nsub):
        sc[s], u = line_trend_pieces(D[s, :], valid[s, :], subint_order, sb, rounds, clip)
        used.append(u)
        if subint_order:
            Ds[s, :] = detrended_pieces(D[s, :], valid[s, :], sc[s], subint_order, sb)
    return Dc, Ds, cc, sc, used
