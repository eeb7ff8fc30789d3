"""Fractional dedispersion of the archive stand-in: psrchive's FFT phase rotation
with a written, reproducible arithmetic order.

psrchive dedisperses a profile by rotating it in phase through its Fourier
transform (Pulsar::Profile::rotate_phase -> fft::shift: forward real FFT,
multiply harmonic k by exp(i 2 pi k s / nbin), inverse real FFT, 1/nbin).  The
reference calls it through ``dedisperse()`` / ``dededisperse()``
(iterative_cleaner.py:91, :100, :104).  psrchive is absent here, so real-data
parity is unpinned; this module DEFINES the stand-in's rotation so that the
GPU kernel (k_rotate, ic_rotate.hip), the C restatement the tests check
against (orc_rotate in the oracle/ directory) and this numpy version agree bit for
bit.

Definition, for a profile x of N = 2M samples (N a power of two, or a multiple
of 8 whose half M has only the prime factors 2, 3 and 5) and a delay
of s bins (``y[j] = x[j + s]`` for integer s; ``dedisperse`` rotates by +s,
``dededisperse`` by -s).  The arithmetic is IEEE single precision, as psrchive's
(its FTransform runs FFTW's single-precision plans on the f32 amplitudes):

1. x' = f32(x - base) (base 0 when no baseline is subtracted), then
   z[j] = (x'[2j], x'[2j+1]), j < M.
2. Z = FFT_M(z), M = 2^a 3^b 5^c: Stockham autosort, in this stage order
   (:func:`stage_radices`): the a power-of-two levels first, as stages of
   radix R = 8 while three or more of them remain, then one of radix 4 or 2;
   then b stages of radix 3; then c stages of radix 5.  Ns = the product of
   the earlier radices.  Butterfly j < M/R: k = j mod Ns,
   a_q = z[j + q M/R]; from the second stage on (Ns > 1) b_q = a_q * w_q for
   q >= 1 with w_q = tw[q k N/(R Ns)] and the product (a.r w.r - a.i w.i,
   a.r w.i + a.i w.r), else b = a; y = DFT_R(b); out[(j - k) R + k + p Ns] = y_p.
   DFT_2: y0 = b0 + b1, y1 = b0 - b1.  DFT_4: c0 = b0 + b2, c1 = b0 - b2,
   c2 = b1 + b3, c3 = -i (b1 - b3) = (d.i, -d.r); y0 = c0 + c2, y1 = c1 + c3,
   y2 = c0 - c2, y3 = c1 - c3.  DFT_8: c_q = b_q + b_(q+4), c_(q+4) = b_q -
   b_(q+4) (q < 4); c5 = ((c5.r + c5.i) s, (c5.i - c5.r) s), c6 = (c6.i, -c6.r),
   c7 = ((c7.i - c7.r) s, -((c7.r + c7.i) s)) with s = f32(f64(sqrt(2)/2)); the
   even outputs y_(2p) = DFT_4(c0..c3)_p, the odd y_(2p+1) = DFT_4(c4..c7)_p.
   DFT_3: t = b1 + b2, d = b1 - b2, y0 = b0 + t, m = b0 - t h (h = 1/2),
   e = d s3 (both parts by the real s3 = f32(f64(sqrt(3)/2))); y1 = m - i e =
   (m.r + e.i, m.i - e.r), y2 = m + i e = (m.r - e.i, m.i + e.r).
   DFT_5: t1 = b1 + b4, t2 = b2 + b3, d1 = b1 - b4, d2 = b2 - b3;
   y0 = b0 + (t1 + t2); m1 = (b0 + t1 c1) + t2 c2, m2 = (b0 + t1 c2) + t2 c1;
   e1 = d1 s1 + d2 s2, e2 = d1 s2 - d2 s1 (every product a complex by a real:
   both parts); y1 = m1 - i e1, y4 = m1 + i e1, y2 = m2 - i e2, y3 = m2 + i e2
   (-i e and +i e as in DFT_3), with c1 = f32(f64(cos(2 pi/5))), c2 =
   f32(f64(cos(4 pi/5))), s1 = f32(f64(sin(2 pi/5))), s2 = f32(f64(sin(4 pi/5))).
3. For k = 1 .. M/2, q = M - k: the half-length spectrum of the inverse from
   Z_k, Z_q in one linear map (:func:`_pair`: the real spectrum, the phasors
   (P.r, sign * P.i) and the inverse's packing composed), stored conjugated,
   the conjugate's imaginary part as (-a) + (-b) of the two terms' imaginary
   parts (k = M/2 pairs with itself: the k values are stored last).
   DC and Nyquist: X_0 = Z_0.r + Z_0.i, X_M = Z_0.r - Z_0.i (real),
   Y_0 = X_0 P_0.r, Y_M = X_M P_M.r, stored (Y_0 + Y_M)/2, -((Y_0 - Y_M)/2).
4. r = FFT_M(stored) (same stages); out[2j] = r[j].r * (1/M),
   out[2j+1] = (-r[j].i) * (1/M), 1/M the f32 of the f64 quotient (exact for
   a power of two).

Every step is a single IEEE f32 operation in the written order (no fused
multiply-add).  Tables: tw[q] = exp(-2 pi i q / N), evaluated in x87 long
double (cosl/sinl), rounded to f64 (:func:`twiddles`, the table k_diag's FFT
shares) and then to f32; the phasors P[k] = exp(+2 pi i k s / N) of a delay s,
evaluated by the f64 formula of :func:`phasors` (the GPU's ic_phasor,
ic_internal.h) and rounded to f32, so that the library's per-channel table and
its per-profile evaluation (psrchive's per-Integration folding period: one
delay per subint and channel) give the same bits.

History: rounds 2-5 ran radix-2 stages in f64; round 6 redefined the stages
as radix 8 (98 operations per 8 points instead of 120), the pair step as one
linear map, and then the arithmetic as f32, which is psrchive's own
precision and lets k_rotate run every complex operation as packed f32 pairs
(v_pk_add_f32 / v_pk_mul_f32: half the f64 instruction count) with half the
LDS traffic.  The result is within a few f32 ulps of the profile's largest
sample of numpy's f64 ``irfft(rfft(x) * exp(2j pi k s / N))`` (oracle/restated.py
fft_phase_shift, tests/test_phase_rotation.py), as psrchive's FFTW-f32 rotation
is.

Lengths: the definition holds for every N above; the GPU kernels serve the
powers of two 64 .. 8192 (k_rotate<N>) and the mixed-radix set MR of
:func:`mr_supported` (k_rotate_mr): 64 <= N <= 4096, N a multiple of 8 (rows
and half rows stay 16-byte addressable), N/2 = 2^a 3^b 5^c, N not a power of
two.  Measured on random profiles (tests/test_phase_rotation_mr.py) the MR
lengths stay within the same 4 f32 epsilons of the largest sample as the
powers of two.

Any length (opt-in).  Every other n in 16 .. 4096, odd and prime n included,
is served only when the caller opts in (``any_length=True``, or the environment
switch IC_ANY_NBIN read by :func:`any_length_enabled`; the library's
IC_DEDISP_FFT_ANY and ic_rotate_profiles_any, kernel k_rotate_czt); with
nothing switched on such a length is refused as before.  The lengths the
default kernels serve (:func:`kernel_supported`) keep the definition above and
its bits under the opt-in too; the others take this chirp-z (Bluestein)
statement, :func:`rotate_czt`: a DFT of length n as a circular convolution of
length L, the smallest power of two >= 2 n - 1, every step one IEEE f32
operation in the written order, the complex product always (a.r w.r - a.i w.i,
a.r w.i + a.i w.r):

1. x' = f32(x - base); v[j] = (x'[j] w[j].r, x'[j] w[j].i) for j < n, +0 for
   n <= j < L, with the chirp w[j] = exp(-i pi (j^2 mod 2n) / n) =
   tw_2n[j^2 mod 2n] (the reduction in exact integers; tw_2n = twiddles(2n):
   long double, then f64, then f32).
2. V = FFT_L(v): the Stockham stages of step 2 above for a power of two (radix
   8 while three or more levels remain, then 4 or 2), with
   w_q = tw_L[q k L/(R Ns)], tw_L = f32 of twiddles(L).  C = V B (the
   product above, a = V); D = FFT_L(conj(C)) (conj negates the imaginary part).
3. For k < n: X[k] = (conj(D[k]) w[k]) (1/L), both parts by the exact f32 1/L:
   the spectrum DFT_n(x').  Y[k] = X[k] Ph[k], where Ph[k] = (P[k].r,
   sign P[k].i) for k <= n/2 and the conjugate of that at n - k for k > n/2
   (P = f32 of :func:`phasors`, n//2 + 1 entries); for an even n the Nyquist
   harmonic takes P.r only: Y[n/2] = (X.r P.r, X.i P.r).
   v[k] = conj(Y[k]) w[k], +0 for n <= k < L.
4. Step 2 on that v; out[j] = ((conj(D[j]) w[j]).r (1/L)) (1/n), 1/n the f32
   of the f64 quotient.

The filter table B = FFT_L(b), b[j] = b[L - j] = conj(w[j]) for j < n and 0
elsewhere, is built once per length in f64 (:func:`czt_filter`): the f64
chirp, the same Stockham stages with every operation in f64, f64 twiddles(L)
and the f64 sqrt(2)/2, then one rounding to f32 (the library runs the same
stages on the host without contraction and gives the same bits; within 1 f32
ulp of numpy's f64 fft of b).  With B computed by the f32 stages instead the
error below grows by about one epsilon.  Measured against numpy's f64 rotation
on the inputs of tests/test_phase_rotation_mr.py, in f32 epsilons of the
largest |sample| (tests/test_phase_rotation_any.py): 16: 4.08, 17: 2.73,
33: 3.30, 48: 2.92, 100: 3.09, 125: 2.47, 129: 3.25, 448: 3.16, 500: 3.08,
997: 3.54, 2047: 3.23, 2049: 3.05, 2500: 3.78, 4095: 2.93; the asserted bound
is 5.5.  phasors() serves an odd n as it stands (harmonics 0 .. (n - 1)/2,
within 1e-15 of x87 long double).
"""
from __future__ import annotations

import numpy as np

__all__ = ["PI_L", "twiddles", "phasors", "rotate", "is_supported", "mr_supported", "stage_radices",
           "MR_NBIN_MIN", "MR_NBIN_MAX", "UNSUPPORTED", "any_length_enabled", "kernel_supported", "czt_selected",
           "rotate_czt", "czt_length", "czt_chirp", "czt_filter", "CZT_NBIN_MIN", "CZT_NBIN_MAX"]

PI_L = np.longdouble("3.141592653589793238462643383279502884")


MR_NBIN_MIN, MR_NBIN_MAX = 64, 4096    # the library's mr_supported (csrc/ic_internal.h)

# what every refusal says (the checks of archive.py, dedispersion.py and rotate())
UNSUPPORTED = ("needs a power-of-two nbin in 64..8192, or a multiple of 8 in %d..%d whose half has only "
               "the prime factors 2, 3 and 5" % (MR_NBIN_MIN, MR_NBIN_MAX))


def _smooth235(m: int) -> bool:
    for f in (2, 3, 5):
        while m % f == 0:
            m //= f
    return m == 1


def mr_supported(nbin: int) -> bool:
    """The mixed-radix set MR: 64 <= nbin <= 4096, a multiple of 8, nbin/2 =
    2^a 3^b 5^c, not a power of two (those are the templated kernels')."""
    return (MR_NBIN_MIN <= nbin <= MR_NBIN_MAX and nbin % 8 == 0 and (nbin & (nbin - 1)) != 0
            and _smooth235(nbin // 2))


def is_supported(nbin: int) -> bool:
    """The rotation is defined for a power-of-two nbin (the GPU kernels: 64 ..
    8192) and for the mixed-radix lengths of :func:`mr_supported`."""
    return (nbin >= 4 and (nbin & (nbin - 1)) == 0) or mr_supported(nbin)


def stage_radices(m: int) -> list:
    """The Stockham stages of FFT_m, m = 2^a 3^b 5^c, in the definition's order:
    radix 8 while three or more power-of-two levels remain, then 4 or 2, then
    the 3s, then the 5s."""
    a = 0
    while m % 2 == 0:
        m //= 2
        a += 1
    out = [8] * (a // 3) + {0: [], 1: [2], 2: [4]}[a % 3]
    for f in (3, 5):
        while m % f == 0:
            m //= f
            out.append(f)
    if m != 1:
        raise ValueError("FFT length with a prime factor above 5")
    return out


def twiddles(nbin: int) -> np.ndarray:
    """(2, nbin) f64: cos / sin of -2 pi q / nbin (long double, then f64)."""
    q = np.arange(nbin).astype(np.longdouble)
    ang = (np.longdouble(-2.0) * PI_L) * q / np.longdouble(nbin)
    return np.stack([np.cos(ang).astype(np.float64), np.sin(ang).astype(np.float64)])


# Taylor coefficients of sin((pi/2) z) and cos((pi/2) z):
# (-1)^j (pi/2)^(2j+1) / (2j+1)!  and  (-1)^j (pi/2)^(2j) / (2j)!, j = 0 .. 8,
# each the f64 nearest the exact value
_PH_S = tuple(float.fromhex(h) for h in (
    "0x1.921fb54442d18p+0", "-0x1.4abbce625be53p-1", "0x1.466bc6775aae2p-4", "-0x1.32d2cce62bd86p-8",
    "0x1.50783487ee782p-13", "-0x1.e3074fde8871fp-19", "0x1.e8f434d018d63p-25", "-0x1.6fadb9f155744p-31",
    "0x1.aaec32af93359p-38"))
_PH_C = tuple(float.fromhex(h) for h in (
    "0x1.0000000000000p+0", "-0x1.3bd3cc9be45dep+0", "0x1.03c1f081b5ac4p-2", "-0x1.55d3c7e3cbffap-6",
    "0x1.e1f506891babbp-11", "-0x1.a6d1f2a204a8cp-16", "0x1.f9d38a3763cc3p-22", "-0x1.b6e24f44b128fp-28",
    "0x1.20c62c2f2d7f5p-34"))


def phasors(nbin: int, delays) -> np.ndarray:
    """(2, *delays.shape, nbin/2 + 1) f64: exp(+2 pi i k s / nbin) for every
    delay s (bins) and harmonic k <= nbin/2 (any nbin <= 8192, odd ones with
    nbin/2 rounded down: the chirp-z statement's; 1/nbin and
    4/nbin are rounded f64 factors unless nbin is a power of two), in this f64
    operation order:

    * Veltkamp split s = sh + sl (c = s * 8193; sh = c - (c - s); sl = s - sh):
      sh has 40 significant bits, so k*sh and k*sl are exact (k < 2^13);
    * t = k sh - nbin rint((k sh) (1 / nbin))   (exact; |t| <= nbin/2, or an
      ulp of k sh / nbin beyond it when nbin is not a power of two)
    * y = (t + k sl) * (4 / nbin)          quarter turns, one rounding
    * q = rint(y); z = y - q               (exact; |z| <= 1/2)
    * w = z*z; sin = z * (S0 + w (S1 + ... w S8)); cos = C0 + w (C1 + ... w C8)
    * quadrant q mod 4: (cos, sin), (-sin, cos), (-cos, -sin), (sin, -cos).

    That is P0(k); the phasor itself (the GPU's ic_phasor) is P0(k) for k < 64
    and for multiples of 64, else the product P0(k mod 64) * P0(k - k mod 64)
    with separately rounded operations (re = a.re b.re - a.im b.im, im = a.re
    b.im + a.im b.re), so that a profile's phasors take 64 + nbin/128
    polynomial evaluations.  Within 7e-16 of the exact phasor for a
    power-of-two nbin (tests/test_phase_rotation.py checks it against x87 long
    double) and within 1e-15 otherwise (tests/test_phase_rotation_mr.py)."""
    m = nbin // 2
    k = np.arange(m + 1, dtype=np.float64)
    s = np.asarray(delays, dtype=np.float64)[..., None]
    nn = float(nbin)
    c = s * 8193.0
    sh = c - (c - s)
    sl = s - sh
    xh = k * sh
    xl = k * sl
    t = xh - nn * np.rint(xh * (1.0 / nn))
    y = (t + xl) * (4.0 / nn)
    q = np.rint(y)
    z = y - q
    w = z * z
    sp = np.full_like(z, _PH_S[8])
    cp = np.full_like(z, _PH_C[8])
    for j in range(7, -1, -1):
        sp = _PH_S[j] + w * sp
        cp = _PH_C[j] + w * cp
    sn = z * sp
    qi = q.astype(np.int64) & 3
    re = np.where(qi == 0, cp, np.where(qi == 1, -sn, np.where(qi == 2, -cp, sn)))
    im = np.where(qi == 0, sn, np.where(qi == 1, cp, np.where(qi == 2, -sn, -cp)))
    # the product form: P(k) = P0(k mod 64) P0(k - k mod 64) where both parts are nonzero
    ki = np.arange(m + 1)
    lo, hi = ki & 63, ki - (ki & 63)
    sel = (lo != 0) & (hi != 0)
    if sel.any():
        ar, ai = re[..., lo[sel]], im[..., lo[sel]]
        br, bi = re[..., hi[sel]], im[..., hi[sel]]
        re = re.copy()
        im = im.copy()
        re[..., sel] = ar * br - ai * bi
        im[..., sel] = ar * bi + ai * br
    return np.stack([re, im])


S8 = np.float32(0.7071067811865476)   # f32 of f64(sqrt(2)/2) = Re exp(-i pi/4) of the f32 twiddle table
S8_64 = np.float64(0.7071067811865476)   # the f64 stages of the chirp-z filter table (czt_filter)


def _dft4(ar, ai):
    """DFT of 4 points (lists of arrays) in the definition's order (module docstring)."""
    c0r, c0i = ar[0] + ar[2], ai[0] + ai[2]
    c1r, c1i = ar[0] - ar[2], ai[0] - ai[2]
    c2r, c2i = ar[1] + ar[3], ai[1] + ai[3]
    dr, di = ar[1] - ar[3], ai[1] - ai[3]
    c3r, c3i = di, -dr                       # -i (b1 - b3)
    return ([c0r + c2r, c1r + c3r, c0r - c2r, c1r - c3r],
            [c0i + c2i, c1i + c3i, c0i - c2i, c1i - c3i])


def _dft8(ar, ai):
    cr = [ar[q] + ar[q + 4] for q in range(4)] + [ar[q] - ar[q + 4] for q in range(4)]
    ci = [ai[q] + ai[q + 4] for q in range(4)] + [ai[q] - ai[q + 4] for q in range(4)]
    s8 = S8 if ar[0].dtype == np.float32 else S8_64
    t1, t2 = cr[5] + ci[5], ci[5] - cr[5]    # c5 * exp(-i pi/4)
    cr[5], ci[5] = t1 * s8, t2 * s8
    cr[6], ci[6] = ci[6], -cr[6]             # c6 * -i
    t1, t2 = ci[7] - cr[7], cr[7] + ci[7]    # c7 * exp(-3 i pi/4)
    cr[7], ci[7] = t1 * s8, -(t2 * s8)
    er, ei = _dft4(cr[:4], ci[:4])
    orr, oi = _dft4(cr[4:], ci[4:])
    return ([er[0], orr[0], er[1], orr[1], er[2], orr[2], er[3], orr[3]],
            [ei[0], oi[0], ei[1], oi[1], ei[2], oi[2], ei[3], oi[3]])


S3 = np.float32(0.8660254037844386)    # f32 of f64(sqrt(3)/2)
HALF = np.float32(0.5)
C51 = np.float32(0.30901699437494745)   # f32 of f64(cos(2 pi/5))
C52 = np.float32(-0.8090169943749475)   # f32 of f64(cos(4 pi/5))
S51 = np.float32(0.9510565162951535)    # f32 of f64(sin(2 pi/5))
S52 = np.float32(0.5877852522924731)    # f32 of f64(sin(4 pi/5))


def _dft3(ar, ai):
    tr, ti = ar[1] + ar[2], ai[1] + ai[2]
    dr, di = ar[1] - ar[2], ai[1] - ai[2]
    mr, mi = ar[0] - tr * HALF, ai[0] - ti * HALF
    er, ei = dr * S3, di * S3
    return ([ar[0] + tr, mr + ei, mr - ei], [ai[0] + ti, mi - er, mi + er])


def _dft5(ar, ai):
    t1r, t1i = ar[1] + ar[4], ai[1] + ai[4]
    t2r, t2i = ar[2] + ar[3], ai[2] + ai[3]
    d1r, d1i = ar[1] - ar[4], ai[1] - ai[4]
    d2r, d2i = ar[2] - ar[3], ai[2] - ai[3]
    m1r, m1i = (ar[0] + t1r * C51) + t2r * C52, (ai[0] + t1i * C51) + t2i * C52
    m2r, m2i = (ar[0] + t1r * C52) + t2r * C51, (ai[0] + t1i * C52) + t2i * C51
    e1r, e1i = d1r * S51 + d2r * S52, d1i * S51 + d2i * S52
    e2r, e2i = d1r * S52 - d2r * S51, d1i * S52 - d2i * S51
    return ([ar[0] + (t1r + t2r), m1r + e1i, m2r + e2i, m2r - e2i, m1r - e1i],
            [ai[0] + (t1i + t2i), m1i - e1r, m2i - e2r, m2i + e2r, m1i + e1r])


def _stockham(vr: np.ndarray, vi: np.ndarray, tw: np.ndarray, n: int | None = None):
    """FFT of the last axis (M complex points): Stockham stages in the order of
    :func:`stage_radices` (module docstring).  tw: exp(-2 pi i q / n), n = 2 M
    (the real rotation's table) unless given (the chirp-z transform's n = M)."""
    m = vr.shape[-1]
    if n is None:
        n = 2 * m
    ns = 1
    for r in stage_radices(m):
        g = m // r
        j = np.arange(g)
        k = j % ns
        ar = [vr[..., q * g:(q + 1) * g] for q in range(r)]
        ai = [vi[..., q * g:(q + 1) * g] for q in range(r)]
        if ns > 1:
            for q in range(1, r):
                idx = q * k * (n // (r * ns))
                wr, wi = tw[0][idx], tw[1][idx]
                ar[q], ai[q] = ar[q] * wr - ai[q] * wi, ar[q] * wi + ai[q] * wr
        if r == 8:
            yr, yi = _dft8(ar, ai)
        elif r == 4:
            yr, yi = _dft4(ar, ai)
        elif r == 5:
            yr, yi = _dft5(ar, ai)
        elif r == 3:
            yr, yi = _dft3(ar, ai)
        else:
            yr, yi = [ar[0] + ar[1], ar[0] - ar[1]], [ai[0] + ai[1], ai[0] - ai[1]]
        o = (j - k) * r + k
        nr = np.empty_like(vr)
        ni = np.empty_like(vi)
        for p in range(r):
            nr[..., o + p * ns] = yr[p]
            ni[..., o + p * ns] = yi[p]
        vr, vi = nr, ni
        ns *= r
    return vr, vi


def _pair(zkr, zki, zqr, zqi, c, sn, pkr, pki, pqr, pqi):
    """The half-length inputs of the inverse, conjugated (what it stores):
    conj(Z'_k) and conj(Z'_q) (q = M - k), from the transform's Z_k, Z_q in one
    linear map: with w = exp(-2 pi i k / N) = (c, sn) and the phasors P_k, P_q
    (their imaginary parts signed for the direction), the real spectrum
    X_k = E_k + w O_k, Y = P X and the inverse's packing Z' = E' + i conj(w) H'
    compose to
        Z'_k = A_k Z_k + B_k conj(Z_q),  Z'_q = A_q Z_q - conj(B_k) conj(Z_k),
        A_k = ((1 + sn) P_k + (1 - sn) conj(P_q)) / 2,
        A_q = ((1 + sn) P_q + (1 - sn) conj(P_k)) / 2,
        B_k = i c (P_k - conj(P_q)) / 2.
    Each Z' is the sum of its two terms; its conjugate's imaginary part is the
    sum of the two terms' negated imaginary parts ((-a) + (-b), which differs
    from -(a + b) only in the sign of a zero sum)."""
    h1 = (1.0 + sn) * 0.5
    h2 = (1.0 - sn) * 0.5
    hc = c * 0.5
    akr = h1 * pkr + h2 * pqr
    aki = h1 * pki - h2 * pqi
    aqr = h1 * pqr + h2 * pkr
    aqi = h1 * pqi - h2 * pki
    bkr = -(hc * (pki + pqi))
    bki = hc * (pkr - pqr)
    return ((akr * zkr - aki * zki) + (bkr * zqr + bki * zqi),
            (-(akr * zki + aki * zkr)) + (-(bki * zqr - bkr * zqi)),
            (aqr * zqr - aqi * zqi) + (bki * zki - bkr * zkr),
            (-(aqr * zqi + aqi * zqr)) + (-(bki * zkr + bkr * zki)))


def rotate(x: np.ndarray, ph: np.ndarray, sign: int, tw: np.ndarray | None = None,
           base: np.ndarray | None = None, any_length: bool | None = None) -> np.ndarray:
    """Rotate profiles x (..., nchan, nbin) f32 by their delays.

    ph: phasors(nbin, delays) for the nchan channels (axis -2 of x), or for
    every profile (delays of x's leading shape, e.g. (nsub, nchan)); sign +1 =
    dedisperse (y[j] = x[j + s]), -1 = dededisperse; base (..., nchan) f32 is
    subtracted first in f32 (remove_baseline's levels).  any_length (None = the
    IC_ANY_NBIN switch, :func:`any_length_enabled`): a length in 16..4096 that
    the rotation kernels do not serve takes the chirp-z statement
    (:func:`rotate_czt`); the lengths they serve keep this one's bits."""
    x = np.asarray(x, dtype=np.float32)
    n = x.shape[-1]
    if czt_selected(n, any_length):
        with np.errstate(invalid="ignore", over="ignore"):
            return rotate_czt(x, ph, sign, base)
    if not is_supported(n):
        raise ValueError("fractional dedispersion %s (nbin=%d)%s" % (UNSUPPORTED, n, any_hint(n, any_length)))
    if tw is None:
        tw = twiddles(n)
    tw = np.asarray(tw, dtype=np.float64).astype(np.float32)   # f32 of the f64 table
    with np.errstate(invalid="ignore", over="ignore"):   # NaN / Inf samples propagate
        return _rotate(x, ph, sign, tw, base)


def _rotate(x, ph, sign, tw, base):
    n = x.shape[-1]
    if base is not None:
        x = (x - np.asarray(base, dtype=np.float32)[..., None]).astype(np.float32)
    m = n // 2
    vr = np.ascontiguousarray(x[..., 0::2])
    vi = np.ascontiguousarray(x[..., 1::2])
    vr, vi = _stockham(vr, vi, tw)
    pr = np.asarray(ph[0]).astype(np.float32)
    pi = np.asarray(ph[1] if sign > 0 else -ph[1]).astype(np.float32)
    k = np.arange(1, m // 2 + 1)
    q = m - k
    zkr, zki, zqr, zqi = vr[..., k], vi[..., k], vr[..., q], vi[..., q]
    zkr2, zki2, zqr2, zqi2 = _pair(zkr, zki, zqr, zqi, tw[0][k], tw[1][k], pr[..., k], pi[..., k], pr[..., q],
                                   pi[..., q])
    x0 = vr[..., 0] + vi[..., 0]
    xm = vr[..., 0] - vi[..., 0]
    y0 = x0 * pr[..., 0]
    ym = xm * pr[..., m]
    ur = np.empty_like(vr)
    ui = np.empty_like(vi)
    ur[..., 0] = (y0 + ym) * 0.5
    ui[..., 0] = -((y0 - ym) * 0.5)
    ur[..., q] = zqr2      # conj(Z'_q), conj(Z'_k) (_pair)
    ui[..., q] = zqi2
    ur[..., k] = zkr2      # k = M/2 pairs with itself: the k values are stored last
    ui[..., k] = zki2
    rr, ri = _stockham(ur, ui, tw)
    inv = np.float32(1.0 / m)
    out = np.empty(x.shape, dtype=np.float32)
    out[..., 0::2] = rr * inv
    out[..., 1::2] = (-ri) * inv
    for a in (vr, vi, ur, ui, rr, ri):
        assert a.dtype == np.float32   # every operation of the definition is f32
    return out


# ---------------------------------------------------------------------------
# The opt-in chirp-z statement: any nbin in 16..4096 (module docstring, "Any
# length")

CZT_NBIN_MIN, CZT_NBIN_MAX = 16, 4096    # the library's kCztMin / kCztMax (csrc/ic_internal.h)
ANY_NBIN_ENV = "IC_ANY_NBIN"


def any_length_enabled() -> bool:
    """The process-wide opt-in switch of the host layer: the environment
    variable IC_ANY_NBIN (unset, empty or ``0`` = off).  Read at every call."""
    import os
    return os.environ.get(ANY_NBIN_ENV, "") not in ("", "0")


def kernel_supported(nbin: int) -> bool:
    """The lengths the default rotation kernels serve (the library's
    rotate_supported): a power of two in 64..8192, or a mixed-radix length."""
    return (64 <= nbin <= 8192 and (nbin & (nbin - 1)) == 0) or mr_supported(nbin)


def czt_selected(nbin: int, any_length: bool | None = None) -> bool:
    """The chirp-z statement serves nbin: the opt-in is on (any_length, None =
    :func:`any_length_enabled`), 16 <= nbin <= 4096, and the default kernels do
    not serve it (those lengths keep their statement and their bits)."""
    if any_length is None:
        any_length = any_length_enabled()
    return bool(any_length) and CZT_NBIN_MIN <= nbin <= CZT_NBIN_MAX and not kernel_supported(nbin)


def any_hint(nbin: int, any_length: bool | None = None) -> str:
    """What a refusal adds to UNSUPPORTED: the switch, or its range when it is on."""
    if any_length is None:
        any_length = any_length_enabled()
    if any_length:
        return "; with any_length / %s, any other nbin in %d..%d" % (ANY_NBIN_ENV, CZT_NBIN_MIN, CZT_NBIN_MAX)
    if CZT_NBIN_MIN <= nbin <= CZT_NBIN_MAX:
        return "; any_length=True or %s=1 opts in to the chirp-z rotation of any nbin in %d..%d" % (
            ANY_NBIN_ENV, CZT_NBIN_MIN, CZT_NBIN_MAX)
    return ""


def czt_length(n: int) -> int:
    """L: the smallest power of two >= 2 n - 1."""
    L = 1
    while L < 2 * n - 1:
        L *= 2
    return L


def czt_chirp(n: int) -> np.ndarray:
    """(2, n) f64: w[j] = exp(-i pi (j^2 mod 2n) / n) = twiddles(2n)[j^2 mod 2n]
    (the reduction is exact integer arithmetic)."""
    j = np.arange(n, dtype=np.int64)
    return twiddles(2 * n)[:, (j * j) % (2 * n)]


def czt_filter(n: int) -> np.ndarray:
    """(2, L) f32: B = FFT_L(b), b[j] = b[L - j] = conj(w[j]) (j < n), 0
    elsewhere, by the module's Stockham stages run in f64 (f64 chirp, f64
    twiddles(L), f64 sqrt(2)/2), then rounded to f32."""
    L = czt_length(n)
    w = czt_chirp(n)
    br = np.zeros(L)
    bi = np.zeros(L)
    j = np.arange(n)
    br[j], bi[j] = w[0], -w[1]
    br[(L - j) % L], bi[(L - j) % L] = w[0], -w[1]
    Br, Bi = _stockham(br, bi, twiddles(L), L)
    assert Br.dtype == np.float64
    return np.stack([Br, Bi]).astype(np.float32)


def _cmul(ar, ai, wr, wi):
    """The rotation's complex product (a.r w.r - a.i w.i, a.r w.i + a.i w.r)."""
    return ar * wr - ai * wi, ar * wi + ai * wr


def _czt_conv(ar, ai, B, twL, L):
    """D = FFT_L(conj(FFT_L(a, zero-padded to L) B)) for a (..., n) f32, the
    chirped input: D[k] = L conj(DFT_n)[k] / w[k] for k < n (module docstring,
    "Any length", step 2)."""
    n = ar.shape[-1]
    vr = np.zeros(ar.shape[:-1] + (L,), np.float32)
    vi = np.zeros(ar.shape[:-1] + (L,), np.float32)
    vr[..., :n], vi[..., :n] = ar, ai
    vr, vi = _stockham(vr, vi, twL, L)
    cr, ci = _cmul(vr, vi, B[0], B[1])
    return _stockham(cr, -ci, twL, L)


def rotate_czt(x: np.ndarray, ph: np.ndarray, sign: int, base: np.ndarray | None = None) -> np.ndarray:
    """The chirp-z statement of the rotation (module docstring, "Any length"):
    x (..., nchan, n) f32, ph = phasors(n, delays), any n >= 2 (the library
    serves 16..4096)."""
    x = np.asarray(x, dtype=np.float32)
    n = x.shape[-1]
    L = czt_length(n)
    h = n // 2
    w = czt_chirp(n).astype(np.float32)
    B = czt_filter(n)
    twL = twiddles(L).astype(np.float32)
    invL = np.float32(1.0 / L)
    invn = np.float32(1.0 / n)
    if base is not None:
        x = (x - np.asarray(base, dtype=np.float32)[..., None]).astype(np.float32)
    # X = DFT_n(x)
    dr, di = _czt_conv(x * w[0], x * w[1], B, twL, L)
    xr, xi = _cmul(dr[..., :n], -di[..., :n], w[0], w[1])
    xr, xi = xr * invL, xi * invL
    # Y = X P: harmonic k <= n/2 takes (P.r, sign P.i)[k], k > n/2 its conjugate at n - k
    k = np.arange(n)
    kk = np.where(k <= h, k, n - k)
    pr = np.asarray(ph[0]).astype(np.float32)[..., kk]
    pi = np.asarray(ph[1] if sign > 0 else -ph[1]).astype(np.float32)[..., kk]
    pi = np.where(k <= h, pi, -pi)
    yr, yi = _cmul(xr, xi, pr, pi)
    if n % 2 == 0:   # the Nyquist harmonic takes P.r only
        yr[..., h], yi[..., h] = xr[..., h] * pr[..., h], xi[..., h] * pr[..., h]
    # y = Re conj(DFT_n(conj(Y))) / n
    vr, vi = _cmul(yr, -yi, w[0], w[1])
    dr, di = _czt_conv(vr, vi, B, twL, L)
    orr, _ = _cmul(dr[..., :n], -di[..., :n], w[0], w[1])
    out = (orr * invL) * invn
    for a in (dr, di, xr, xi, yr, yi, out):
        assert a.dtype == np.float32   # every operation of the definition is f32
    return out
