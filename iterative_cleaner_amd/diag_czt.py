"""The chirp-z statistics FFT in numpy: what k_diag_czt computes for fftmax.

The diagnostics kernel of the profile lengths that are neither a power of two
nor mixed-radix (ic_internal.h diag_czt_supported: 129..4096, odd lengths to
2048; the transform itself is stated for any length) replaces the
generic kernel's direct O(n^2) DFT by a Bluestein (chirp-z) transform in f64 on
power-of-two Stockham stages.  This module is the written reference for its
index rules (the chirp's integer reduction, the wrap of the filter, an odd
half length, an odd length); the kernel is pinned to numpy's rfft within 1e-9,
not to this module bit for bit.

fftmax(v) = max_k |rfft(v)_k| of a real row v of n samples (the caller has
already subtracted the mean):

  even n   m = n/2, z[q] = v[2q] + i v[2q+1], Z = DFT_m(z), then the real
           spectrum's pair step for k = 0 .. m,
             X_k = (Z_k + conj Z_(m-k))/2 - (i/2) W^k (Z_k - conj Z_(m-k)),
           W = exp(-2 pi i/n), indices mod m.  m may be odd (n = 18, 50, 250):
           then no k pairs with itself, and nothing else changes.
  odd n    m = n, X = DFT_n(v), bins 0 .. (n-1)/2.

DFT_m by Bluestein: with the chirp w[j] = exp(-i pi (j^2 mod 2m)/m) (the index
reduced as an integer) and L the smallest power of two >= 2m - 1,
  a = z w zero-padded to L, A = FFT_L(a), Y = A B with the per-length filter
  B = FFT_L(b), b[j] = b[L - j] = conj(w[j]) for j < m, y = IFFT_L(Y) as
  conj(FFT_L(conj Y))/L, and DFT_m(z)[k] = w[k] y[k], k < m.
The FFT_L are phase_rotation's Stockham stages (radix 8 while three levels
remain, then 4 or 2) run in f64."""
from __future__ import annotations

import numpy as np

from .phase_rotation import _stockham, czt_length, twiddles


def points(n: int) -> int:
    """m: the length of the Bluestein DFT of an n-sample row."""
    return n if n % 2 else n // 2


def length(n: int) -> int:
    """L of an n-sample row: czt_length of its DFT length."""
    return czt_length(points(n))


def chirp(m: int) -> np.ndarray:
    """(m,) complex128: w[j] = exp(-i pi (j^2 mod 2m)/m) = twiddles(2m)[j^2 mod 2m]."""
    j = np.arange(m, dtype=np.int64)
    t = twiddles(2 * m)[:, (j * j) % (2 * m)]
    return t[0] + 1j * t[1]


def _fft(a: np.ndarray, L: int) -> np.ndarray:
    r, i = _stockham(np.ascontiguousarray(a.real), np.ascontiguousarray(a.imag), twiddles(L), L)
    return r + 1j * i


def filter(m: int) -> np.ndarray:   # noqa: A001 - the transform's own name for it
    """(L,) complex128: B = FFT_L(b), b[j] = b[L - j] = conj(w[j]), j < m, 0 elsewhere."""
    L = czt_length(m)
    w = chirp(m)
    b = np.zeros(L, np.complex128)
    j = np.arange(m)
    b[j] = np.conj(w)
    b[(L - j) % L] = np.conj(w)
    return _fft(b, L)


def dft(z: np.ndarray) -> np.ndarray:
    """DFT_m of the last axis of z (complex128) by Bluestein."""
    m = z.shape[-1]
    L = czt_length(m)
    w = chirp(m)
    a = np.zeros(z.shape[:-1] + (L,), np.complex128)
    a[..., :m] = z * w
    Y = _fft(a, L) * filter(m)
    y = np.conj(_fft(np.conj(Y), L)) / L
    return w * y[..., :m]


def spectrum(v: np.ndarray) -> np.ndarray:
    """rfft of the last axis of v (f64, n samples): n//2 + 1 bins."""
    v = np.asarray(v, np.float64)
    n = v.shape[-1]
    if n % 2:
        return dft(v.astype(np.complex128))[..., :(n - 1) // 2 + 1]
    m = n // 2
    Z = dft(v[..., 0::2] + 1j * v[..., 1::2])
    k = np.arange(m + 1)
    t = twiddles(n)[:, k % n]
    W = t[0] + 1j * t[1]
    Zk, Zc = Z[..., k % m], np.conj(Z[..., (m - k) % m])
    return 0.5 * (Zk + Zc) - 0.5j * W * (Zk - Zc)


def fftmax(v: np.ndarray) -> np.ndarray:
    """max_k |rfft(v)_k| over the last axis: NaN when a sample is not finite
    (as numpy's rfft spreads it over every bin), exactly 0 for an all-zero row."""
    v = np.asarray(v, np.float64)
    with np.errstate(all="ignore"):
        out = np.abs(spectrum(v)).max(axis=-1)
    return np.where(np.isfinite(v).all(axis=-1), out, np.nan)
