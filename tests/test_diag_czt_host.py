"""The chirp-z statistics FFT's numpy statement (iterative_cleaner_amd/diag_czt.py)
against numpy's rfft: within 1e-12 relative at lengths that cover an odd half
length (18, 50, 250), odd and prime lengths (17, 33, 125, 129, 997, 2047, 2049,
4095), both sides of a convolution length's step (510 / 514, 2047 / 2049 / 2050,
4094 / 4095) and the ends of the range; the convolution length of each; the
chirp's index reduced in integers."""
import numpy as np
import pytest

from iterative_cleaner_amd import diag_czt

# nbin: L
LENGTHS = {16: 16, 17: 64, 18: 32, 33: 128, 50: 64, 56: 64, 100: 128, 125: 256, 129: 512, 250: 256, 448: 512,
           500: 512, 510: 512, 514: 1024, 997: 2048, 2047: 4096, 2049: 8192, 2050: 4096, 2500: 4096, 4094: 4096,
           4095: 8192}


@pytest.mark.parametrize("nbin", sorted(LENGTHS))
def test_model_matches_numpy_rfft(nbin):
    rng = np.random.default_rng(nbin)
    v = (rng.standard_normal((6, nbin)) * 50).astype(np.float32).astype(np.float64)
    v[3] = 0.0
    v[3, nbin // 3] = 7.0       # a single spike: a flat spectrum
    v[4] = 0.0                  # all zero
    v[5, nbin - 1] = np.nan
    got = diag_czt.fftmax(v)
    with np.errstate(all="ignore"):
        want = np.abs(np.fft.rfft(v, axis=-1)).max(axis=-1)
    err = np.abs(got[:4] - want[:4]) / want[:4]
    print("nbin", nbin, "max rel error", err.max())
    assert np.all(err <= 1e-12)
    assert got[4] == 0.0 and not np.signbit(got[4])
    assert np.isnan(got[5]) and np.isnan(want[5])
    # every bin, not only the largest: within 1e-12 of the row's largest bin
    sp = diag_czt.spectrum(v[:4])
    ref = np.fft.rfft(v[:4], axis=-1)
    assert sp.shape == ref.shape
    assert np.all(np.abs(sp - ref) <= 1e-12 * np.abs(ref).max(axis=-1, keepdims=True))


@pytest.mark.parametrize("nbin", sorted(LENGTHS))
def test_convolution_length(nbin):
    m = diag_czt.points(nbin)
    assert m == (nbin if nbin % 2 else nbin // 2)
    L = diag_czt.length(nbin)
    assert L == LENGTHS[nbin]
    assert L & (L - 1) == 0 and L >= 2 * m - 1 and L // 2 < 2 * m - 1
    assert diag_czt.filter(m).shape == (L,) and diag_czt.chirp(m).shape == (m,)


def test_chirp_index_is_reduced_in_integers():
    """j^2 reaches 1e6 at m = 997: an angle formed as pi j^2 / m in f64 is
    rounded at 4.5e-13 there; the reduced index keeps the chirp within an ulp
    or two of a long double evaluation."""
    m = 997
    j = np.arange(m, dtype=np.int64)
    r = ((j * j) % (2 * m)).astype(np.longdouble)
    ang = -np.longdouble("3.14159265358979323846264338327950288") * r / m
    want_r, want_i = np.cos(ang), np.sin(ang)
    w = diag_czt.chirp(m)
    assert np.all(np.abs(w.real - want_r.astype(np.float64)) <= 4e-16)
    assert np.all(np.abs(w.imag - want_i.astype(np.float64)) <= 4e-16)
    # the unreduced f64 angle reaches 3131 rad, whose ulp is 4.5e-13: visibly worse
    naive = np.exp(-1j * np.pi * (j * j).astype(np.float64) / m)
    assert np.abs(naive - w).max() > 1e-13 > np.abs(np.abs(w) - 1.0).max()
