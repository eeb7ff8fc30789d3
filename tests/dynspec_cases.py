"""Shared inputs of the dynamic-spectrum tests (test_dynspec_host.py,
test_dynspec_gpu.py): seeded templates, profiles and small archives, and the
module's answers computed once per case."""
import numpy as np

F = np.float32

ONESHOT_NBINS = (4, 16, 63, 64, 65, 100, 1024, 4096, 8192)
ONESHOT_NPROFS = (1, 5, 67)


def template(nbin, seed=0):
    """A Gaussian pulse at phase 0.3 (width nbin / 16, at least one bin) on a
    small seeded ripple, f32: never constant."""
    rng = np.random.default_rng(1000 + seed)
    i = np.arange(nbin, dtype=np.float64)
    sig = max(nbin / 16.0, 1.0)
    T = 3.0 * np.exp(-0.5 * ((i - 0.3 * nbin) / sig) ** 2) + 0.01 * rng.standard_normal(nbin) + 0.25
    return T.astype(F)


def profiles(nbin, nprof, seed=0):
    """(T, X (nprof, nbin) f32, w (nprof,) f32, g, b): X = g T + b + N(0, 1) with
    seeded gains g in 0.5..4 and baselines b in -20..20; weights 1 but for a few
    fractional ones (never 0)."""
    rng = np.random.default_rng(2000 + 7 * nbin + nprof + seed)
    T = template(nbin, seed)
    g = rng.uniform(0.5, 4.0, nprof)
    b = rng.uniform(-20.0, 20.0, nprof)
    X = (g[:, None] * T.astype(np.float64)[None, :] + b[:, None] + rng.standard_normal((nprof, nbin))).astype(F)
    w = np.ones(nprof, F)
    w[::4] = F(0.5)
    return T, X, w, g, b


def edge_profiles(nbin=100, nprof=5):
    """profiles() with a zero-weight row of NaNs, a live row holding an Inf and
    a second zero-weight row of ordinary samples."""
    T, X, w, _, _ = profiles(nbin, nprof, seed=9)
    X[1, :] = np.nan
    w[1] = 0
    X[2, nbin // 3] = np.inf
    w[2] = 1
    w[4] = 0
    return T, X, w


_want = {}


def module_profiles(nbin, nprof):
    """dynspec.profiles of profiles(nbin, nprof), computed once."""
    from iterative_cleaner_amd import dynspec as ds
    if (nbin, nprof) not in _want:
        T, X, w, _, _ = profiles(nbin, nprof)
        _want[nbin, nprof] = ds.profiles(T, X, w)
    return _want[nbin, nprof]


def archive(nsub, nchan, nbin, seed=5, rfi=0.1):
    """(raw (nsub, nchan, nbin) f32, w0, shift) of a synthetic archive with some
    interference and dead profiles, so that a run ends with zero weights."""
    from iterative_cleaner_amd import synth
    data, w0, shift = synth.make_cube(nsub, nchan, nbin, seed, rfi)
    w0[0, 0] = 0                       # at least one masked profile, whatever the seed
    return np.ascontiguousarray(data[:, 0]), w0, shift


def same(got, want, what=""):
    """amp, err and base equal bit for bit; a NaN equals any NaN."""
    from helpers import bits_equal_nan
    for key in ("amp", "err", "base"):
        g, w = np.asarray(got[key]), np.asarray(want[key])
        assert g.shape == w.shape and g.dtype == np.float64 == w.dtype, (what, key, g.shape, w.shape)
        if not bits_equal_nan(g, w):
            gi, wi = np.ascontiguousarray(g).view(np.int64), np.ascontiguousarray(w).view(np.int64)
            bad = np.argwhere((gi != wi) & ~(np.isnan(g) & np.isnan(w)))
            raise AssertionError("%s: %s differs at %d places, first %s: %r != %r" % (
                what, key, len(bad), bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]))
    return True
