"""Inputs shared by the quantised-download tests (test_encode_host.py,
test_encode_gpu.py): seeded, built once per process, never modified."""
import numpy as np

NBINS = (64, 100, 128, 1024, 8192)      # the supported lengths under test; 50 adds the unvectorised path
TIE_SAMPLES = (0.5, 1.5, 2.5, -1.5)     # with scl 1 and offs 0: rint must give 0, 2, 2, -2
TIE_Q = (0, 2, 2, -2)
_CACHE = {}


def tie_profile(nbin):
    """Minimum -32767 and maximum 32767 (scl == 1, offs == 0 exactly), then the
    ties that tell round-half-even from floor(x + 0.5), then integers + 0.25."""
    rng = np.random.default_rng(11)
    p = (rng.integers(-30000, 30000, nbin) + 0.25).astype(np.float32)
    p[0], p[1] = -32767.0, 32767.0
    p[2:6] = TIE_SAMPLES
    return p


def edge_cube(nbin):
    """(3, 5, nbin) f32, one kind of profile per row (see EDGE_ROWS)."""
    if nbin in _CACHE:
        return _CACHE[nbin]
    rng = np.random.default_rng(1000 + nbin)

    def noise(scale, mean=0.0):
        return (mean + scale * rng.standard_normal(nbin)).astype(np.float32)

    rows = [noise(1e-3), noise(1e-1, 7.0), noise(1.0, -3.0), noise(1e2), noise(1e4, 1e5), noise(1e6)]
    rows.append(np.full(nbin, 3.25, np.float32))                 # a constant profile
    rows.append(np.zeros(nbin, np.float32))                      # all +0
    p = noise(5.0)
    p[nbin // 3] = np.nan                                        # one NaN
    rows.append(p)
    p = noise(5.0)
    p[nbin - 1] = np.inf                                         # one +inf
    rows.append(p)
    p = noise(5.0)
    p[1], p[nbin // 2] = -np.inf, np.inf                         # both infinities
    rows.append(p)
    p = noise(1e30)
    p[0], p[nbin - 2] = 3e38, -3e38                              # +-3e38: mx - mn overflows f32, not f64
    rows.append(p)
    rows.append(tie_profile(nbin))
    sub = np.float32(1e-45)                                      # the smallest subnormal
    rows.append((rng.integers(-4000000, 4000000, nbin).astype(np.float32) * sub).astype(np.float32))
    rows.append((rng.integers(0, 3, nbin).astype(np.float32) * sub).astype(np.float32))   # scl underflows: 1
    cube = np.ascontiguousarray(np.stack(rows).reshape(3, 5, nbin))
    assert np.count_nonzero(cube[2, 3]) and np.all(np.abs(cube[2, 3:]) < np.finfo(np.float32).tiny)
    cube.setflags(write=False)
    _CACHE[nbin] = cube
    return cube


def random_cube():
    """(16, 64, 1024) f32, seed 7: unit noise times a profile amplitude uniform in
    0.1 .. 1e4."""
    if "random" not in _CACHE:
        rng = np.random.default_rng(7)
        amp = rng.uniform(0.1, 1e4, size=(16, 64, 1)).astype(np.float32)
        cube = (amp * rng.standard_normal((16, 64, 1024)).astype(np.float32)).astype(np.float32)
        cube.setflags(write=False)
        _CACHE["random"] = cube
    return _CACHE["random"]


def host_quantise(cube):
    """psrfits.quantise of a (nsub, nchan, nbin) cube, the reference of every
    comparison (host code that predates the GPU encode): (q, scl, offs) without
    the polarisation axis."""
    from iterative_cleaner_amd import psrfits
    key = ("q", id(cube))
    if key not in _CACHE:
        with np.errstate(all="ignore"):
            q, scl, offs = psrfits.quantise(np.asarray(cube)[:, None])
        _CACHE[key] = (cube, np.ascontiguousarray(q[:, 0]), np.ascontiguousarray(scl[:, 0]),
                       np.ascontiguousarray(offs[:, 0]))
    return _CACHE[key][1:]


def quantise_all_f32(cube):
    """The shortcut the encode must not take: psrfits.quantise with every step
    in f32."""
    d = np.asarray(cube, np.float32)
    mn, mx = d.min(axis=-1), d.max(axis=-1)
    offs = (np.float32(0.5) * (mx + mn)).astype(np.float32)
    scl = ((mx - mn) / np.float32(65534.0)).astype(np.float32)
    scl = np.where((scl > 0) & np.isfinite(scl), scl, np.float32(1.0)).astype(np.float32)
    x = np.rint((d - offs[..., None]) / scl[..., None])
    return np.clip(np.nan_to_num(x), -32767, 32767).astype(np.int16), scl, offs
