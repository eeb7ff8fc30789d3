"""Inputs shared by the hot-bin tests (host and GPU): the 6 x 8 profiles of the
kernel parity test with every edge case of the definition among them, and the
parameter sets they are run under."""
import numpy as np

NPROF = 48          # 6 x 8
BIG = np.float32(100.0)


def base(nbin, k):
    """A bounded deterministic profile: nothing in it stands out at threshold 4
    (its deviations stay below 2.1, the limit above 4)."""
    j = np.arange(nbin, dtype=np.float64)
    return np.sin(0.7 * j + 0.37 * k).astype(np.float32)


def param_sets(nbin):
    """name -> (widen, threshold, on_start, on_end, rounds)."""
    a, b = nbin // 4, nbin // 4 + nbin // 8
    return {
        "plain": (0, 4.0, a, b, 4),
        "wrapped, widened": (1, 4.0, nbin - 5, 6, 4),
        "one round": (0, 4.0, a, b, 1),
        "no window, 8 rounds": (0, 2.5, 0, 0, 8),
        "low threshold": (0, 0.5, a, b, 4),
        "odd off-pulse count": (0, 4.0, a, b + 1, 4),
    }


def off_bins(nbin, o, on_start, on_end):
    """The stored off-pulse bins of a profile with offset o (no widening)."""
    j = np.arange(nbin)
    L = (on_end - on_start) % nbin
    return j[((j - o) % nbin - on_start) % nbin >= L]


def profiles(nbin, seed=5):
    """(X (48, nbin) f32, w (48,) f32, offsets (48,) int32, names): the edge
    cases are laid out for the "plain" parameter set."""
    _, _, a, b, _ = param_sets(nbin)["plain"]
    rng = np.random.default_rng(seed + nbin)
    X = np.empty((NPROF, nbin), np.float32)
    w = np.ones(NPROF, np.float32)
    # offsets: zero, ordinary, nbin - 1, beyond nbin, negative
    offs = np.array([(0, 3, nbin - 1, nbin + 2, -5, 17)[k % 6] for k in range(NPROF)], np.int32)
    names = []
    for k in range(NPROF):
        off = off_bins(nbin, int(offs[k]) % nbin, a, b)
        on = np.setdiff1d(np.arange(nbin), off)
        cap = len(off) // 4
        x = base(nbin, k)
        name = "noise"
        if k == 0:
            name = "bounded, nothing hot"
        elif k == 1:
            x[:] = 2.5
            name = "constant (mad == 0)"
        elif k == 2:
            x[:] = -1.0
            x[off[3]] = BIG
            name = "constant but one bin (mad == 0)"
        elif k == 3:
            x[off[5]] = np.nan
            x[off[1]] = BIG
            name = "NaN off-pulse"
        elif k == 4:
            x[off[-1]] = np.inf
            name = "Inf off-pulse"
        elif k == 5:
            x[on[0]] = np.nan
            x[on[-1]] = -np.inf
            x[off[2]] = BIG
            x[off[-2]] = -BIG
            name = "NaN and Inf on-pulse only, two hot bins"
        elif k == 6:
            x[off[::4][:cap]] = BIG
            name = "exactly the cap"
        elif k == 7:
            x[off[::3][:cap + 1]] = BIG
            name = "one over the cap"
        elif k == 8:
            w[k] = 0.0
            x[off[4]] = BIG
            name = "w0 == 0"
        elif k == 9:
            x[on] = 50.0
            name = "on-pulse spikes only"
        elif k == 10:
            x[off[0]] = BIG
            x[off[-1]] = BIG
            x[off[len(off) // 2]] = -BIG
            name = "first and last off-pulse bins"
        elif k == 11:
            x[:] = np.where(np.arange(nbin) % 2, 1.0, -1.0)
            x[off[7]] = BIG
            name = "tied medians (+-1), one hot"
        elif k == 12:
            x[:] = np.where(np.arange(nbin) % 2, 0.0, -0.0)
            x[off[1]] = 3.0
            name = "signed zeros (mad == 0)"
        elif k == 13:
            x[:] = rng.standard_cauchy(nbin).astype(np.float32)
            name = "heavy tails (later rounds find more)"
        elif k == 14:
            x[:] = (1e30 * rng.standard_normal(nbin)).astype(np.float32)
            x[off[3]] = np.float32(3e38)
            name = "huge values"
        elif k == 15:
            x[:] = (1e-40 * rng.standard_normal(nbin)).astype(np.float32)
            x[off[3]] = np.float32(1e-38)
            name = "subnormal values"
        else:
            x[:] = rng.standard_normal(nbin).astype(np.float32)
            nsp = k % 4
            if nsp:
                hit = rng.choice(off, size=nsp, replace=False)
                x[hit] += (rng.choice([-1.0, 1.0], size=nsp) * rng.uniform(8.0, 40.0, size=nsp)).astype(np.float32)
            name = "noise + %d spikes" % nsp
        X[k] = x
        names.append(name)
    return X, w, offs, names
