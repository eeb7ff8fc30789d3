"""Shared inputs of the standard-template tests (host and GPU)."""
import numpy as np


def gauss(n, centre, sigma, amp):
    """A circular Gaussian over n bins (f64)."""
    d = (np.arange(n, dtype=np.float64) - centre + n / 2.0) % n - n / 2.0
    return amp * np.exp(-0.5 * (d / sigma) ** 2)


def pulse(n):
    """The test pulse: a main component at 0.3 n and a weaker one at 0.42 n, f32."""
    return (10000.0 * (gauss(n, 0.3 * n, n / 32.0, 1.0) + gauss(n, 0.42 * n, n / 20.0, 0.35))).astype(np.float32)


def delayed(A, d):
    """A seen d bins early, S[j] = A[j + d], by the written f32 rotation: the
    alignment of S against A must recover d."""
    from iterative_cleaner_amd import phase_rotation as pr
    A = np.asarray(A, np.float32)
    return pr.rotate(A[None, :], pr.phasors(A.shape[0], [float(d)]), +1, any_length=False)[0]


def noisy(A, seed, sigma=40.0):
    """A plus seeded Gaussian noise (0.4 % of the pulse's peak), f32."""
    rng = np.random.default_rng(seed)
    return (np.asarray(A, np.float64) + sigma * rng.standard_normal(A.shape[0])).astype(np.float32)
