#!/usr/bin/env python
"""Golden fixtures of the reference's clean() at profile lengths only the
opt-in chirp-z rotation serves (fractional delays at nbin = 56, 100, 125, 448,
500: iterative_cleaner_amd/phase_rotation.py rotate_czt).

Runs where make_golden.py runs, through its ``run_clean_case`` (the reference
imported with the stub psrchive; nothing of the reference is copied), with the
host layer's switch IC_ANY_NBIN set: the stand-in archive then dedisperses by
the chirp-z statement at these lengths.

The cases cover an odd length (125), lengths that are no multiple of 8 (100,
500), multiples of 8 whose half has a prime factor 7 (56, 448), the
convolution lengths L = 128, 256 and 1024; per-channel and per-profile delays;
the residual archive (-u), a pulse region, f64 data with fractional weights,
and an archive stored dedispersed.

The files are named ``any_clean_<case>.npz``, not ``clean_<case>.npz``: the
tests that run every ``clean_*.npz`` fixture also run the C oracle on it, and
the oracle's rotation is written for powers of two only.

usage: python tests/golden/make_golden_any.py [--out tests/golden]
"""
from __future__ import annotations

import argparse
import os
import shutil
import sys
import tempfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402

# name -> (positional arguments of run_clean_case after the name, keywords)
CASES = {
    "s6x24x100_fft": ((6, 24, 100, 3, 0.1), dict(frac_delay=True, keep_cubes=False)),
    "s5x20x125_fft_pp_u": ((5, 20, 125, 7, 0.1), dict(frac_delay2=True, extra_args=("-u",))),
    "s4x16x500_fft_pr": ((4, 16, 500, 9, 0.1), dict(frac_delay=True, extra_args=("-r", "0.5", "150", "250"),
                                                    keep_cubes=False)),
    "s4x12x448_fft_ded": ((4, 12, 448, 21, 0.2), dict(frac_delay=True, stored_dedispersed=True,
                                                      keep_cubes=False)),
    "s6x20x56_fft_f64": ((6, 20, 56, 5, 0.1), dict(frac_delay=True, data_f64=True, frac_weights=True,
                                                   keep_cubes=False)),
}
SMALLEST = "s4x12x448_fft_ded"  # the smallest file: the one tests/test_golden_regen_any.py regenerates
SWITCH = "IC_ANY_NBIN"          # phase_rotation.any_length_enabled


def fixture_path(name, out_dir=HERE):
    return os.path.join(out_dir, "any_clean_%s.npz" % name)


def run_case(ic, name, workdir, out_dir):
    """run_clean_case writes clean_<name>.npz; it is made in workdir and moved."""
    pos, kw = CASES[name]
    before = os.environ.get(SWITCH)
    os.environ[SWITCH] = "1"
    try:
        make_golden.run_clean_case(ic, name, *pos, workdir=workdir, out_dir=workdir, **kw)
    finally:
        if before is None:
            del os.environ[SWITCH]
        else:
            os.environ[SWITCH] = before
    shutil.move(os.path.join(workdir, "clean_%s.npz" % name), fixture_path(name, out_dir))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    ic = make_golden.import_reference()
    with tempfile.TemporaryDirectory() as wd:
        for name in CASES:
            run_case(ic, name, wd, a.out)


if __name__ == "__main__":
    main()
