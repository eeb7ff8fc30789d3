#!/usr/bin/env python
"""Golden fixtures of the reference's clean() at mixed-radix profile lengths
(fractional delays at nbin = 96, 120, 200, 1000, 1536: the FFT phase rotation
of iterative_cleaner_amd/phase_rotation.py with radix-3 and radix-5 stages).

Runs where make_golden.py runs, through its ``run_clean_case`` (the reference
imported with the stub psrchive; nothing of the reference is copied).

The cases cover radix 3 (96, 1536), radix 5 (200, 1000) and both (120); each
power-of-two leftover 2 (96: 8, 2, 3), 4 (120, 200, 1000, 1536) and 8; odd
stages with Ns > 1 (all); stages with more than 64 butterflies (1000, 1536);
per-channel and per-profile delays; the residual archive (-u), a pulse region,
f64 data with fractional weights, and an archive stored dedispersed.

The files are named ``mr_clean_<case>.npz``, not ``clean_<case>.npz``: the
tests that run every ``clean_*.npz`` fixture also run the C oracle on it, and
the oracle's rotation is written for powers of two only.

usage: python tests/golden/make_golden_mr.py [--out tests/golden]
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
    "s6x24x96_fft": ((6, 24, 96, 3, 0.1), dict(frac_delay=True)),
    "s5x20x200_fft_pp_u": ((5, 20, 200, 7, 0.1), dict(frac_delay2=True, extra_args=("-u",))),
    "s6x20x120_fft_f64": ((6, 20, 120, 5, 0.1), dict(frac_delay=True, data_f64=True, frac_weights=True,
                                                     keep_cubes=False)),
    "s4x16x1000_fft_pr": ((4, 16, 1000, 9, 0.1), dict(frac_delay=True, extra_args=("-r", "0.5", "300", "500"),
                                                      keep_cubes=False)),
    "s4x12x1536_fft_ded": ((4, 12, 1536, 21, 0.2), dict(frac_delay=True, stored_dedispersed=True,
                                                        keep_cubes=False)),
}
SMALLEST = "s4x12x1536_fft_ded"   # the smallest file: the one tests/test_golden_regen_mr.py regenerates


def fixture_path(name, out_dir=HERE):
    return os.path.join(out_dir, "mr_clean_%s.npz" % name)


def run_case(ic, name, workdir, out_dir):
    """run_clean_case writes clean_<name>.npz; it is made in workdir and moved."""
    pos, kw = CASES[name]
    make_golden.run_clean_case(ic, name, *pos, workdir=workdir, out_dir=workdir, **kw)
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
