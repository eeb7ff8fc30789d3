#!/usr/bin/env python
"""Time per clean at profile lengths that are neither a power of two nor mixed-radix.

Times, in one process on one GPU, whole cleans (ic_run, max_iter 5, exact fit,
archive resident in HBM, nothing fetched) of one synthetic archive of --shape
NSUBxNCHAN profiles (default 360x3200, C2's profile count) and --nbin bins
(default 500; a comma-separated list runs one after the other), in the modes
``int`` (integer shifts; on request) and, in IC_DEDISP_FFT_ANY, ``fft`` (one
fractional delay per channel) and ``fft_pp`` (per-profile delays).  Every timed window is
--steps cleans after --warmup, closed by a device synchronise, --repeat windows
per mode.  One further clean per mode runs with every kernel timed
(ic_get_kernel_times), outside the timed windows; its line carries
k_rotate's share of the kernels' summed time (at these lengths every k_rotate
launch is k_rotate_czt, or the identity for an archive stored dedispersed).
One JSON line per window and per breakdown:

    python tools/bench_any.py --steps 2 --warmup 1 --repeat 3 --out profiles/czt_clean_360x3200x500.jsonl

Two trees are compared by running this file of one tree against either
library (IC_LIBRARY names the other tree's libicgpu.so), --tag saying which ran,
the runs alternating.  --diag-fork 0 times the unforked schedule, in which
every k_diag launch measures every profile: the per-launch figure
(k_diag_ms_per_launch) then compares the statistics kernels themselves.

The archive is tools/bench_mr.py's (noise, a dispersed pulse, narrow-band and
impulsive RFI, dead channels); it is not one of bench.py's workloads.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

MODES = ("fft", "fft_pp")          # the default legs
ALL_MODES = ("int",) + MODES


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--shape", default="360x3200", help="NSUBxNCHAN")
    ap.add_argument("--nbin", default="500", help="one length, or several separated by commas")
    ap.add_argument("--diag-fork", type=int, default=None, help="session option diag_fork (0: unforked)")
    ap.add_argument("--tag", default=None, help="copied into every line (which tree ran)")
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--rfi", type=float, default=0.05)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    modes = a.modes.split(",")
    if not set(modes) <= set(ALL_MODES):
        ap.error("--modes: %s" % ", ".join(ALL_MODES))
    try:
        nsub, nchan = (int(x) for x in a.shape.lower().split("x"))
    except ValueError:
        ap.error("--shape NSUBxNCHAN")
    try:
        nbins = [int(x) for x in a.nbin.split(",")]
    except ValueError:
        ap.error("--nbin N[,N...]")
    options = None if a.diag_fork is None else {"diag_fork": a.diag_fork}

    import torch
    from bench_mr import make_archive

    from iterative_cleaner_amd import _native, synth
    if not torch.cuda.is_available():
        raise SystemExit("bench_any: no GPU")
    dev = torch.device("cuda", a.device)
    sink = open(a.out, "a") if a.out else None

    def emit(rec):
        if a.tag:
            rec = dict(rec, tag=a.tag)
        if options:
            rec = dict(rec, options=options)
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    P = nsub * nchan
    for nbin, mode in ((n, m) for n in nbins for m in modes):
        if mode == "fft_pp":
            delay = synth.per_profile_delays(np.arange(nchan) % 7, nbin, nsub)
        elif mode == "fft":
            delay = synth.fractional_delays(np.arange(nchan) % 7, nbin)
        else:
            delay = None
        cube, w0, shift = make_archive(nsub, nchan, nbin, a.seed, a.rfi, dev)
        if delay is not None:
            shift.zero_()
        with _native.GpuSession(nsub, nchan, nbin, max_iter=5, device=a.device, delay=delay,
                                any_length=delay is not None, options=options) as s:
            torch.cuda.synchronize()
            s.upload_device(cube.data_ptr(), w0.data_ptr(), shift.data_ptr())
            del cube
            torch.cuda.empty_cache()
            for _ in range(a.warmup):
                s.run(fetch=False)
            for rep in range(a.repeat):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                loops = [s.run(fetch=False)["loops"] for _ in range(a.steps)]
                torch.cuda.synchronize()
                ms = 1000.0 * (time.perf_counter() - t0) / a.steps
                emit({"shape": [nsub, nchan, nbin], "mode": mode, "repeat": rep, "steps": a.steps,
                      "warmup": a.warmup, "ms_per_clean": round(ms, 3), "profiles_per_s": round(P / ms * 1e3),
                      "loops": sorted(set(loops))})
            s.set_timing(True)   # the per-kernel breakdown, outside the timed windows
            torch.cuda.synchronize()
            out = s.run(fetch=False)
            torch.cuda.synchronize()
            kt = {k: {"ms": round(v["ms"], 3), "launches": v["launches"]} for k, v in s.kernel_times().items()
                  if v["launches"]}
            total = sum(v["ms"] for v in kt.values())
            rec = {"shape": [nsub, nchan, nbin], "mode": mode, "loops": out["loops"], "n_iter": out["n_iter"],
                   "kernel_ms": kt, "kernel_ms_total": round(total, 3)}
            for k in ("k_rotate", "k_diag"):
                if k in kt and total > 0:
                    rec[k + "_share"] = round(kt[k]["ms"] / total, 4)
            if "k_diag" in kt:
                rec["k_diag_ms_per_launch"] = round(kt["k_diag"]["ms"] / kt["k_diag"]["launches"], 4)
            emit(rec)
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
