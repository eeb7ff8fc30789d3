#!/usr/bin/env python
"""Dynamic spectrum: what k_dynspec costs on a full-size archive.

A C2-shaped archive, resident in HBM as bench.py makes it, is cleaned once
(closed fit, one iteration: only the resident cube, template and weights
matter here) and GpuSession.dynspec() is then called --runs times with
k_dynspec alone timed by its dispatch packet's timestamps
(ic_get_kernel_times).  Legs: 360 x 3200 x 1024 with integer shifts (the
gather form), the same with fractional delays (the row-major rotated view) and
360 x 3200 x 4096 with integer shifts (the row of 64 samples per lane, the table
in LDS).  Reports the milliseconds per call, the cube bytes covered per second
(nsub x nchan x nbin x 4 over the time; zero-weight rows are skipped, so the
bytes read are fewer by their share) and the fraction of zero weights.  Prints
one JSON line per record; --out appends them to a file.

    python tools/bench_dynspec.py --runs 7 --out profiles/dynspec_c2.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402

LEGS = {"1024_shift": ((360, 3200, 1024), False), "1024_fft": ((360, 3200, 1024), True),
        "4096_shift": ((360, 3200, 4096), False)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--legs", default=",".join(LEGS), help="comma-separated: %s" % ", ".join(LEGS))
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()

    import torch

    from iterative_cleaner_amd import _native, synth
    dev = torch.device("cuda", a.device)
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    for leg in a.legs.split(","):
        (nsub, nchan, nbin), fft = LEGS[leg]
        cube, w0, shift = bench.make_cube_device(nsub, nchan, nbin, a.seed, 0.05, dev)
        delay = synth.fractional_delays(shift.cpu().numpy().astype(np.int64), nbin) if fft else None
        cube_bytes = 4 * nsub * nchan * nbin
        ms = []
        with _native.GpuSession(nsub, nchan, nbin, max_iter=1, device=a.device, fit_mode=_native.FIT_CLOSED,
                                delay=delay) as s:
            s.upload_device(cube.data_ptr(), w0.data_ptr(), shift.data_ptr())
            out = s.run()
            zero = float((out["weights"] == 0).mean())
            for run in range(a.runs + 1):
                s.set_timing(True, only="k_dynspec")      # clears the totals: one call's worth
                dyn = s.dynspec()
                k = s.kernel_times()["k_dynspec"]
                assert k["launches"] == 1
                if run == 0:
                    continue                              # warm-up (and the scratch's allocation)
                ms.append(k["ms"])
                emit({"leg": leg, "run": run, "shape": [nsub, nchan, nbin], "ms": round(k["ms"], 4),
                      "cube_GB_per_s": round(cube_bytes / k["ms"] / 1e6, 1)})
            live = out["weights"] != 0
            assert np.all(np.isfinite(dyn["amp"][live])) and np.all(dyn["amp"][~live] == 0)
        med = float(np.median(ms))
        emit({"leg": leg, "summary": True, "shape": [nsub, nchan, nbin], "fft_delays": fft, "runs": a.runs,
              "k_dynspec_ms_median": round(med, 4), "k_dynspec_ms_min": round(min(ms), 4),
              "k_dynspec_ms_max": round(max(ms), 4), "cube_GB_per_s": round(cube_bytes / med / 1e6, 1),
              "zero_weight_fraction": round(zero, 4)})
        del cube, w0, shift
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
