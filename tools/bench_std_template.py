#!/usr/bin/env python
"""Standard template: what a clean against a supplied profile costs.

For each workload (default C2 and C5), resident in HBM as bench.py makes it, in
one process on one GPU the legs, alternating --repeat times:

    default     the iterative-template clean (max_iter 5), as bench.py times it
    std_none    the same session with std_template = that clean's own final
                template, align "none": one pass, no alignment
    std_frac    the same with align "frac" (cross-correlation, peak, one-profile
                rotation, install): one pass

and, on a small session at 1024 and 8192 bins, the time of the two alignment
kernels alone (k_std_ccf + k_std_peak, from the dispatch packets' timestamps).
Prints one JSON line per leg and repeat; --out appends them to a file.

    python tools/bench_std_template.py --steps 5 --repeat 3 --out profiles/std_template_c2.jsonl
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

import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="C2,C5")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=3, help="times the legs alternate")
    ap.add_argument("--align-nbins", default="1024,8192", help="lengths of the alignment-kernel timing")
    ap.add_argument("--align-runs", type=int, default=20)
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

    for wl in [w for w in a.workloads.split(",") if w]:
        nsub, nchan, nbin, seed, rfi = bench.WORKLOADS[wl]
        cube, w0, shift = bench.make_cube_device(nsub, nchan, nbin, seed, rfi, dev)
        torch.cuda.synchronize()
        with _native.GpuSession(nsub, nchan, nbin, max_iter=5, device=a.device) as s:
            s.upload_device(cube.data_ptr(), w0.data_ptr(), shift.data_ptr())
            ref = s.run()
            T = s.template()

            def leg(mode):
                if mode is None:
                    s.clear_std_template()
                else:
                    s.set_std_template(T, mode)
                for _ in range(a.warmup):
                    s.run(fetch=False)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    out = s.run(fetch=False)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / a.steps
                full = s.run()
                return dt, out, full

            for rep in range(a.repeat):
                for name, mode in (("default", None), ("std_none", "none"), ("std_frac", "frac")):
                    dt, out, full = leg(mode)
                    emit({"leg": name, "repeat": rep, "workload": wl, "shape": [nsub, nchan, nbin],
                          "steps": a.steps, "warmup": a.warmup, "ms_per_clean": round(1e3 * dt, 3),
                          "loops": out["loops"], "n_iter": out["n_iter"],
                          "zapped": int((full["weights"] == 0).sum()),
                          "mask_differs_from_default": int((full["weights"] != ref["weights"]).sum()),
                          "alignment": full.get("std_alignment")})
        del cube, w0, shift
        torch.cuda.empty_cache()

    for nbin in [int(x) for x in a.align_nbins.split(",") if x]:
        data, w0, shift = synth.make_cube(4, 64, nbin, 3, 0.1)
        raw = np.ascontiguousarray(data[:, 0])
        with _native.GpuSession(4, 64, nbin, max_iter=1, device=a.device) as s:
            s.upload(raw, w0, shift)
            s.run(fetch=False)
            s.set_std_template(np.roll(s.template(), -5), "int")
            s.run(fetch=False)
            s.set_timing(True, only="k_std_align")
            for _ in range(a.align_runs):
                s.run(fetch=False)
            kt = s.kernel_times()["k_std_align"]
            emit({"leg": "align_kernels", "nbin": nbin, "runs": a.align_runs, "launches": kt["launches"],
                  "ms_per_alignment": round(kt["ms"] / a.align_runs, 5),
                  "note": "k_std_ccf + k_std_peak, dispatch-packet timestamps"})

    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
