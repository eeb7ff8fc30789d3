#!/usr/bin/env python
"""8192-bin profiles against C5 (4096 bins) at the same sample count.

Times, in one process on one GPU, whole cleans (ic_run, max_iter 5, archive
resident in HBM, nothing fetched) of

    N8192  a synthetic 64 x 512 x 8192 archive (1 GiB as f32)
    C5     bench.py's 256 x 1024 x 4096 archive (the same 2^28 samples)

in the modes ``exact`` (integer shifts), ``fft_pp`` (exact fit, fractional
per-profile delays) and ``closed`` (closed-form fit, integer shifts).  The two
archives alternate --repeat times per mode; every timed window is --steps
cleans after --warmup, closed by a device synchronise.  One further clean per
archive and mode runs with every kernel timed (ic_get_kernel_times), outside
the timed windows.  One JSON line per window and per breakdown:

    python tools/bench_nbin8192.py --steps 5 --warmup 1 --repeat 3 --out profiles/nbin8192.jsonl

ns_per_sample_loop divides by the loops the clean ran, since the two archives
need not converge after the same number of loops.
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

SHAPES = {
    "N8192": (64, 512, 8192, 58, 0.30),
    "C5": bench.WORKLOADS["C5"],
}
MODES = ("exact", "fft_pp", "closed")     # the default legs
ALL_MODES = MODES + ("fft",)              # fft: exact fit, one fractional delay per channel


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=3, help="times the two archives alternate per mode")
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    modes, shapes = a.modes.split(","), a.shapes.split(",")
    if not set(modes) <= set(ALL_MODES) or not set(shapes) <= set(SHAPES):
        ap.error("--modes: %s; --shapes: %s" % (", ".join(ALL_MODES), ", ".join(SHAPES)))

    import torch

    from iterative_cleaner_amd import _native, synth
    if not torch.cuda.is_available():
        raise SystemExit("bench_nbin8192: no GPU")
    dev = torch.device("cuda", a.device)
    sink = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    for mode in modes:
        sessions = {}
        for name in shapes:
            nsub, nchan, nbin, seed, rfi = SHAPES[name]
            delay = None
            if mode == "fft_pp":
                delay = synth.per_profile_delays(np.arange(nchan) % 7, nbin, nsub)
            elif mode == "fft":
                delay = synth.fractional_delays(np.arange(nchan) % 7, nbin)
            cube, w0, shift = bench.make_cube_device(nsub, nchan, nbin, seed, rfi, dev)
            s = _native.GpuSession(nsub, nchan, nbin, max_iter=5, device=a.device, delay=delay,
                                   fit_mode=_native.FIT_CLOSED if mode == "closed" else _native.FIT_EXACT)
            torch.cuda.synchronize()
            s.upload_device(cube.data_ptr(), w0.data_ptr(), shift.data_ptr())
            del cube
            torch.cuda.empty_cache()
            for _ in range(a.warmup):
                s.run(fetch=False)
            sessions[name] = s
        for rep in range(a.repeat):
            for name in shapes:
                nsub, nchan, nbin = SHAPES[name][:3]
                s = sessions[name]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                loops = [s.run(fetch=False)["loops"] for _ in range(a.steps)]
                torch.cuda.synchronize()
                ms = 1000.0 * (time.perf_counter() - t0) / a.steps
                P = nsub * nchan
                emit({"shape_name": name, "shape": [nsub, nchan, nbin], "mode": mode, "repeat": rep, "steps": a.steps,
                      "warmup": a.warmup, "ms_per_clean": round(ms, 3), "profiles_per_s": round(P / ms * 1e3),
                      "loops": sorted(set(loops)),
                      "ns_per_sample_loop": round(ms * 1e6 / (P * nbin) / (sum(loops) / len(loops)), 5)})
        for name in shapes:       # the per-kernel breakdown, outside the timed windows
            s = sessions[name]
            s.set_timing(True)
            torch.cuda.synchronize()
            out = s.run(fetch=False)
            torch.cuda.synchronize()
            kt = {k: {"ms": round(v["ms"], 3), "launches": v["launches"]} for k, v in s.kernel_times().items()
                  if v["launches"]}
            emit({"shape_name": name, "mode": mode, "loops": out["loops"], "kernel_ms": kt})
            s.close()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
