#!/usr/bin/env python
"""Hot-bin repair: what the pass costs on a full-size archive.

A C2-shaped archive (default 360 x 3200 x 1024), resident in HBM as bench.py
makes it, with three +-30 spikes in the off-pulse bins of about 0.1 % of its
profiles.  The cube is uploaded from device memory --runs times to one session
with hot bins set, so that every run starts with the pass; k_hotbins and
k_hotbin_scan are timed by the dispatch packets' timestamps
(ic_get_kernel_times).  Reports, per run and as the median, the milliseconds of
k_hotbins, the cube bytes it covers per second (the whole cube: nsub x nchan x
nbin x 4 bytes) and the bytes it actually reads per second (the off-pulse
samples), next to the copy rate of the same cube on the same device
(device-to-device hipMemcpy: a read and a write of every byte) for comparison.
Prints one JSON line per record; --out appends them to a file.

    python tools/bench_hotbins.py --runs 5 --out profiles/hotbins_c2.jsonl
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
    ap.add_argument("--shape", default="360,3200,1024")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--fraction", type=float, default=0.001, help="fraction of the profiles that get spikes")
    ap.add_argument("--threshold", type=float, default=5.0)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()

    import torch

    from iterative_cleaner_amd import _native
    dev = torch.device("cuda", a.device)
    nsub, nchan, nbin = (int(x) for x in a.shape.split(","))
    P = nsub * nchan
    cube, w0, shift = bench.make_cube_device(nsub, nchan, nbin, a.seed, 0.05, dev)
    # the pulse sits at phase 0.3 with sigma 0.02, delayed by up to 6 bins: the
    # window covers +-4 sigma and the delays
    on_start, on_end = int(0.22 * nbin), int(0.38 * nbin) + 7
    rng = np.random.default_rng(a.seed)
    nhit = max(1, int(round(a.fraction * P)))
    prof = np.sort(rng.choice(P, size=nhit, replace=False))
    off = np.concatenate([np.arange(0, on_start - 7), np.arange(on_end + 7, nbin)])
    bins = np.stack([rng.choice(off, size=3, replace=False) for _ in range(nhit)])
    flat = torch.from_numpy((prof[:, None].astype(np.int64) * nbin + bins).reshape(-1)).to(dev)
    sign = torch.from_numpy(rng.choice([-30.0, 30.0], size=flat.shape[0]).astype(np.float32)).to(dev)
    cube.view(-1).index_add_(0, flat, sign)
    torch.cuda.synchronize()
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    cube_bytes = 4 * P * nbin
    read_bytes = 4 * P * (nbin - (on_end - on_start))
    # the comparison: a device-to-device copy of the cube
    scratch = torch.empty_like(cube)
    scratch.copy_(cube)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        scratch.copy_(cube)
    torch.cuda.synchronize()
    copy_ms = 1e3 * (time.perf_counter() - t0) / 3
    del scratch
    torch.cuda.empty_cache()
    emit({"leg": "d2d_copy", "shape": [nsub, nchan, nbin], "ms": round(copy_ms, 3),
          "cube_GB_per_s": round(cube_bytes / copy_ms / 1e6, 1),
          "note": "reads and writes every byte: traffic is twice the cube"})

    ms = []
    with _native.GpuSession(nsub, nchan, nbin, max_iter=1, device=a.device, fit_mode=_native.FIT_CLOSED,
                            hotbins=(a.threshold, on_start, on_end, a.rounds)) as s:
        for run in range(a.runs + 1):
            s.upload_device(cube.data_ptr(), w0.data_ptr(), shift.data_ptr())
            s.set_timing(True)      # clears the totals: one run's worth
            out = s.run(fetch=False)
            kt = s.kernel_times()
            if run == 0:
                continue            # warm-up
            k, sc = kt["k_hotbins"], kt["k_hotbin_scan"]
            assert k["launches"] == 1 and sc["launches"] == 1
            ms.append(k["ms"])
            hot = out["hotbins"]
            emit({"leg": "k_hotbins", "run": run, "shape": [nsub, nchan, nbin], "ms": round(k["ms"], 4),
                  "scan_ms": round(sc["ms"], 4), "cube_GB_per_s": round(cube_bytes / k["ms"] / 1e6, 1),
                  "read_GB_per_s": round(read_bytes / k["ms"] / 1e6, 1), "spiked_profiles": int(nhit),
                  "repaired_profiles": int((hot["count"] > 0).sum()), "capped_profiles": int((hot["count"] < 0).sum()),
                  "repaired_bins": int(hot["total"]), "threshold": a.threshold, "rounds": a.rounds,
                  "window": [on_start, on_end]})
    med = float(np.median(ms))
    emit({"leg": "summary", "shape": [nsub, nchan, nbin], "runs": a.runs, "k_hotbins_ms_median": round(med, 4),
          "k_hotbins_ms_min": round(min(ms), 4), "k_hotbins_ms_max": round(max(ms), 4),
          "cube_GB_per_s": round(cube_bytes / med / 1e6, 1), "read_GB_per_s": round(read_bytes / med / 1e6, 1),
          "d2d_copy_cube_GB_per_s": round(cube_bytes / copy_ms / 1e6, 1)})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
