#!/usr/bin/env python
"""The -u residual of one archive on its way to a PSRFITS file, the f32 download
against the quantised download.

Cleans one synthetic archive of the workload's shape (bench.py's table entry,
generated in HBM as bench.py generates it) and then runs, in one process on one
GPU, the legs

    f32        s.residual() - the f32 cube into pageable memory, 4 bytes per
               sample - followed by psrfits.quantise on the host: what a writer
               of that cube as PSRFITS has to do
    quantised  s.residual_quantised(big_endian=True): the same int16 samples,
               scales and offsets encoded on the GPU, 2 bytes per sample, in
               the FITS byte order

alternating --repeat times after one untimed round (staging allocated, pages
touched), and prints one JSON line per leg and repeat: the time on the GPU and
the bus (``gpu_copy_ms``: residual kernel [+ encode] + copy), the host's share
(``host_ms``: quantise; the quantised leg has none) and their sum.  The first
round also checks that the two legs give the same bytes.

    python tools/bench_residual_encode.py --workload C4 --repeat 3
    python tools/bench_residual_encode.py --workload C2 --repeat 2

A workload whose host quantise would not fit the free memory (about 38 bytes
per sample: the two f32 cubes and quantise's f64 temporaries) is reported as
skipped, unless --force.
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

HOST_BYTES_PER_SAMPLE = 38     # residual f32 + four f64 temporaries of quantise + int16


def mem_available() -> int:
    try:
        with open("/proc/meminfo") as fh:
            for line in fh:
                if line.startswith("MemAvailable:"):
                    return int(line.split()[1]) * 1024
    except OSError:
        pass
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="C4", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--repeat", type=int, default=3, help="times the legs alternate")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--force", action="store_true", help="run whatever the free host memory")
    a = ap.parse_args()

    nsub, nchan, nbin, seed, rfi = bench.WORKLOADS[a.workload]
    n = nsub * nchan * nbin
    base = {"workload": a.workload, "shape": [nsub, nchan, nbin]}
    need, have = HOST_BYTES_PER_SAMPLE * n, mem_available()
    if have and need > have and not a.force:
        print(json.dumps(dict(base, skipped="host quantise needs about %.1f GB, %.1f GB available"
                              % (need / 1e9, have / 1e9))), flush=True)
        return

    import torch

    from iterative_cleaner_amd import _native, psrfits
    dev = torch.device("cuda", a.device)
    _native.load_library()
    cube, w0, shift = bench.make_cube_device(nsub, nchan, nbin, seed, rfi, dev)
    torch.cuda.synchronize()
    with _native.GpuSession(nsub, nchan, nbin, max_iter=5, device=a.device) as s:
        s.upload_device(cube.data_ptr(), w0.data_ptr(), shift.data_ptr())
        out = s.run(fetch=False)
        del cube
        torch.cuda.empty_cache()

        def leg_f32():
            t0 = time.perf_counter()
            r = s.residual()
            t1 = time.perf_counter()
            q = psrfits.quantise(r[:, None])
            t2 = time.perf_counter()
            return q, 1000.0 * (t1 - t0), 1000.0 * (t2 - t1), 4 * n

        def leg_quantised():
            t0 = time.perf_counter()
            q = s.residual_quantised(big_endian=True)
            t1 = time.perf_counter()
            return q, 1000.0 * (t1 - t0), 0.0, 2 * n + 8 * nsub * nchan

        legs = (("f32", leg_f32), ("quantised", leg_quantised))
        first = {name: fn()[0] for name, fn in legs}
        same = (first["quantised"][0].tobytes() == first["f32"][0].astype(">i2").tobytes()
                and all(np.array_equal(x, y[:, 0], equal_nan=True)
                        for x, y in zip(first["quantised"][1:], first["f32"][1:])))
        del first
        for rep in range(a.repeat):
            for name, fn in legs:
                q, gpu_ms, host_ms, d2h = fn()
                del q
                print(json.dumps(dict(base, leg=name, repeat=rep, loops=out["loops"],
                                      gpu_copy_ms=round(gpu_ms, 2), host_ms=round(host_ms, 2),
                                      total_ms=round(gpu_ms + host_ms, 2), d2h_bytes=d2h,
                                      d2h_gbs=round(d2h / gpu_ms / 1e6, 2), same_bytes=bool(same))), flush=True)


if __name__ == "__main__":
    main()
