#!/usr/bin/env python
"""C4 batch from page-locked host memory, f32 uploads against quantised uploads.

Mirrors bench.py's batch mode (same workload table entry, three archives
cycled, --batch archives per step on --lanes concurrent sessions, H2D copies
included in the time) and runs, in one process on one GPU, the legs

    f32        the synthetic cubes as ``bench.py --batch`` sends them
               (three-element items, ic_upload_async: 4 bytes per sample)
    quantised  the same archives PSRFITS-quantised (psrfits.quantise) as
               five-element items (ic_upload_quantised_async: 2 bytes per
               sample, decoded on the copy stream)
    decoded    the host decode of those samples sent as f32: exactly the cubes
               the quantised leg cleans, so the two differ in the upload alone

alternating --repeat times, and prints one JSON line per leg and repeat with
ms per archive and H2D bytes per archive.

    python tools/bench_quantised_batch.py --batch 16 --lanes 2 --steps 5 --warmup 1 --repeat 3

--upload times instead the synchronous uploads of ONE archive of the workload's
shape from pageable memory, as the CLI makes them: ic_upload of the f32 cube
against ic_upload_quantised of its int16 samples with nsum 1 and 2 (random
samples: only the copies and the decode are timed, nothing is cleaned).

    python tools/bench_quantised_batch.py --workload C2 --upload --repeat 3
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


def upload_main(a):
    from iterative_cleaner_amd import _native
    nsub, nchan, nbin = bench.WORKLOADS[a.workload][:3]
    rng = np.random.default_rng(0)
    q = rng.integers(-32767, 32768, size=(nsub, 2, nchan, nbin), dtype=np.int16)
    scl = rng.uniform(0.001, 0.01, size=(nsub, 2, nchan)).astype(np.float32)
    offs = rng.standard_normal((nsub, 2, nchan)).astype(np.float32)
    cube = q[:, 0].astype(np.float32)
    w0 = np.ones((nsub, nchan), np.float32)
    shift = np.zeros(nchan, np.int64)
    if a.big_endian:
        q = q.astype(">i2")
    q1 = np.ascontiguousarray(q[:, :1])
    legs = (("ic_upload", 4, lambda s: s.upload(cube, w0, shift)),
            ("ic_upload_quantised nsum 1", 2, lambda s: s.upload_quantised(q1, scl[:, :1], offs[:, :1], w0, shift, 1)),
            ("ic_upload_quantised nsum 2", 4, lambda s: s.upload_quantised(q, scl, offs, w0, shift, 2)))
    with _native.GpuSession(nsub, nchan, nbin, device=a.device) as s:
        for _, _, fn in legs:
            fn(s)                                   # staging allocated, pages touched
        for rep in range(a.repeat):
            for name, bps, fn in legs:
                t0 = time.perf_counter()
                fn(s)
                ms = 1000.0 * (time.perf_counter() - t0)
                print(json.dumps({"leg": name, "repeat": rep, "workload": a.workload, "shape": [nsub, nchan, nbin],
                                  "big_endian": bool(a.big_endian), "ms": round(ms, 2),
                                  "h2d_bytes": bps * nsub * nchan * nbin,
                                  "h2d_gbs": round(bps * nsub * nchan * nbin / ms / 1e6, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="C4", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--lanes", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=3, help="times the legs alternate")
    ap.add_argument("--legs", default="f32,quantised,decoded")
    ap.add_argument("--npol", type=int, default=1, help="polarisations of the quantised archives")
    ap.add_argument("--nsum", type=int, default=1, choices=(1, 2))
    ap.add_argument("--big-endian", action="store_true", help="samples in the FITS byte order ('>i2')")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--upload", action="store_true", help="time one archive's synchronous uploads instead")
    a = ap.parse_args()
    if a.upload:
        return upload_main(a)
    legs = a.legs.split(",")
    if not set(legs) <= {"f32", "quantised", "decoded"}:
        ap.error("--legs: f32, quantised, decoded")

    from iterative_cleaner_amd import _native, batch, psrfits, synth
    nsub, nchan, nbin, seed, rfi = bench.WORKLOADS[a.workload]
    P = nsub * nchan
    pinned = []

    def pin(arrays):
        out = []
        for arr in arrays:
            p = _native.PinnedArray(arr.shape, arr.dtype)
            p.array[...] = arr
            pinned.append(p)
            out.append(p.array)
        return tuple(out)

    items = {leg: [] for leg in legs}
    for k in range(3):
        data, w0, shift = synth.make_cube(nsub, nchan, nbin, seed + k, rfi, npol=a.npol)
        sh = shift.astype(np.int32)
        if "f32" in items:
            cube = data[:, 0] if a.nsum == 1 else (data[:, 0] + data[:, 1]).astype(np.float32)
            items["f32"].append(pin((np.ascontiguousarray(cube), w0, sh)))
        q, scl, offs = psrfits.quantise(data)
        if "decoded" in items:
            dec = psrfits.decode(q[:, :a.nsum], scl[:, :a.nsum], offs[:, :a.nsum])
            cube = dec[:, 0] if a.nsum == 1 else (dec[:, 0] + dec[:, 1]).astype(np.float32)
            items["decoded"].append(pin((np.ascontiguousarray(cube), w0, sh)))
        if "quantised" in items:
            items["quantised"].append(pin((q.astype(">i2") if a.big_endian else q, scl, offs, w0, sh)))
        del data, q
    h2d = {"f32": 4 * P * nbin + 4 * P + 4 * nchan, "decoded": 4 * P * nbin + 4 * P + 4 * nchan,
           "quantised": a.nsum * (2 * P * nbin + 8 * P) + 4 * P + 4 * nchan}

    sessions = [_native.GpuSession(nsub, nchan, nbin, max_iter=5, device=a.device) for _ in range(a.lanes)]
    streams = {leg: [items[leg][k % 3] for k in range(a.batch)] for leg in legs}
    for _ in range(a.warmup):
        for leg in legs:
            for _out in batch.run_lanes(sessions, streams[leg], fetch=False, nsum=a.nsum):
                pass
    for rep in range(a.repeat):
        for leg in legs:
            loops = []
            t0 = time.perf_counter()      # run() returns with its archive cleaned: nothing is left in flight
            for _ in range(a.steps):
                for out in batch.run_lanes(sessions, streams[leg], fetch=False, nsum=a.nsum):
                    loops.append(out["loops"])
            elapsed = time.perf_counter() - t0
            n_arch = a.steps * a.batch
            print(json.dumps({
                "leg": leg, "repeat": rep, "workload": a.workload, "shape": [nsub, nchan, nbin],
                "batch": a.batch, "lanes": a.lanes, "steps": a.steps, "warmup": a.warmup,
                "npol": a.npol, "nsum": a.nsum, "big_endian": bool(a.big_endian and leg == "quantised"),
                "ms_per_archive": round(1000.0 * elapsed / n_arch, 3),
                "h2d_bytes_per_archive": h2d[leg],
                "h2d_gbs": round(h2d[leg] * n_arch / elapsed / 1e9, 1),
                "archives_per_s": round(n_arch / elapsed, 2), "loops": sorted(set(loops))}), flush=True)
    for sess in sessions:
        sess.close()
    for p in pinned:
        p.close()


if __name__ == "__main__":
    main()
