#!/usr/bin/env python
"""C4 batch with fractional delays (FFT dedispersion), every archive with its own.

Mirrors bench.py's batch mode (same workload table entry, three archives
cycled, --batch archives per step on --lanes concurrent sessions, from
page-locked host memory, H2D copies included in the time).  The delays are
synth.fractional_delays of the archive's shifts, moved a little from archive to
archive.  In one process on one GPU the legs

    set_delays   the upload_async pipeline with a synchronous set_delays
                 (ic_set_delays) before each run: the only way before delays
                 could travel with an upload
    attached     the same delays attached to the upload (ic_upload_delays_async,
                 per channel): copied, and the phasor table built, on the copy
                 stream behind the archive's copy
    attached_pp  per-profile delays attached (the channel row scaled by
                 1 + 1e-6 s in subint s): no table, the rotation evaluates the
                 phasors per profile

alternate --repeat times; one JSON line per leg and repeat, ms per archive.

    python tools/bench_fft_batch.py --batch 16 --lanes 2 --steps 5 --warmup 1 --repeat 3
"""
from __future__ import annotations

import argparse
import collections
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402

LEGS = ("set_delays", "attached", "attached_pp")


class SetDelaysSession:
    """A session as batch.run_lanes drives it, with an item's delays set by a
    synchronous set_delays before the run that cleans it."""

    def __init__(self, session):
        self.session = session
        self.delays = collections.deque()

    def upload_async(self, cube, w0, shift, delay):
        self.delays.append(delay)
        self.session.upload_async(cube, w0, shift)

    def run(self, fetch=True):
        self.session.set_delays(self.delays.popleft())
        return self.session.run(fetch)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="C4", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--lanes", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=3, help="times the legs alternate")
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    legs = a.legs.split(",")
    if not set(legs) <= set(LEGS):
        ap.error("--legs: " + ", ".join(LEGS))

    from iterative_cleaner_amd import _native, batch, synth
    nsub, nchan, nbin, seed, rfi = bench.WORKLOADS[a.workload]
    pinned = []

    def pin(arrays):
        out = []
        for arr in arrays:
            p = _native.PinnedArray(arr.shape, arr.dtype)
            p.array[...] = arr
            pinned.append(p)
            out.append(p.array)
        return tuple(out)

    per_channel, per_profile = [], []
    for k in range(3):
        data, w0, shift = synth.make_cube(nsub, nchan, nbin, seed + k, rfi)
        d = synth.fractional_delays(shift, nbin) + 0.01 * k
        d2 = d[None, :] * (1.0 + 1e-6 * np.arange(nsub))[:, None]
        cube, w0, zero = pin((np.ascontiguousarray(data[:, 0]), w0, np.zeros(nchan, np.int32)))
        per_channel.append((cube, w0, zero) + pin((d,)))
        per_profile.append((cube, w0, zero) + pin((np.ascontiguousarray(d2),)))
        del data

    sessions = [_native.GpuSession(nsub, nchan, nbin, max_iter=5, device=a.device, dedisp_fft=True)
                for _ in range(a.lanes)]
    drivers = {"set_delays": [SetDelaysSession(s) for s in sessions], "attached": sessions, "attached_pp": sessions}
    streams = {"set_delays": [per_channel[k % 3] for k in range(a.batch)],
               "attached": [per_channel[k % 3] for k in range(a.batch)],
               "attached_pp": [per_profile[k % 3] for k in range(a.batch)]}
    for _ in range(a.warmup):
        for leg in legs:
            for _out in batch.run_lanes(drivers[leg], streams[leg], fetch=False):
                pass
    for rep in range(a.repeat):
        for leg in legs:
            loops = []
            t0 = time.perf_counter()      # run() returns with its archive cleaned: nothing is left in flight
            for _ in range(a.steps):
                for out in batch.run_lanes(drivers[leg], streams[leg], fetch=False):
                    loops.append(out["loops"])
            elapsed = time.perf_counter() - t0
            n_arch = a.steps * a.batch
            print(json.dumps({
                "leg": leg, "repeat": rep, "workload": a.workload, "shape": [nsub, nchan, nbin],
                "batch": a.batch, "lanes": a.lanes, "steps": a.steps, "warmup": a.warmup,
                "ms_per_archive": round(1000.0 * elapsed / n_arch, 3),
                "archives_per_s": round(n_arch / elapsed, 2), "loops": sorted(set(loops))}), flush=True)
    for sess in sessions:
        sess.close()
    for p in pinned:
        p.close()


if __name__ == "__main__":
    main()
