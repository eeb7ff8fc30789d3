#!/usr/bin/env python
"""C4 batch with residuals: what the encoded residual of every archive costs.

Quantised page-locked items (three archives cycled, --batch archives per step,
as tools/bench_quantised_batch.py makes them), and in one process on one GPU
the legs, alternating --repeat times:

    sync            the loop possible without batch residuals, one session:
                    upload_quantised_async of the next archive, run(), then the
                    synchronous residual_quantised(big_endian=True) into fresh
                    pageable arrays
    serial          the same loop with the download into page-locked arrays
                    (residual_quantised_async + residual_wait at once): the
                    copy at full rate, but nothing overlaps it
    lanesN+res      batch.run_lanes(residuals=...) on N sessions: the scheduler
                    clean_batch(residuals=True) drives, fed from page-locked
                    items, residuals into page-locked slots (3 per lane, 2 for
                    one lane)
    lanesN          the same without residuals
    batchN+res      clean_batch(residuals=True) itself, N lanes: adds its
    batchN          loader thread's host copy of every item into the ring, and
                    per call the sessions and the page-locked rings it makes

and prints one JSON line per leg and repeat with ms per archive; --out appends
them to a file.

    python tools/bench_residual_batch.py --batch 16 --steps 3 --repeat 3 --out profiles/residual_batch_c4.jsonl
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
    ap.add_argument("--workload", default="C4", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--lanes", default="1,2,4", help="lane counts of the lanes / batch legs")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=3, help="times the legs alternate")
    ap.add_argument("--legs", default="sync,serial,lanes+res,lanes,batch+res,batch")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    kinds = a.legs.split(",")
    if not set(kinds) <= {"sync", "serial", "lanes+res", "lanes", "batch+res", "batch"}:
        ap.error("--legs: sync, serial, lanes+res, lanes, batch+res, batch")
    lane_counts = [int(x) for x in a.lanes.split(",")]

    from iterative_cleaner_amd import _native, batch, psrfits, synth
    nsub, nchan, nbin, seed, rfi = bench.WORKLOADS[a.workload]
    shape = (nsub, nchan, nbin)
    pinned = []

    def pin_like(shp, dtype):
        p = _native.PinnedArray(shp, dtype)
        pinned.append(p)
        return p.array

    def pin(arrays):
        out = []
        for arr in arrays:
            dst = pin_like(arr.shape, arr.dtype)
            dst[...] = arr
            out.append(dst)
        return tuple(out)

    def result_slots(n):
        return [(pin_like(shape, ">i2"), pin_like((nsub, nchan), np.float32), pin_like((nsub, nchan), np.float32))
                for _ in range(n)]

    archives = []
    for k in range(3):
        data, w0, shift = synth.make_cube(nsub, nchan, nbin, seed + k, rfi)
        q, scl, offs = psrfits.quantise(data)
        archives.append(pin((q.astype(">i2"), scl, offs, w0, shift.astype(np.int32))))
        del data, q
    stream = [archives[k % 3] for k in range(a.batch * a.steps)]   # a leg is one pass over --steps batches
    nmax = max(lane_counts)
    sessions = [_native.GpuSession(*shape, max_iter=5, device=a.device) for _ in range(nmax)]
    slots = [result_slots(3) for _ in range(nmax)]
    seen = []   # a checksum per leg, so every leg is seen to move the residual it claims

    def loop(serial):
        """One session, upload of the next archive queued before run()."""
        s = sessions[0]
        s.upload_quantised_async(*stream[0], 1)
        for k in range(len(stream)):
            if k + 1 < len(stream):
                s.upload_quantised_async(*stream[k + 1], 1)
            s.run(False)
            if serial:
                s.residual_quantised_async(*slots[0][k % 2])
                s.residual_wait()
                seen.append(float(slots[0][k % 2][1][0, 0]))
            else:
                seen.append(float(s.residual_quantised(big_endian=True)[1][0, 0]))

    def lanes(n, res):
        r = ([slots[q][:2 if n == 1 else 3] for q in range(n)]) if res else None
        for out in batch.run_lanes(sessions[:n], stream, fetch=False, nsum=1, residuals=r):
            if res:
                seen.append(float(out["residual_q"][1][0, 0]))

    def whole(n, res):
        for out in batch.clean_batch(iter(stream), shape, device=a.device, lanes=n, quantised=True, nsum=1,
                                     residuals=res):
            if res:
                seen.append(float(out["residual_q"][1][0, 0]))

    legs = []
    for kind in kinds:
        if kind == "sync":
            legs.append(("sync", 1, True, lambda: loop(False)))
        elif kind == "serial":
            legs.append(("serial", 1, True, lambda: loop(True)))
        else:
            for n in lane_counts:
                res = kind.endswith("+res")
                fn = lanes if kind.startswith("lanes") else whole
                name = "%s%d%s" % ("lanes" if fn is lanes else "batch", n, "+res" if res else "")
                legs.append((name, n, res, lambda fn=fn, n=n, res=res: fn(n, res)))

    for _ in range(a.warmup):
        for _, _, _, fn in legs:
            fn()
    lines = []
    for rep in range(a.repeat):
        for name, n, res, fn in legs:
            del seen[:]
            t0 = time.perf_counter()      # every leg returns with its last residual on the host
            fn()
            elapsed = time.perf_counter() - t0
            n_arch = a.steps * a.batch
            line = json.dumps({
                "leg": name, "repeat": rep, "workload": a.workload, "shape": list(shape), "batch": a.batch,
                "lanes": n, "steps": a.steps, "warmup": a.warmup, "residuals": bool(res),
                "ms_per_archive": round(1000.0 * elapsed / n_arch, 3),
                "d2h_bytes_per_archive": (2 * nsub * nchan * nbin + 8 * nsub * nchan) if res else 0,
                "archives_per_s": round(n_arch / elapsed, 2), "scl_sum": round(sum(seen), 6)})
            print(line, flush=True)
            lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")
    for sess in sessions:
        sess.close()
    for p in pinned:
        p.close()


if __name__ == "__main__":
    main()
