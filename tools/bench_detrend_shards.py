#!/usr/bin/env python
"""What detrending costs on channel shards, beside the undetrended shard loop.

One process, one GPU, a 360 x 3200 x 256 archive (bench.py's generator, on the
device), cleaned as --worlds in-process channel shards (one host thread each).
Three forms alternate --pairs times per world:

    plain     no detrending (ic_shard_enable_detrend is never called)
    detrend   orders (1, 2): shard_rowtrends, k_combine_dt_sh
    pieces    orders (1, 2), a piece every 16 channels of a subint's line
              (200 pieces): the piecewise kernels, k_combine_pw_sh

Each leg is one warm-up clean, then --runs cleans (ic_run, max_iter 5) with
every kernel timed by HIP events (ic_get_kernel_times) on every shard; the
figures are rank 0's, per iteration: the line stage (k_linestats: channel
lines, and the owner's row fits), the exchanges of the whole iteration
(`exchange`), the pack / assemble / unpack kernels (k_shard_pack) and k_combine.
In-process exchanges on one GPU are device copies: they say nothing about xGMI.
--forms plain runs the first form alone (it also runs on a tree without the
feature).  One JSON line per leg:

    python tools/bench_detrend_shards.py --out profiles/detrend_shards.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import threading
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPE = (360, 3200, 256)
SEED, RFI = 1, 0.05           # synth.CONFIGS["C2"]'s
ORDERS = (1, 2)
FORMS = {"plain": {}, "detrend": dict(shard_detrend=True, detrend=ORDERS),
         "pieces": dict(shard_detrend=True, detrend=ORDERS, detrend_pieces=(None, "w16"))}
IDS = ("k_linestats", "exchange", "k_shard_pack", "k_combine")


def leg(name, world, slices, runs, device, tag):
    from iterative_cleaner_amd import _native
    nsub, nchan, nbin = SHAPE
    out = [None] * world
    errors = []
    with _native.ShardGroup(world) as group:
        sess = []
        try:
            for r in range(world):
                sess.append(_native.ShardSession(nsub, nchan, nbin, r, world, group=group, device=device, max_iter=5,
                                                 **FORMS[name]))
                sess[r].upload_device(*(t.data_ptr() for t in slices[r]))

            def work(r):
                try:
                    s = sess[r]
                    s.run(fetch=False)
                    s.set_timing(True)
                    t0 = time.perf_counter()
                    n_iter = 0
                    for _ in range(runs):
                        n_iter = s.run(fetch=False)["n_iter"]
                    out[r] = (n_iter, (time.perf_counter() - t0) * 1e3 / runs, s.kernel_times())
                except Exception as e:  # noqa: BLE001 - reported below
                    errors.append(e)
            threads = [threading.Thread(target=work, args=(r,)) for r in range(world)]
            for t in threads:
                t.start()
            for t in threads:
                t.join()
        finally:
            for s in sess:
                s.close()
    if errors:
        raise errors[0]
    n_iter, wall, kt = out[0]
    rec = {"tree": tag, "form": name, "world": world, "shape": list(SHAPE), "n_iter": n_iter, "runs": runs,
           "wall_ms_per_clean": round(wall, 3)}
    for kid in IDS:
        rec[kid + "_ms_per_iteration"] = round(kt[kid]["ms"] / (runs * n_iter), 4)
        rec[kid + "_launches_per_iteration"] = round(kt[kid]["launches"] / (runs * n_iter), 2)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--worlds", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--forms", nargs="+", default=list(FORMS), choices=list(FORMS))
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--tag", default="head", help="recorded in every line (which tree ran)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import bench
    from iterative_cleaner_amd import _native
    dev = torch.device("cuda", a.device)
    cube, w0, shift = bench.make_cube_device(*SHAPE, SEED, RFI, dev)
    lines = []
    for world in a.worlds:
        chans, _ = _native.shard_layout(SHAPE[0], SHAPE[1], world)
        slices = [(cube[:, c0:c1].contiguous(), w0[:, c0:c1].contiguous(), shift[c0:c1].contiguous())
                  for c0, c1 in chans]
        torch.cuda.synchronize(dev)
        for _ in range(a.pairs):
            for name in a.forms:
                lines.append(json.dumps(leg(name, world, slices, a.runs, a.device, a.tag)))
                print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
