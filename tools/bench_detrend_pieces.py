#!/usr/bin/env python
"""What piecewise detrending costs in the line stage, beside the whole-line form.

One process, one GPU, bench.py's C2 archive (360 x 3200 x 1024, generated on the
device and resident in HBM).  Two sessions alternate --pairs times:

    unpieced  detrend (1, 2): k_linetrend + k_combine_dt
    pieces    detrend (1, 2), a piece every 16 channels of a subint's line
              (200 pieces): k_linetrend_pw + k_combine_pw

Each leg is one warm-up clean, then --runs cleans (ic_run, max_iter 5) with
every kernel timed by HIP events (ic_get_kernel_times); both kernel pairs are
timed under the ids k_linestats / k_combine.  One JSON line per leg:

    python tools/bench_detrend_pieces.py --out profiles/detrend_pieces_c2.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPE = (360, 3200, 1024)
SEED, RFI = 1, 0.05           # synth.CONFIGS["C2"]
ORDERS = (1, 2)
LEGS = {"unpieced": None, "pieces": (None, "w16")}


def leg(name, cube, w0, shift, runs, device):
    from iterative_cleaner_amd import _native
    with _native.GpuSession(*SHAPE, max_iter=5, device=device, detrend=ORDERS, detrend_pieces=LEGS[name]) as s:
        s.upload_device(cube.data_ptr(), w0.data_ptr(), shift.data_ptr())
        s.run(fetch=False)
        s.set_timing(True)
        n_iter = 0
        for _ in range(runs):
            n_iter = s.run(fetch=False)["n_iter"]
        kt = s.kernel_times()
    ls, cb = kt["k_linestats"], kt["k_combine"]
    npieces = 1 if LEGS[name] is None else len(range(0, SHAPE[1], 16))
    return {"mode": name, "shape": list(SHAPE), "orders": list(ORDERS), "subint_pieces": npieces, "n_iter": n_iter,
            "runs": runs,
            "line_ms_per_clean": round(ls["ms"] / runs, 4), "line_ms_per_iteration": round(ls["ms"] / ls["launches"], 4),
            "combine_ms_per_clean": round(cb["ms"] / runs, 4),
            "combine_ms_per_iteration": round(cb["ms"] / cb["launches"], 4),
            "line_stage_ms_per_clean": round((ls["ms"] + cb["ms"]) / runs, 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import bench
    dev = torch.device("cuda", a.device)
    cube, w0, shift = bench.make_cube_device(*SHAPE, SEED, RFI, dev)
    torch.cuda.synchronize(dev)
    lines = []
    for _ in range(a.pairs):
        for name in LEGS:
            rec = leg(name, cube, w0, shift, a.runs, a.device)
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
