#!/usr/bin/env python
"""1000-bin profiles against 1024-bin ones at the same archive shape.

Times, in one process on one GPU, whole cleans (ic_run, max_iter 5, archive
resident in HBM, nothing fetched) of two synthetic archives of --shape
NSUBxNCHAN profiles (default 360x3200, C2's profile count):

    MR1000  nbin 1000 (mixed radix: k_diag_mr, k_rotate_mr)
    P1024   nbin 1024 (the power-of-two kernels)

in the modes ``exact`` (integer shifts), ``fft`` (exact fit, one fractional
delay per channel) and ``fft_pp`` (per-profile delays); ``fft_rs0`` is ``fft``
with the option rot_stats = 0, so that both lengths measure the rotated
residual in a DIAG_STATS pass of k_diag.  The two archives alternate --repeat
times per mode; every timed window is --steps cleans after --warmup, closed by
a device synchronise.  One further clean per archive and mode runs with every
kernel timed (ic_get_kernel_times), outside the timed windows.  One JSON line
per window and per breakdown:

    python tools/bench_mr.py --steps 3 --warmup 1 --repeat 3 --out profiles/diag_mr.jsonl

The archives are generated here (noise, a dispersed pulse, narrow-band and
impulsive RFI, dead channels); they are not bench.py's workloads.
kdiag_ns_per_sample of a breakdown line is k_diag's time per iteration over
the archive's samples (an iteration's launches, forked or not, measure every
profile once): the figure the two lengths are compared by.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

NBINS = {"MR1000": 1000, "P1024": 1024}
MODES = ("exact", "fft", "fft_pp")       # the default legs
ALL_MODES = MODES + ("fft_rs0",)


def make_archive(nsub, nchan, nbin, seed, rfi, device):
    """(cube f32 [nsub][nchan][nbin], w0 f32, shift i32) in HBM."""
    import torch
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    f32, f64 = torch.float32, torch.float64
    phase = (torch.arange(nbin, device=device, dtype=f64) + 0.5) / nbin
    pulse = torch.exp(-0.5 * ((phase - 0.3) / 0.02) ** 2)
    shift = (torch.arange(nchan, device=device) % 7).to(torch.int32)
    idx = (torch.arange(nbin, device=device)[None, :] - shift[:, None].long()) % nbin
    pulse_disp = pulse[idx].to(f32)
    gain = (0.5 + torch.rand((nsub, nchan), generator=g, device=device, dtype=f64)).to(f32)
    cube = torch.randn((nsub, nchan, nbin), generator=g, device=device, dtype=f32)
    for s0 in range(0, nsub, 32):
        cube[s0:s0 + 32] += gain[s0:s0 + 32, :, None] * pulse_disp[None]
    n_nb = int(round(rfi * nchan))
    if n_nb:
        chans = torch.randperm(nchan, generator=g, device=device)[:n_nb]
        nu = 1.0 + 19.0 * torch.rand(n_nb, generator=g, device=device, dtype=f64)
        amp = 5.0 * torch.randn((nsub, n_nb), generator=g, device=device, dtype=f64)
        wave = torch.sin(2.0 * math.pi * nu[:, None] * phase[None, :])
        cube[:, chans, :] += (amp[:, :, None] * wave[None]).to(f32)
    for s in torch.randperm(nsub, generator=g, device=device)[:int(round(rfi * nsub))].tolist():
        cube[s] += (torch.rand((nchan, nbin), generator=g, device=device) < 0.01).to(f32) * 20.0
    w0 = torch.ones((nsub, nchan), device=device, dtype=f32)
    n_dead = int(round(0.02 * nchan))
    if n_dead:
        w0[:, torch.randperm(nchan, generator=g, device=device)[:n_dead]] = 0.0
    return cube.contiguous(), w0.contiguous(), shift.contiguous()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=3, help="times the two archives alternate per mode")
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--shape", default="360x3200", help="NSUBxNCHAN of both archives")
    ap.add_argument("--archives", default=",".join(NBINS), help="a subset of %s (a profiler run of one length)" % ",".join(NBINS))
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--rfi", type=float, default=0.05)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--tag", default=None, help="copied into every line (which tree ran)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    modes = a.modes.split(",")
    if not set(modes) <= set(ALL_MODES):
        ap.error("--modes: %s" % ", ".join(ALL_MODES))
    if not set(a.archives.split(",")) <= set(NBINS):
        ap.error("--archives: %s" % ", ".join(NBINS))
    nbins = {k: v for k, v in NBINS.items() if k in a.archives.split(",")}
    try:
        nsub, nchan = (int(x) for x in a.shape.lower().split("x"))
    except ValueError:
        ap.error("--shape NSUBxNCHAN")

    import torch

    from iterative_cleaner_amd import _native, synth
    if not torch.cuda.is_available():
        raise SystemExit("bench_mr: no GPU")
    dev = torch.device("cuda", a.device)
    sink = open(a.out, "a") if a.out else None

    def emit(rec):
        if a.tag:
            rec = dict(tag=a.tag, **rec)
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    P = nsub * nchan
    for mode in modes:
        sessions = {}
        for name, nbin in nbins.items():
            delay = None
            if mode == "fft_pp":
                delay = synth.per_profile_delays(np.arange(nchan) % 7, nbin, nsub)
            elif mode in ("fft", "fft_rs0"):
                delay = synth.fractional_delays(np.arange(nchan) % 7, nbin)
            cube, w0, shift = make_archive(nsub, nchan, nbin, a.seed, a.rfi, dev)
            if delay is not None:
                shift.zero_()
            s = _native.GpuSession(nsub, nchan, nbin, max_iter=5, device=a.device, delay=delay,
                                   options={"rot_stats": 0} if mode == "fft_rs0" else None)
            torch.cuda.synchronize()
            s.upload_device(cube.data_ptr(), w0.data_ptr(), shift.data_ptr())
            del cube
            torch.cuda.empty_cache()
            for _ in range(a.warmup):
                s.run(fetch=False)
            sessions[name] = s
        for rep in range(a.repeat):
            for name, nbin in nbins.items():
                s = sessions[name]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                loops = [s.run(fetch=False)["loops"] for _ in range(a.steps)]
                torch.cuda.synchronize()
                ms = 1000.0 * (time.perf_counter() - t0) / a.steps
                emit({"shape_name": name, "shape": [nsub, nchan, nbin], "mode": mode, "repeat": rep, "steps": a.steps,
                      "warmup": a.warmup, "ms_per_clean": round(ms, 3), "profiles_per_s": round(P / ms * 1e3),
                      "loops": sorted(set(loops)),
                      "ns_per_sample_loop": round(ms * 1e6 / (P * nbin) / (sum(loops) / len(loops)), 5)})
        for name, nbin in nbins.items():   # the per-kernel breakdown, outside the timed windows
            s = sessions[name]
            s.set_timing(True)
            torch.cuda.synchronize()
            out = s.run(fetch=False)
            torch.cuda.synchronize()
            kt = {k: {"ms": round(v["ms"], 3), "launches": v["launches"]} for k, v in s.kernel_times().items()
                  if v["launches"]}
            rec = {"shape_name": name, "shape": [nsub, nchan, nbin], "mode": mode, "loops": out["loops"],
                   "n_iter": out["n_iter"], "kernel_ms": kt}
            if "k_diag" in kt:
                rec["kdiag_ms_per_iter"] = round(kt["k_diag"]["ms"] / out["n_iter"], 4)
                rec["kdiag_ns_per_sample"] = round(kt["k_diag"]["ms"] * 1e6 / (out["n_iter"] * P * nbin), 6)
            emit(rec)
            s.close()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
