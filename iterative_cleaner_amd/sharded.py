"""Channel-sharded cleaning of one large archive (config C3).

The reference cleans an archive in one process (iterative_cleaner.py:83-146).
Here the same loop runs as ``world`` channel shards (shards.py), each a
libicgpu shard session; results are bit-identical to one unsharded session.

* ``clean_cube_local``: all shards in this process, one host thread each, on one
  or several devices (in-process group: device-to-device / peer copies).
* ``clean_cube_dist``: this rank's shard under torchrun, exchanging through
  torch.distributed (dist.TorchComm: RCCL over xGMI on "nccl"); the full test /
  weights arrays are all-gathered so every rank returns the same dict.
"""
from __future__ import annotations

import threading

import numpy as np

from . import _native


def _gather_cols(parts, ranges, shape, dtype):
    out = np.empty(shape, dtype)
    for (c0, c1), part in zip(ranges, parts):
        out[:, c0:c1] = part
    return out


# the keywords of **args: the session's (_loop_kwargs), `delay`, which the
# callers slice per rank themselves, and `dynspec`, which they act on after the run
_LOOP_KEYS = ("max_iter", "chanthresh", "subintthresh", "pulse_region", "baseline_duty", "fit_mode", "data_f64",
              "options", "input_dedispersed", "any_length", "detrend", "detrend_pieces", "shard_detrend",
              "std_template", "hotbins")


def _loop_kwargs(args, global_shape=None, nbin=None):
    """The ShardSession keywords of a clean_cube_* call's **args.  An unknown
    keyword is an error, not dropped.  detrend (detrend.normalise's forms) needs
    shard_detrend=True, the opt-in every rank must give (ic_shard_enable_detrend);
    detrend_pieces are resolved once against the global (nsub, nchan), so every
    rank gets the same starts.  std_template (std_template.normalise's forms
    but None, which is off: run_loop is where the IC_STD_TEMPLATE switch is
    read) is loaded and checked once per call, for the archive's nbin.
    hotbins (hotbins.normalise's forms but None, which is off: run_loop reads
    the IC_HOTBINS switch): the hot-bin repair, each rank on its own slice."""
    unknown = sorted(set(args) - set(_LOOP_KEYS) - {"delay", "dynspec"})
    if unknown:
        raise TypeError("unknown keyword(s) for a sharded clean: %s" % ", ".join(unknown))
    kw = dict(max_iter=args.get("max_iter", 5), chanthresh=args.get("chanthresh", 5.0),
              subintthresh=args.get("subintthresh", 5.0),
              pulse_region=args.get("pulse_region", (0, 0, 1)),
              baseline_duty=args.get("baseline_duty", 0.15), fit_mode=args.get("fit_mode", 0),
              data_f64=args.get("data_f64", False), options=args.get("options"),
              input_dedispersed=args.get("input_dedispersed", False), any_length=args.get("any_length"))
    if args.get("std_template") is not None:
        from .std_template import normalise as std_normalise
        kw["std_template"] = std_normalise(args["std_template"], int(nbin))
    if args.get("hotbins") is not None:
        from .hotbins import normalise as hot_normalise
        hot = hot_normalise(args["hotbins"])
        if hot is not None:
            kw["hotbins"] = hot
    shard_detrend = bool(args.get("shard_detrend", False))
    detrend, pieces = args.get("detrend"), args.get("detrend_pieces")
    if detrend is not None and not shard_detrend:
        raise ValueError("detrend on channel shards needs the opt-in shard_detrend=True on every rank "
                         "(ic_shard_enable_detrend)")
    if pieces is not None and detrend is None:
        raise ValueError("detrend_pieces needs detrend")
    if shard_detrend:
        kw["shard_detrend"] = True
    if detrend is not None:
        from .detrend import check_params, normalise_pieces
        detrend = check_params(*detrend)
        kw["detrend"] = detrend
        if pieces is not None:
            if global_shape is None:
                raise ValueError("detrend_pieces need the archive's global shape")
            pieces = normalise_pieces(pieces, global_shape[0], global_shape[1], detrend)
            if pieces is not None:
                kw["detrend_pieces"] = tuple(None if b is None else tuple(int(v) for v in b) for b in pieces)
    return kw


def clean_cube_local(cube, w0, shift, world, devices=None, want_details=False, fit_tail=None, **args):
    """Clean a (nsub, nchan, nbin) f32 cube as `world` in-process channel shards.
    Returns the ic_run dict with full-archive ``test`` / ``weights`` (and, with
    want_details, ``amp``, ``info``, ``std``, ``mean``, ``ptp``, ``fft``, ``T``).
    ``detrend`` / ``detrend_pieces`` (GpuSession's) with ``shard_detrend=True``:
    the detrended scaling on shards; want_details then adds ``trend_chan``
    (every shard's channel coefficients, joined along the channels) and
    ``trend_subint`` (all rows', checked equal across the shards).
    ``std_template`` (a profile, a path, or a pair with the align mode; None:
    off): the opt-in cleaning against a standard
    profile (std_template.py), the same on every shard; ``std_alignment`` is
    every shard's (checked equal).  ``hotbins`` = (threshold, on_start,
    on_end[, rounds]) (None: off): the opt-in hot-bin repair (hotbins.py);
    every shard repairs its own channels and ``hotbins`` is the whole
    archive's dict(count, total, offsets, bins).  ``dynspec=True``: ``dynspec``
    = dict(amp, err, base), the archive's dynamic spectrum (dynspec.py), every
    shard's slice joined in rank order."""
    nsub, nchan, nbin = cube.shape
    devices = list(devices) if devices is not None else [0] * world
    if len(devices) != world:
        raise ValueError("need one device per shard")
    chans, _ = _native.shard_layout(nsub, nchan, world)
    kw = _loop_kwargs(args, (nsub, nchan), nbin)
    delay = args.get("delay")
    results = [None] * world
    errors = []
    with _native.ShardGroup(world) as group:
        sessions = []
        try:
            for r in range(world):   # (inside the try: a shard that cannot be made closes the ones before it)
                sessions.append(_native.ShardSession(
                    nsub, nchan, nbin, r, world, group=group, device=devices[r],
                    delay=None if delay is None else np.asarray(delay)[..., chans[r][0]:chans[r][1]], **kw))
            for r, s in enumerate(sessions):
                c0, c1 = chans[r]
                if fit_tail is not None:
                    s.set_fit_tail(fit_tail)
                s.upload(cube[:, c0:c1], w0[:, c0:c1], np.asarray(shift)[c0:c1])

            def work(r):
                try:
                    s = sessions[r]
                    out = s.run()
                    if args.get("dynspec") and out["n_iter"] > 0:
                        out["dynspec"] = s.dynspec()
                    if want_details and out["n_iter"] > 0:
                        out["amp"], out["info"] = s.fit()
                        out["std"], out["mean"], out["ptp"], out["fft"] = s.diagnostics()
                        out["T"] = s.template()
                        if kw.get("detrend") is not None and any(kw["detrend"][:2]):
                            out["trend_chan"], out["trend_subint"] = s.trends()
                    results[r] = out
                except Exception as e:  # noqa: BLE001 - re-raised below
                    errors.append((r, e))

            threads = [threading.Thread(target=work, args=(r,)) for r in range(world)]
            for t in threads:
                t.start()
            for t in threads:
                t.join()
        finally:
            for s in sessions:
                s.close()
    if errors:
        r, e = errors[0]
        raise _native.NativeError("shard %d failed: %s" % (r, e))
    return _merge(results, chans, (nsub, nchan), want_details)


def _merge(results, chans, shape2, want_details):
    first = results[0]
    for r, out in enumerate(results[1:], 1):
        for key in ("loops", "n_iter", "converged"):
            if out[key] != first[key]:
                raise _native.NativeError("shard %d disagrees on %s" % (r, key))
        if not (np.array_equal(out["changed"], first["changed"])
                and np.array_equal(out["nzero"], first["nzero"])):
            raise _native.NativeError("shard %d disagrees on the convergence counters" % r)
        if out.get("std_alignment") != first.get("std_alignment"):
            raise _native.NativeError("shard %d aligned the standard template differently" % r)
    merged = dict(first)
    merged["test"] = _gather_cols([o["test"] for o in results], chans, shape2, np.float64)
    merged["weights"] = _gather_cols([o["weights"] for o in results], chans, shape2, np.float32)
    if "hotbins" in first:
        from .hotbins import merge_shards
        merged["hotbins"] = merge_shards([o["hotbins"] for o in results])
    if "dynspec" in first:
        from .dynspec import merge_shards as merge_dynspec
        merged["dynspec"] = merge_dynspec([o["dynspec"] for o in results])
    if want_details and "amp" in first:
        for key, dt in (("amp", np.float64), ("info", np.int32), ("std", np.float64),
                        ("mean", np.float64), ("ptp", first["ptp"].dtype), ("fft", np.float64)):
            merged[key] = _gather_cols([o[key] for o in results], chans, shape2, dt)
        for r, o in enumerate(results[1:], 1):
            if o["T"].tobytes() != first["T"].tobytes():
                raise _native.NativeError("shard %d has a different template" % r)
        if "trend_chan" in first:
            merged["trend_chan"] = np.concatenate([o["trend_chan"] for o in results], axis=1)
            for r, o in enumerate(results[1:], 1):
                if o["trend_subint"].tobytes() != first["trend_subint"].tobytes():
                    raise _native.NativeError("shard %d has different subint trends" % r)
    return merged


def clean_cube_dist(cube_slice, w0_slice, shift_slice, global_shape, device, group=None,
                    want_residual=False, fail_at=None, **args):
    """This rank's channel shard of one archive under torch.distributed.
    `cube_slice` etc. are the rank's channel range (``_native.shard_layout``);
    returns the merged full-archive dict on every rank (with want_residual, the
    full residual cube on rank 0 only).  ``delay`` (in args): the slice's
    fractional delays (FFT-rotation dedispersion; (nchan_r,) or (nsub, nchan_r)).
    ``detrend`` / ``detrend_pieces`` with ``shard_detrend=True``: as
    clean_cube_local; the pieces are resolved against `global_shape`.
    ``std_template``, ``hotbins``, ``dynspec``: as clean_cube_local; every rank must pass the same."""
    import torch.distributed as dist

    from .dist import TorchComm
    nsub, nchan, nbin = global_shape
    comm = TorchComm(device, group, fail_at=fail_at)
    world, rank = comm.world, comm.rank
    chans, _ = _native.shard_layout(nsub, nchan, world)
    try:
        with _native.ShardSession(nsub, nchan, nbin, rank, world, comm=comm, device=_device_index(device),
                                  delay=args.get("delay"), **_loop_kwargs(args, (nsub, nchan), nbin)) as s:
            if np.ndim(cube_slice) == 4:   # full-pol: pscrunched on the GPU
                s.upload_pols(cube_slice, w0_slice, shift_slice)
            else:
                s.upload(cube_slice, w0_slice, shift_slice)
            out = s.run()
            if args.get("dynspec") and out["n_iter"] > 0:
                out["dynspec"] = s.dynspec()
            res = s.residual() if want_residual and out["n_iter"] > 0 else None
    except _native.NativeError:
        comm.abort()          # peers waiting in a collective with this rank must not block
        raise
    return _merge_dist(out, res, chans, (nsub, nchan, nbin), comm, group, want_residual)


def _merge_dist(out, res, chans, shape, comm, group, want_residual):
    """Every rank's (nsub, nchan_r) test / weights slices -> the full arrays on
    every rank, and the residual slices -> the full cube on rank 0, through
    tensor collectives (padded to the widest slice; RCCL on "nccl", host
    tensors on "gloo").  The scalar loop results are checked for agreement."""
    import torch
    import torch.distributed as dist
    nsub, nchan, nbin = shape
    world, rank = comm.world, comm.rank
    dev = comm.device if comm.backend != "gloo" else torch.device("cpu")
    wmax = max(c1 - c0 for c0, c1 in chans)
    nc = chans[rank][1] - chans[rank][0]
    scalars = {k: out[k] for k in ("loops", "n_iter", "converged")}
    scalars.update(changed=list(map(int, out["changed"])), nzero=list(map(int, out["nzero"])),
                   bad_fits=list(map(int, out.get("bad_fits", []))))
    if "std_alignment" in out:
        scalars["std_alignment"] = out["std_alignment"]
    every = [None] * world
    dist.all_gather_object(every, scalars, group=group)
    for r, sc in enumerate(every[1:], 1):
        if sc != every[0]:
            raise _native.NativeError("shard %d disagrees on the loop results: %s vs %s" % (r, sc, every[0]))
    merged = dict(out)

    def gather_cols(a, dtype, to_all=True):
        t = torch.zeros((nsub, wmax) + a.shape[2:], dtype=dtype, device=dev)
        t[:, :nc] = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        if to_all:
            parts = [torch.empty_like(t) for _ in range(world)]
            dist.all_gather(parts, t, group=group)
        else:
            parts = [torch.empty_like(t) for _ in range(world)] if rank == 0 else None
            dist.gather(t, parts, dst=0, group=group)
            if rank != 0:
                return None
        full = np.empty((nsub, nchan) + a.shape[2:], dtype=t.cpu().numpy().dtype)
        for (c0, c1), part in zip(chans, parts):
            full[:, c0:c1] = part[:, :c1 - c0].cpu().numpy()
        return full

    merged["test"] = gather_cols(out["test"], torch.float64)
    merged["weights"] = gather_cols(out["weights"], torch.float32)
    if "hotbins" in out:
        # sparse: the ranks' counts and lists as objects, merged on every rank
        from .hotbins import merge_shards
        parts = [None] * world
        dist.all_gather_object(parts, {k: out["hotbins"][k] for k in ("count", "offsets", "bins")}, group=group)
        merged["hotbins"] = merge_shards(parts)
    if "dynspec" in out:
        # the ranks' slices joined in rank order (dynspec.merge_shards), on every rank
        merged["dynspec"] = {k: gather_cols(out["dynspec"][k], torch.float64) for k in ("amp", "err", "base")}
    if want_residual:
        R = gather_cols(res if res is not None else np.zeros((nsub, nc, nbin), np.float32), torch.float32,
                        to_all=False)
        if rank == 0 and merged["n_iter"] > 0:
            merged["residual"] = R
    return merged


def _device_index(device):
    import torch
    d = torch.device(device)
    return d.index if d.index is not None else 0
