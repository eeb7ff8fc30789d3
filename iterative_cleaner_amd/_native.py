"""ctypes binding of libicgpu.so (include/iterative_cleaner.h).

The product path has no CPU fallback: if the HIP library is missing, cannot
be loaded, or no GPU is visible, the calls below raise ``NativeError``.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# IC_LIBRARY: an alternative build of the same library (A/B measurements)
LIB_PATH = os.environ.get("IC_LIBRARY") or os.path.join(HERE, "libicgpu.so")
ABI_VERSION = 9

# symbols exported by libicgpu.so, as declared in include/iterative_cleaner.h
EXPORTS = ("ic_abi_version", "ic_device_count", "ic_session_create", "ic_session_destroy",
           "ic_upload", "ic_upload_device", "ic_run", "ic_get_residual", "ic_get_template",
           "ic_get_fit", "ic_get_diagnostics", "ic_get_kernel_times", "ic_kernel_name",
           "ic_set_timing", "ic_get_run_stats", "ic_set_fit_tail", "ic_last_error",
           "ic_shard_layout", "ic_session_create_shard", "ic_group_create", "ic_group_destroy",
           "ic_session_create_grouped", "ic_upload_async", "ic_host_alloc", "ic_host_free",
           "ic_upload_pols", "ic_comprehensive_stats", "ic_get_bad_fits",
           "ic_fit_profiles", "ic_get_diagnostics_f64", "ic_set_delays", "ic_rotate_profiles",
           "ic_set_timing_kernel", "ic_set_option", "ic_get_option", "ic_comprehensive_stats_rowstat",
           "ic_rccl_unique_id", "ic_session_create_rccl", "ic_rccl_set_library", "ic_rccl_set_init_timeout",
           "ic_set_delays2", "ic_rotate_profiles2", "ic_upload_quantised", "ic_upload_quantised_async",
           "ic_decode_profiles", "ic_upload_delays_async", "ic_encode_profiles", "ic_get_residual_quantised",
           "ic_rotate_profiles_any", "ic_get_residual_quantised_async", "ic_residual_wait",
           "ic_set_detrend", "ic_get_trends", "ic_comprehensive_stats_detrend",
           "ic_set_detrend_pieces", "ic_get_trends_pieces", "ic_comprehensive_stats_detrend_pieces",
           "ic_shard_enable_detrend", "ic_set_std_template", "ic_get_std_alignment", "ic_align_template",
           "ic_set_hotbins", "ic_get_hotbins", "ic_get_hotbin_list", "ic_hotbins_profiles",
           "ic_get_dynspec", "ic_dynspec_profiles")

# session schedule options (ic_set_option; include/iterative_cleaner.h): they
# choose how the loop is scheduled, never its arithmetic
OPTIONS = {"fit_tail": 1, "diag_fork": 2, "fork_delay": 3, "template_incr": 4, "fit_tiled": 5,
           "rowstat_waves": 6, "rowstat_minlen": 7, "diag_chain": 8, "sync_timeout_ms": 9,
           "fit_schedule": 10, "tail_split": 13, "rot_stats": 14, "grid_cap": 15}
FIT_ROUNDS = 0   # IC_FIT_ROUNDS: sweep / state rounds (k_fit_pass, k_fit_state, k_fit_tail); the only schedule

Q_BIG_ENDIAN = 1   # IC_Q_BIG_ENDIAN: int16 samples in the FITS byte order

FIT_EXACT = 0    # IC_FIT_EXACT: scipy leastsq emulated bit for bit (the reference's arithmetic)
FIT_CLOSED = 1   # IC_FIT_CLOSED: closed-form amplitude fused with the diagnostics (fast mode)
DEDISP_SHIFT = 0  # IC_DEDISP_SHIFT: integer dedispersion shifts
DEDISP_FFT = 1    # IC_DEDISP_FFT: fractional delays, FFT phase rotation (phase_rotation.py)
DEDISP_FFT_ANY = 2    # IC_DEDISP_FFT_ANY (opt-in): the same, plus the chirp-z rotation of any other nbin in 16..4096


class NativeError(RuntimeError):
    pass


class Params(C.Structure):
    _fields_ = [("nsub", C.c_int32), ("nchan", C.c_int32), ("nbin", C.c_int32),
                ("max_iter", C.c_int32), ("chanthresh", C.c_double),
                ("subintthresh", C.c_double), ("pr_on", C.c_int32), ("pr_factor", C.c_double),
                ("pr_start", C.c_int32), ("pr_end", C.c_int32), ("baseline_duty", C.c_double),
                ("fit_mode", C.c_int32), ("data_f64", C.c_int32), ("dedisp_mode", C.c_int32),
                ("input_dedispersed", C.c_int32)]


class RunStats(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("fit_rounds", C.c_int32),
                ("fit_profile_sweeps", C.c_int64), ("fit_tail_sweeps", C.c_int64),
                ("window_moves", C.c_int32), ("near_threshold", C.c_int32), ("reserved0", C.c_int64),
                ("reserved1", C.c_int64)]


class KernelTime(C.Structure):
    _fields_ = [("kernel", C.c_int32), ("launches", C.c_int32), ("ms", C.c_double)]


# ic_comm_ops callbacks (include/iterative_cleaner.h)
ALLOC_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p))
RELEASE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p)
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
ALLTOALLV_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p,
                           C.POINTER(C.c_size_t), C.c_void_p)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)


class CommOps(C.Structure):
    _fields_ = [("ctx", C.c_void_p), ("alloc", ALLOC_FN), ("release", RELEASE_FN),
                ("allgather", ALLGATHER_FN), ("alltoallv", ALLTOALLV_FN),
                ("allreduce_sum_i32", ALLREDUCE_FN)]


_lib = None


def _init_torch_hip():
    """torch-ROCm bundles its own HIP runtime (torch/lib/libamdhip64.so) next to
    the one libicgpu.so links (/opt/rocm/lib/libamdhip64.so.7); both share the
    process's GPU address space, which is what lets torch tensors be passed to
    the C-ABI by pointer.  torch's runtime only finds the GPUs when it
    initialises first, so when torch is installed it is initialised before
    libicgpu is loaded (torch owns exchange buffers and streams in sharded and
    benchmark runs)."""
    try:
        import torch
    except ImportError:  # pragma: no cover - torch is part of the image
        return
    try:
        torch.cuda.is_available()
    except Exception:  # pragma: no cover
        pass


def load_library(path: str = LIB_PATH):
    """Load libicgpu.so (raises NativeError when absent — no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise NativeError("libicgpu.so not built at %s (run __graft_entry__.build() or make -C "
                          "iterative_cleaner_amd/csrc)" % path)
    _init_torch_hip()
    try:
        lib = C.CDLL(path)
    except OSError as e:  # pragma: no cover - environment dependent
        raise NativeError("cannot load %s: %s" % (path, e))
    vp = C.c_void_p
    lib.ic_abi_version.restype = C.c_int
    lib.ic_device_count.restype = C.c_int
    lib.ic_last_error.restype = C.c_char_p
    lib.ic_kernel_name.restype = C.c_char_p
    lib.ic_kernel_name.argtypes = [C.c_int]
    lib.ic_session_create.argtypes = [C.POINTER(Params), C.c_int, C.POINTER(vp)]
    lib.ic_session_destroy.argtypes = [vp]
    lib.ic_session_destroy.restype = None
    lib.ic_upload.argtypes = [vp, vp, vp, vp]
    lib.ic_upload_device.argtypes = [vp, vp, vp, vp]
    lib.ic_run.argtypes = [vp] * 8
    lib.ic_get_residual.argtypes = [vp, vp]
    lib.ic_get_template.argtypes = [vp, vp]
    lib.ic_get_fit.argtypes = [vp, vp, vp]
    lib.ic_get_diagnostics.argtypes = [vp, vp, vp, vp, vp]
    lib.ic_get_diagnostics_f64.argtypes = [vp, vp, vp, vp, vp]
    lib.ic_get_kernel_times.argtypes = [vp, C.POINTER(KernelTime), C.c_int]
    lib.ic_set_timing.argtypes = [vp, C.c_int]
    lib.ic_set_timing_kernel.argtypes = [vp, C.c_int]
    lib.ic_get_run_stats.argtypes = [vp, C.POINTER(RunStats)]
    lib.ic_set_fit_tail.argtypes = [vp, C.c_int64]
    lib.ic_set_option.argtypes = [vp, C.c_int, C.c_int64]
    lib.ic_get_option.argtypes = [vp, C.c_int, C.POINTER(C.c_int64)]
    lib.ic_upload_async.argtypes = [vp, vp, vp, vp]
    lib.ic_upload_pols.argtypes = [vp, vp, C.c_int, vp, vp]
    lib.ic_upload_quantised.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]
    lib.ic_upload_quantised_async.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]
    lib.ic_decode_profiles.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp]
    lib.ic_encode_profiles.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp]
    lib.ic_get_residual_quantised.argtypes = [vp, C.c_int, vp, vp, vp]
    lib.ic_get_residual_quantised_async.argtypes = [vp, C.c_int, vp, vp, vp]
    lib.ic_residual_wait.argtypes = [vp]
    lib.ic_host_alloc.argtypes = [C.c_size_t, C.POINTER(vp)]
    lib.ic_host_free.argtypes = [vp]
    lib.ic_host_free.restype = None
    lib.ic_shard_layout.argtypes = [C.c_int, C.c_int, C.c_int, vp, vp]
    lib.ic_session_create_shard.argtypes = [C.POINTER(Params), C.c_int, C.c_int, C.c_int,
                                            C.POINTER(CommOps), C.POINTER(vp)]
    lib.ic_group_create.argtypes = [C.c_int, C.POINTER(vp)]
    lib.ic_group_destroy.argtypes = [vp]
    lib.ic_group_destroy.restype = None
    lib.ic_session_create_grouped.argtypes = [C.POINTER(Params), C.c_int, vp, C.c_int, C.POINTER(vp)]
    lib.ic_rccl_unique_id.argtypes = [vp]
    lib.ic_session_create_rccl.argtypes = [C.POINTER(Params), C.c_int, C.c_int, C.c_int, vp, C.POINTER(vp)]
    lib.ic_rccl_set_library.argtypes = [C.c_char_p]
    lib.ic_rccl_set_init_timeout.argtypes = [C.c_int64]
    lib.ic_get_bad_fits.argtypes = [vp, vp, C.c_int]
    lib.ic_fit_profiles.argtypes = [C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, vp]
    lib.ic_set_delays.argtypes = [vp, vp]
    lib.ic_set_delays2.argtypes = [vp, vp]
    lib.ic_upload_delays_async.argtypes = [vp, vp, C.c_int]
    lib.ic_rotate_profiles.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp]
    lib.ic_rotate_profiles2.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp]
    lib.ic_rotate_profiles_any.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, vp]
    lib.ic_comprehensive_stats.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_double, C.c_double,
                                           vp, vp, vp, vp, vp]
    lib.ic_comprehensive_stats_rowstat.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_double,
                                                   C.c_double, vp, vp, vp, vp, vp, C.c_int, C.c_int]
    lib.ic_set_detrend.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_double]
    lib.ic_get_trends.argtypes = [vp, vp, vp]
    lib.ic_comprehensive_stats_detrend.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_double, C.c_double,
                                                   vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int,
                                                   C.c_double, vp, vp]
    lib.ic_set_detrend_pieces.argtypes = [vp, C.c_int, vp, C.c_int, vp]
    lib.ic_get_trends_pieces.argtypes = [vp, vp, vp]
    lib.ic_shard_enable_detrend.argtypes = [vp]
    lib.ic_set_std_template.argtypes = [vp, vp, C.c_int, C.c_int]
    lib.ic_get_std_alignment.argtypes = [vp, vp, vp, vp]
    lib.ic_align_template.argtypes = [C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp]
    lib.ic_set_hotbins.argtypes = [vp, C.c_double, C.c_int, C.c_int, C.c_int]
    lib.ic_get_hotbins.argtypes = [vp, vp, C.POINTER(C.c_int64)]
    lib.ic_get_hotbin_list.argtypes = [vp, vp, C.c_int64]
    lib.ic_hotbins_profiles.argtypes = [C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int, C.c_double, C.c_int, C.c_int,
                                        C.c_int, vp, vp, vp, C.c_int64, C.POINTER(C.c_int64)]
    lib.ic_get_dynspec.argtypes = [vp, vp, vp, vp]
    lib.ic_dynspec_profiles.argtypes = [C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
    lib.ic_comprehensive_stats_detrend_pieces.argtypes = (list(lib.ic_comprehensive_stats_detrend.argtypes)
                                                          + [C.c_int, vp, C.c_int, vp])
    if lib.ic_abi_version() != ABI_VERSION:
        raise NativeError("libicgpu ABI %d != expected %d" % (lib.ic_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def _err(lib) -> str:
    m = lib.ic_last_error()
    return m.decode() if m else ""


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def _piece_starts(spec, n):
    """One direction's pieces (None, a count, "wN" or starts) on lines of n
    entries -> (npieces, int32 starts or None) as the C-ABI takes them.  A list
    of starts goes to the library as it is: the library checks it."""
    from .detrend import piece_spec, resolve_pieces
    sp = piece_spec(spec, "detrend_pieces")
    if sp is None:
        return 0, None
    b = np.ascontiguousarray(sp if isinstance(sp, tuple) else resolve_pieces(sp, n), dtype=np.int32)
    return int(b.shape[0]), b


def device_count() -> int:
    return int(load_library().ic_device_count())


def normalise_pulse_region(pulse_region, nbin):
    """Reference K6 (iterative_cleaner.py:280-283): active iff != [0, 0, 1];
    (factor, start, end) with Python slice semantics on nbin."""
    if list(pulse_region) == [0, 0, 1]:
        return 0, 1.0, 0, 0
    start, stop, _ = slice(int(pulse_region[1]), int(pulse_region[2])).indices(nbin)
    if stop < start:
        stop = start
    return 1, float(pulse_region[0]), start, stop


class GpuSession:
    """One cleaning session on one GPU (wraps ic_session_*)."""

    def __init__(self, nsub, nchan, nbin, max_iter=5, chanthresh=5.0, subintthresh=5.0,
                 pulse_region=(0, 0, 1), baseline_duty=0.15, device=0, fit_mode=FIT_EXACT, data_f64=False,
                 delay=None, options=None, input_dedispersed=False, dedisp_fft=False, any_length=None,
                 detrend=None, detrend_pieces=None, std_template=None, hotbins=None):
        """delay: the session dedisperses by the FFT phase rotation (IC_DEDISP_FFT)
        with these delays (set_delays).  dedisp_fft=True: the same mode without
        delays yet: they come with set_delays, or with each archive
        (upload_async / upload_quantised_async delay=).  any_length (None = the
        IC_ANY_NBIN switch, phase_rotation.any_length_enabled): that mode is
        IC_DEDISP_FFT_ANY, which also serves any other nbin in 16..4096 by the
        chirp-z rotation (the lengths IC_DEDISP_FFT serves keep their bits).
        detrend = (chan_order, subint_order[, rounds, clip]): detrended scaling
        (set_detrend; detrend.py); None: ic_set_detrend is never called.
        detrend_pieces = (chan, subint): piecewise detrending
        (set_detrend_pieces); None: ic_set_detrend_pieces is never called.
        std_template = the standard profile (nbin,) or (profile, align): the
        opt-in cleaning against a supplied template (set_std_template;
        std_template.py); None: ic_set_std_template is never called.
        hotbins = (threshold, on_start, on_end[, rounds]): the opt-in hot-bin
        repair (set_hotbins; hotbins.py); None: ic_set_hotbins is never called
        (a session reads no environment switch: run_loop and clean_batch do)."""
        from .phase_rotation import any_length_enabled
        fft_mode = DEDISP_FFT_ANY if (any_length_enabled() if any_length is None else any_length) else DEDISP_FFT
        self.lib = load_library()
        self.shape = (int(nsub), int(nchan), int(nbin))
        self.max_iter = int(max_iter)
        self.fit_mode = int(fit_mode)
        on, fac, a, b = normalise_pulse_region(list(pulse_region), int(nbin))
        self.params = Params(int(nsub), int(nchan), int(nbin), int(max_iter), float(chanthresh),
                             float(subintthresh), on, fac, a, b, float(baseline_duty), self.fit_mode,
                             1 if data_f64 else 0, fft_mode if (delay is not None or dedisp_fft) else DEDISP_SHIFT,
                             1 if input_dedispersed else 0)
        self.data_f64 = bool(data_f64)
        h = C.c_void_p()
        rc = self._create(int(device), h)
        if rc != 0:
            raise NativeError("%s: %s (rc=%d)" % (self._create_name, _err(self.lib), rc))
        self.h = h
        self.pieces = None   # (mc, ms) while pieces are set
        self.std_mode = None   # IC_ALIGN_* while a standard template is set
        self.hotbins_on = False   # while the hot-bin repair is set
        try:
            for name, value in (options or {}).items():
                self.set_option(name, value)
            if delay is not None:
                self._initial_delays(delay)
            if detrend is not None:
                self.set_detrend(*detrend)
            if detrend_pieces is not None:
                self.set_detrend_pieces(*detrend_pieces)
            if std_template is not None:
                self.set_std_template(*_std_pair(std_template))
            if hotbins is not None:
                self.set_hotbins(*hotbins)
        except Exception:
            self.close()   # no half-made session is left for the collector (a shard's must go before its group)
            raise

    def set_detrend_pieces(self, chan, subint):
        """Piecewise detrending for the runs that follow (ic_set_detrend_pieces;
        the definition is detrend.py): the pieces of the channel lines (over
        the subints) and of the subint lines (over the channels), each None
        (one piece), a count, "wN" (a piece every N entries) or a sequence of
        starts.  With either given, detrended runs take the piecewise kernels;
        (None, None) goes back to the whole-line ones.  On a channel shard only
        with shard_detrend (ShardSession); the subint pieces are then those of
        the archive's whole subint lines, the same on every rank."""
        nsub, nchan, _ = getattr(self, "global_shape", self.shape)
        mc, cb = _piece_starts(chan, nsub)
        ms, sb = _piece_starts(subint, nchan)
        self._check(self.lib.ic_set_detrend_pieces(self.h, mc, _ptr(cb), ms, _ptr(sb)), "ic_set_detrend_pieces")
        self.pieces = (max(mc, 1), max(ms, 1)) if (mc or ms) else None

    def set_std_template(self, T, align="auto"):
        """Clean against the standard profile T (nbin,) in the runs that follow
        (ic_set_std_template; the definition is std_template.py): align "none"
        (as given), "int" (rolled by the cross-correlation lag), "frac" (rotated
        by lag + sub-bin part; only where the FFT rotation serves nbin) or
        "auto" (frac where available, else int).  The standard stays set across
        uploads; every run aligns it against that archive and is one pass.  On a
        channel shard every rank must set the same standard and mode."""
        from . import std_template as st
        nbin = self.shape[2]
        S = st.check(T, nbin)
        mode = st.resolve_align(align, nbin)
        self._check(self.lib.ic_set_std_template(self.h, _ptr(S), nbin, mode), "ic_set_std_template")
        self.std_mode = mode

    def clear_std_template(self):
        """Back to the iterative template (ic_set_std_template with NULL)."""
        self._check(self.lib.ic_set_std_template(self.h, None, self.shape[2], 0), "ic_set_std_template")
        self.std_mode = None

    def std_alignment(self):
        """The last run's alignment of the standard (ic_get_std_alignment):
        dict(aligned, lag, shift); all zero with align "none"."""
        al, lag = C.c_int32(), C.c_int32()
        sh = C.c_double()
        self._check(self.lib.ic_get_std_alignment(self.h, C.byref(al), C.byref(lag), C.byref(sh)),
                    "ic_get_std_alignment")
        return dict(aligned=int(al.value), lag=int(lag.value), shift=float(sh.value))

    def set_hotbins(self, threshold, on_start=0, on_end=0, rounds=4):
        """Hot-bin repair for the uploads consumed from here on (ic_set_hotbins;
        the definition is hotbins.py): the off-pulse bins of every profile more
        than `threshold` scaled MADs from their median are set to the median of
        the rest, once per upload, before the loop reads the cube.  The on-pulse
        window [on_start, on_end) is in the dedispersed frame (on_end <=
        on_start wraps; equal: none).  threshold <= 0 switches it off.  run()
        then carries ``hotbins`` = dict(count, total, offsets, bins)."""
        self._check(self.lib.ic_set_hotbins(self.h, float(threshold), int(on_start), int(on_end), int(rounds)),
                    "ic_set_hotbins")
        self.hotbins_on = float(threshold) > 0

    def clear_hotbins(self):
        """Switch the hot-bin repair off (ic_set_hotbins with threshold 0)."""
        self.set_hotbins(0.0)

    def hotbins(self):
        """The repair of the upload the last run() consumed (ic_get_hotbins,
        ic_get_hotbin_list): dict(count int32 (nsub, nchan): bins repaired, 0, or
        -1 = more than a quarter of the off-pulse bins stood out and the profile
        was left alone; total; offsets int64 [P + 1] and bins int32 [total]: the
        repaired bins in CSR layout, profiles in (s, c) order, bins ascending)."""
        from .hotbins import result_dict
        nsub, nchan, _ = self.shape
        count = np.empty((nsub, nchan), np.int32)
        total = C.c_int64()
        self._check(self.lib.ic_get_hotbins(self.h, _ptr(count), C.byref(total)), "ic_get_hotbins")
        bins = np.empty(int(total.value), np.int32)
        self._check(self.lib.ic_get_hotbin_list(self.h, _ptr(bins), int(total.value)), "ic_get_hotbin_list")
        return result_dict(count, bins)

    def set_detrend(self, chan_order, subint_order, rounds=4, clip=5.0):
        """Detrended scaling for the runs that follow (ic_set_detrend; the
        definition is detrend.py): polynomial orders 0..3 of the channel lines
        and of the subint lines, (0, 0) = off; on a channel shard only with
        shard_detrend (ShardSession)."""
        self._check(self.lib.ic_set_detrend(self.h, int(chan_order), int(subint_order), int(rounds), float(clip)),
                    "ic_set_detrend")

    def trends(self):
        """The last iteration's trend coefficients (ic_get_trends): (chan
        (4, nchan, 4), subint (4, nsub, 4)) f64, a_0..a_3 per line, diagnostics
        in the order std, mean, ptp, fftmax.  While pieces are set
        (set_detrend_pieces; ic_get_trends_pieces): (4, nchan, mc, 4) and
        (4, nsub, ms, 4).  On a channel shard (shard_detrend): the shard's own
        channels and all nsub rows (the rows are the same on every rank)."""
        nsub, nchan, _ = self.shape
        if self.pieces is not None:
            cc = np.empty((4, nchan, self.pieces[0], 4), np.float64)
            sc = np.empty((4, nsub, self.pieces[1], 4), np.float64)
            self._check(self.lib.ic_get_trends_pieces(self.h, _ptr(cc), _ptr(sc)), "ic_get_trends_pieces")
            return cc, sc
        cc = np.empty((4, nchan, 4), np.float64)
        sc = np.empty((4, nsub, 4), np.float64)
        self._check(self.lib.ic_get_trends(self.h, _ptr(cc), _ptr(sc)), "ic_get_trends")
        return cc, sc

    def _initial_delays(self, delay):
        self.set_delays(delay)

    def set_delays(self, delay):
        """Fractional delays in bins of a session created with `delay`
        (dedisp_mode IC_DEDISP_FFT), for this session's channels: (nchan,) per
        channel (ic_set_delays) or (nsub, nchan) per profile (ic_set_delays2)."""
        nsub, nchan = self.shape[0], self.shape[1]
        if np.ndim(delay) == 2:
            d = np.ascontiguousarray(delay, dtype=np.float64).reshape(nsub, nchan)
            self._check(self.lib.ic_set_delays2(self.h, _ptr(d)), "ic_set_delays2")
        else:
            d = np.ascontiguousarray(delay, dtype=np.float64).reshape(nchan)
            self._check(self.lib.ic_set_delays(self.h, _ptr(d)), "ic_set_delays")

    _create_name = "ic_session_create"

    def _create(self, device, h):
        return self.lib.ic_session_create(C.byref(self.params), device, C.byref(h))

    # context manager -----------------------------------------------------
    def close(self):
        if getattr(self, "h", None):
            self.lib.ic_session_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc < 0:
            raise NativeError("%s: %s (rc=%d)" % (what, _err(self.lib), rc))
        return rc

    # data ----------------------------------------------------------------
    def upload(self, cube, w0, shift):
        nsub, nchan, nbin = self.shape
        cube = np.ascontiguousarray(cube, dtype=np.float32).reshape(nsub, nchan, nbin)
        w0 = np.ascontiguousarray(w0, dtype=np.float32).reshape(nsub, nchan)
        shift = np.ascontiguousarray(np.mod(shift, nbin), dtype=np.int32).reshape(nchan)
        self._check(self.lib.ic_upload(self.h, _ptr(cube), _ptr(w0), _ptr(shift)), "ic_upload")

    def upload_pols(self, data, w0, shift):
        """Full-polarisation data (nsub, npol, nchan, nbin): pscrunched on the GPU."""
        nsub, nchan, nbin = self.shape
        data = np.ascontiguousarray(data, dtype=np.float32)
        if data.ndim != 4 or data.shape[0] != nsub or data.shape[2:] != (nchan, nbin):
            raise ValueError("upload_pols: data shape %s != (%d, npol, %d, %d)" % (data.shape, nsub, nchan, nbin))
        w0 = np.ascontiguousarray(w0, dtype=np.float32).reshape(nsub, nchan)
        shift = np.ascontiguousarray(np.mod(shift, nbin), dtype=np.int32).reshape(nchan)
        self._check(self.lib.ic_upload_pols(self.h, _ptr(data), int(data.shape[1]), _ptr(w0), _ptr(shift)),
                    "ic_upload_pols")

    def _check_delay(self, delay):
        """The delays of an asynchronous upload are handed over as they are (not
        copied): f64, C-contiguous, (nchan,) per channel or (nsub, nchan) per profile."""
        nsub, nchan = self.shape[0], self.shape[1]
        if (not isinstance(delay, np.ndarray) or delay.dtype != np.float64 or not delay.flags.c_contiguous
                or delay.shape not in ((nchan,), (nsub, nchan))):
            raise ValueError("delay must be a C-contiguous float64 array of shape (%d,) or (%d, %d)"
                             % (nchan, nsub, nchan))

    def _attach_delays(self, delay):
        """ic_upload_delays_async for the upload queued last."""
        self._check(self.lib.ic_upload_delays_async(self.h, _ptr(delay), 1 if delay.ndim == 2 else 0),
                    "ic_upload_delays_async")

    def upload_async(self, cube, w0, shift, delay=None):
        """Queue the copy of the next archive (see ic_upload_async); the arrays
        must stay alive and unmodified until the run() that consumes them returns.
        delay (an IC_DEDISP_FFT session): the archive's fractional delays, f64
        (nchan,) or (nsub, nchan), attached to this upload
        (ic_upload_delays_async): they become the session's delays when run()
        consumes it.  Not copied: the same rule as the other arrays."""
        nsub, nchan, nbin = self.shape
        for a, shape, dt in ((cube, (nsub, nchan, nbin), np.float32), (w0, (nsub, nchan), np.float32),
                             (shift, (nchan,), np.int32)):
            if a.dtype != dt or a.shape != shape or not a.flags.c_contiguous:
                raise ValueError("upload_async needs C-contiguous %s %s arrays" % (dt.__name__, shape))
        if delay is not None:
            self._check_delay(delay)
        self._check(self.lib.ic_upload_async(self.h, _ptr(cube), _ptr(w0), _ptr(shift)), "ic_upload_async")
        if delay is not None:
            self._attach_delays(delay)

    def upload_quantised(self, q, scl, offs, w0, shift, nsum):
        """PSRFITS samples as stored, decoded on the GPU (ic_upload_quantised):
        q int16 (nsub, npol, nchan, nbin) or (nsub, nchan, nbin) for one
        polarisation - dtype '>i2' is sent as it is and byte-swapped on the
        device - with scl / offs f32 (nsub, npol, nchan); the cube becomes
        pol 0 (nsum 1) or pol 0 + pol 1 (nsum 2) of psrfits.decode(q, scl, offs)."""
        nsub, nchan, nbin = self.shape
        q, flags = _quantised_samples(q)
        if q.ndim == 3:
            q = q.reshape(q.shape[0], 1, q.shape[1], q.shape[2])
        q = np.ascontiguousarray(q)
        if q.ndim != 4 or q.shape[0] != nsub or q.shape[2:] != (nchan, nbin):
            raise ValueError("upload_quantised: q shape %s != (%d, npol, %d, %d)" % (q.shape, nsub, nchan, nbin))
        npol = int(q.shape[1])
        scl = np.ascontiguousarray(scl, dtype=np.float32).reshape(nsub, npol, nchan)
        offs = np.ascontiguousarray(offs, dtype=np.float32).reshape(nsub, npol, nchan)
        w0 = np.ascontiguousarray(w0, dtype=np.float32).reshape(nsub, nchan)
        shift = np.ascontiguousarray(np.mod(shift, nbin), dtype=np.int32).reshape(nchan)
        self._check(self.lib.ic_upload_quantised(self.h, _ptr(q), _ptr(scl), _ptr(offs), npol, int(nsum), flags,
                                                 _ptr(w0), _ptr(shift)), "ic_upload_quantised")

    def upload_quantised_async(self, q, scl, offs, w0, shift, nsum, delay=None):
        """Queue the copy and the decode of the next archive
        (ic_upload_quantised_async); the arrays must stay alive and unmodified
        until the run() that consumes them returns.  delay: as upload_async."""
        nsub, nchan, nbin = self.shape
        if q.dtype.kind != "i" or q.dtype.itemsize != 2:
            raise ValueError("upload_quantised_async needs int16 samples (native or '>i2'), got %s" % q.dtype)
        flags = 0 if q.dtype.isnative else Q_BIG_ENDIAN
        npol = 1 if q.ndim == 3 else (q.shape[1] if q.ndim == 4 else -1)
        qshape = (nsub, nchan, nbin) if q.ndim == 3 else (nsub, npol, nchan, nbin)
        for a, shape, dt in ((q, qshape, q.dtype), (scl, (nsub, npol, nchan), np.dtype(np.float32)),
                             (offs, (nsub, npol, nchan), np.dtype(np.float32)),
                             (w0, (nsub, nchan), np.dtype(np.float32)), (shift, (nchan,), np.dtype(np.int32))):
            # a 1-pol archive's scales may come as (nsub, nchan)
            ok = a.shape == shape or (npol == 1 and shape[1:2] == (1,) and a.shape == (nsub, nchan))
            if a.dtype != dt or not ok or not a.flags.c_contiguous:
                raise ValueError("upload_quantised_async needs C-contiguous %s %s arrays" % (dt, shape))
        if delay is not None:
            self._check_delay(delay)
        self._check(self.lib.ic_upload_quantised_async(self.h, _ptr(q), _ptr(scl), _ptr(offs), npol, int(nsum),
                                                       flags, _ptr(w0), _ptr(shift)), "ic_upload_quantised_async")
        if delay is not None:
            self._attach_delays(delay)

    def upload_device(self, cube_ptr: int, w0_ptr: int, shift_ptr: int):
        """Device pointers (e.g. torch tensor .data_ptr()) on this session's GPU."""
        self._check(self.lib.ic_upload_device(self.h, C.c_void_p(cube_ptr), C.c_void_p(w0_ptr),
                                              C.c_void_p(shift_ptr)), "ic_upload_device")

    def run(self, fetch=True):
        nsub, nchan, _ = self.shape
        m = max(self.max_iter, 1)
        test = np.empty((nsub, nchan), np.float64) if fetch else None
        weights = np.empty((nsub, nchan), np.float32) if fetch else None
        loops = np.zeros(1, np.int32)
        changed = np.zeros(m, np.int32)
        nzero = np.zeros(m, np.int32)
        n_iter = np.zeros(1, np.int32)
        conv = np.zeros(1, np.int32)
        self._check(self.lib.ic_run(self.h, _ptr(test), _ptr(weights), _ptr(loops), _ptr(changed),
                                    _ptr(nzero), _ptr(n_iter), _ptr(conv)), "ic_run")
        k = int(n_iter[0])
        bad = np.zeros(m, np.int32)
        self._check(self.lib.ic_get_bad_fits(self.h, _ptr(bad), m), "ic_get_bad_fits")
        out = dict(test=test, weights=weights, loops=int(loops[0]), n_iter=k,
                   converged=bool(conv[0]), changed=changed[:k].copy(), nzero=nzero[:k].copy(),
                   bad_fits=bad[:k].copy())
        if self.std_mode is not None and k > 0:
            out["std_alignment"] = self.std_alignment()
        if self.hotbins_on:
            # (IC_ESTATE: switched on after a run had read this upload, which is
            # then left alone; the next upload gets the pass)
            rc = self.lib.ic_get_hotbins(self.h, None, None)
            if rc != -4:
                self._check(rc, "ic_get_hotbins")
                out["hotbins"] = self.hotbins()
        return out

    def residual(self):
        out = np.empty(self.shape, np.float32)
        self._check(self.lib.ic_get_residual(self.h, _ptr(out)), "ic_get_residual")
        return out

    def residual_quantised(self, big_endian=False):
        """residual() encoded on the GPU as a PSRFITS file stores it
        (ic_get_residual_quantised): (q int16 (nsub, nchan, nbin), scl, offs f32
        (nsub, nchan)), the bits of psrfits.quantise(residual()); the f32 cube is
        never downloaded.  big_endian: q in the FITS byte order, dtype '>i2'."""
        nsub, nchan, _ = self.shape
        q = np.empty(self.shape, ">i2" if big_endian else np.int16)
        scl = np.empty((nsub, nchan), np.float32)
        offs = np.empty((nsub, nchan), np.float32)
        self._check(self.lib.ic_get_residual_quantised(self.h, Q_BIG_ENDIAN if big_endian else 0, _ptr(q), _ptr(scl),
                                                       _ptr(offs)), "ic_get_residual_quantised")
        return q, scl, offs

    def residual_quantised_async(self, q, scl, offs):
        """Queue residual_quantised() into the caller's arrays
        (ic_get_residual_quantised_async) and return: the encode runs behind the
        last run(), the download beside whatever follows (the next run(), later
        uploads).  q: C-contiguous int16 (nsub, nchan, nbin), native or '>i2'
        (the dtype selects the byte order); scl, offs: C-contiguous f32 (nsub,
        nchan).  Page-locked arrays (PinnedArray) let the copy overlap.  They
        must stay alive, and hold nothing defined, until residual_wait() or
        close() returns."""
        check_residual_arrays(self.shape, q, scl, offs, "residual_quantised_async")
        self._check(self.lib.ic_get_residual_quantised_async(self.h, 0 if q.dtype.isnative else Q_BIG_ENDIAN, _ptr(q),
                                                             _ptr(scl), _ptr(offs)),
                    "ic_get_residual_quantised_async")

    def residual_wait(self):
        """Wait until every queued residual download has landed
        (ic_residual_wait); returns at once when none is pending."""
        self._check(self.lib.ic_residual_wait(self.h), "ic_residual_wait")

    def template(self):
        out = np.empty(self.shape[2], np.float32)
        self._check(self.lib.ic_get_template(self.h, _ptr(out)), "ic_get_template")
        return out

    def dynspec(self):
        """The dynamic spectrum of the cube the last run() consumed
        (ic_get_dynspec; the definition is dynspec.py): dict(amp, err, base),
        f64 (nsub, nchan) (a shard: its channel slice): the amplitude of the
        run's template in every dedispersed profile by a fit with a free
        baseline, its error, and that baseline; profiles the run left with
        weight 0 hold zeros.  Launched here, never by run()."""
        nsub, nchan, _ = self.shape
        amp, err, base = (np.empty((nsub, nchan), np.float64) for _ in range(3))
        self._check(self.lib.ic_get_dynspec(self.h, _ptr(amp), _ptr(err), _ptr(base)), "ic_get_dynspec")
        return dict(amp=amp, err=err, base=base)

    def fit(self):
        nsub, nchan, _ = self.shape
        amp = np.empty((nsub, nchan), np.float64)
        info = np.empty((nsub, nchan), np.int32)
        self._check(self.lib.ic_get_fit(self.h, _ptr(amp), _ptr(info)), "ic_get_fit")
        return amp, info

    def diagnostics(self):
        """(std, mean, ptp, fftmax) of the last iteration; ptp is f32 for f32 data
        (numpy.ma's dtype), f64 with data_f64."""
        nsub, nchan, _ = self.shape
        sd, mn, ff = (np.empty((nsub, nchan), np.float64) for _ in range(3))
        if self.data_f64:
            pt = np.empty((nsub, nchan), np.float64)
            self._check(self.lib.ic_get_diagnostics_f64(self.h, _ptr(sd), _ptr(mn), _ptr(pt), _ptr(ff)),
                        "ic_get_diagnostics_f64")
        else:
            pt = np.empty((nsub, nchan), np.float32)
            self._check(self.lib.ic_get_diagnostics(self.h, _ptr(sd), _ptr(mn), _ptr(pt), _ptr(ff)),
                        "ic_get_diagnostics")
        return sd, mn, pt, ff

    def set_timing(self, on: bool, only: str | None = None):
        """Per-kernel HIP-event timing of the following runs; `only`: one kernel
        name (the others run without events)."""
        kid = -1
        if only is not None:
            names = [self.lib.ic_kernel_name(q).decode() for q in range(64)]
            if only not in names:
                raise ValueError("unknown kernel %r" % only)
            kid = names.index(only)
        self._check(self.lib.ic_set_timing_kernel(self.h, kid), "ic_set_timing_kernel")
        self._check(self.lib.ic_set_timing(self.h, 1 if on else 0), "ic_set_timing")

    def set_fit_tail(self, threshold: int):
        """Profiles left at which k_fit_tail takes over the fit (0 = never)."""
        self._check(self.lib.ic_set_fit_tail(self.h, int(threshold)), "ic_set_fit_tail")

    def set_option(self, name: str, value: int):
        """A schedule option (OPTIONS; ic_set_option validates the value)."""
        if name not in OPTIONS:
            raise ValueError("unknown option %r (one of %s)" % (name, ", ".join(sorted(OPTIONS))))
        self._check(self.lib.ic_set_option(self.h, OPTIONS[name], int(value)), "ic_set_option(%s)" % name)

    def get_option(self, name: str) -> int:
        v = C.c_int64()
        self._check(self.lib.ic_get_option(self.h, OPTIONS[name], C.byref(v)), "ic_get_option(%s)" % name)
        return int(v.value)

    def run_stats(self):
        st = RunStats()
        self._check(self.lib.ic_get_run_stats(self.h, C.byref(st)), "ic_get_run_stats")
        return dict(iterations=st.iterations, fit_rounds=st.fit_rounds,
                    fit_profile_sweeps=int(st.fit_profile_sweeps),
                    fit_tail_sweeps=int(st.fit_tail_sweeps),
                    window_moves=int(st.window_moves), near_threshold=int(st.near_threshold))

    def kernel_times(self):
        buf = (KernelTime * 32)()
        n = self._check(self.lib.ic_get_kernel_times(self.h, buf, 32), "ic_get_kernel_times")
        out = {}
        for q in range(n):
            name = self.lib.ic_kernel_name(buf[q].kernel).decode()
            out[name] = dict(ms=buf[q].ms, launches=buf[q].launches)
        return out


def _std_pair(std_template):
    """A std_template argument of a session (a profile, or (profile, align)) ->
    (profile, align)."""
    if (isinstance(std_template, (tuple, list)) and len(std_template) == 2
            and isinstance(std_template[1], (str, int, np.integer)) and np.ndim(std_template[0]) == 1):
        return std_template[0], std_template[1]
    return std_template, "auto"


def align_template(S, A, align="auto", device=0):
    """The alignment kernels alone (ic_align_template): the standard S against
    the template A, both (nbin,) -> dict(aligned, lag, shift, template, mode) as
    std_template.align states it."""
    from . import std_template as st
    lib = load_library()
    S = st.check(S, np.shape(S)[0] if np.ndim(S) == 1 else st.MIN_NBIN)
    nbin = S.shape[0]
    mode = st.resolve_align(align, nbin)
    A = np.ascontiguousarray(A, dtype=np.float32).reshape(nbin)
    out = np.empty(nbin, np.float32)
    al, lag = C.c_int32(), C.c_int32()
    sh = C.c_double()
    rc = lib.ic_align_template(int(device), nbin, _ptr(S), _ptr(A), mode, _ptr(out), C.byref(al), C.byref(lag),
                               C.byref(sh))
    if rc != 0:
        raise NativeError("ic_align_template: %s (rc=%d)" % (_err(lib), rc))
    return dict(aligned=int(al.value), lag=int(lag.value), shift=float(sh.value), template=out, mode=mode)


def hotbins_profiles(profiles, w, offsets, widen, threshold, on_start, on_end, rounds=4, device=0):
    """The hot-bin kernels alone (ic_hotbins_profiles) on (nprof, nbin) f32
    profiles with weights w (nprof,) and offsets (nprof,) int32 (None: 0), as
    hotbins.repair_profiles states them: (out, count int32, bins int32 CSR)."""
    lib = load_library()
    p = np.ascontiguousarray(profiles, dtype=np.float32)
    if p.ndim != 2:
        raise ValueError("hotbins_profiles: profiles must be (nprof, nbin)")
    nprof, nbin = p.shape
    w = np.ascontiguousarray(w, dtype=np.float32).reshape(nprof)
    off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.int32).reshape(nprof)
    out = np.empty_like(p)
    count = np.empty(nprof, np.int32)
    total = C.c_int64()
    args = [int(device), nprof, nbin, _ptr(p), _ptr(w), _ptr(off), 1 if widen else 0, float(threshold),
            int(on_start), int(on_end), int(rounds), _ptr(out), _ptr(count)]
    rc = lib.ic_hotbins_profiles(*args, None, 0, C.byref(total))
    if rc != 0:
        raise NativeError("ic_hotbins_profiles: %s (rc=%d)" % (_err(lib), rc))
    bins = np.empty(int(total.value), np.int32)
    if total.value:
        rc = lib.ic_hotbins_profiles(*args, _ptr(bins), int(total.value), C.byref(total))
        if rc != 0:
            raise NativeError("ic_hotbins_profiles: %s (rc=%d)" % (_err(lib), rc))
    return out, count, bins


def dynspec_profiles(template, profiles, w, device=0):
    """The dynamic-spectrum kernels alone (ic_dynspec_profiles) on (nprof, nbin)
    f32 dedispersed profiles with the template (nbin,) and weights w (nprof,),
    as dynspec.profiles states them: dict(amp, err, base), f64 (nprof,)."""
    lib = load_library()
    p = np.ascontiguousarray(profiles, dtype=np.float32)
    if p.ndim != 2:
        raise ValueError("dynspec_profiles: profiles must be (nprof, nbin)")
    nprof, nbin = p.shape
    T = np.ascontiguousarray(template, dtype=np.float32)
    if T.shape != (nbin,):
        raise ValueError("dynspec_profiles: the template must be (%d,), got %s" % (nbin, T.shape))
    w = np.ascontiguousarray(w, dtype=np.float32)
    if w.size != nprof:
        raise ValueError("dynspec_profiles: %d weights for %d profiles" % (w.size, nprof))
    amp, err, base = (np.empty(nprof, np.float64) for _ in range(3))
    rc = lib.ic_dynspec_profiles(int(device), nprof, nbin, _ptr(T), _ptr(p), _ptr(w), _ptr(amp), _ptr(err),
                                 _ptr(base))
    if rc != 0:
        raise NativeError("ic_dynspec_profiles: %s (rc=%d)" % (_err(lib), rc))
    return dict(amp=amp, err=err, base=base)


def fit_profiles(profiles, template, fit_mode=FIT_EXACT, device=0):
    """remove_profile1d (iterative_cleaner.py:275-288) on the GPU for the
    (nprof, nbin) profiles: (amp f64, info i32, residual f32 a*T - p)."""
    lib = load_library()
    P = np.ascontiguousarray(profiles, dtype=np.float32)
    if P.ndim != 2:
        raise ValueError("fit_profiles: profiles must be (nprof, nbin)")
    T = np.ascontiguousarray(template, dtype=np.float32).reshape(P.shape[1])
    amp = np.empty(P.shape[0], np.float64)
    info = np.empty(P.shape[0], np.int32)
    R = np.empty(P.shape, np.float32)
    rc = lib.ic_fit_profiles(int(device), P.shape[0], P.shape[1], _ptr(T), _ptr(P), int(fit_mode), _ptr(amp),
                             _ptr(info), _ptr(R))
    if rc != 0:
        raise NativeError("ic_fit_profiles: %s (rc=%d)" % (_err(lib), rc))
    return amp, info, R


def _quantised_samples(q):
    """(array, flags): int16 samples as they are - '>i2' keeps the FITS byte
    order and sets IC_Q_BIG_ENDIAN - anything else converted to native int16."""
    q = np.asarray(q)
    if q.dtype.kind == "i" and q.dtype.itemsize == 2:
        return q, (0 if q.dtype.isnative else Q_BIG_ENDIAN)
    return q.astype(np.int16), 0


def decode_profiles(q, scl, offs, nsum, device=0):
    """PSRFITS decode and polarisation sum on the GPU (ic_decode_profiles):
    q int16 (nsub, npol, nchan, nbin) (dtype '>i2': byte-swapped on the
    device), scl / offs f32 (nsub, npol, nchan) -> (nsub, nchan, nbin) f32,
    pol 0 (nsum 1) or pol 0 + pol 1 (nsum 2) of psrfits.decode(q, scl, offs)."""
    lib = load_library()
    q, flags = _quantised_samples(q)
    q = np.ascontiguousarray(q)
    if q.ndim != 4:
        raise ValueError("decode_profiles: q must be (nsub, npol, nchan, nbin)")
    nsub, npol, nchan, nbin = q.shape
    scl = np.ascontiguousarray(scl, dtype=np.float32).reshape(nsub, npol, nchan)
    offs = np.ascontiguousarray(offs, dtype=np.float32).reshape(nsub, npol, nchan)
    out = np.empty((nsub, nchan, nbin), np.float32)
    rc = lib.ic_decode_profiles(int(device), nsub, npol, int(nsum), nchan, nbin, _ptr(q), _ptr(scl), _ptr(offs),
                                flags, _ptr(out))
    if rc != 0:
        raise NativeError("ic_decode_profiles: %s (rc=%d)" % (_err(lib), rc))
    return out


def encode_profiles(cube, big_endian=False, device=0):
    """PSRFITS encode on the GPU (ic_encode_profiles): (nsub, nchan, nbin) f32 ->
    (q int16 (nsub, nchan, nbin), scl, offs f32 (nsub, nchan)), the bits of
    psrfits.quantise; big_endian: q in the FITS byte order, dtype '>i2'."""
    lib = load_library()
    cube = np.ascontiguousarray(cube, dtype=np.float32)
    if cube.ndim != 3:
        raise ValueError("encode_profiles: cube must be (nsub, nchan, nbin)")
    nsub, nchan, nbin = cube.shape
    q = np.empty(cube.shape, ">i2" if big_endian else np.int16)
    scl = np.empty((nsub, nchan), np.float32)
    offs = np.empty((nsub, nchan), np.float32)
    rc = lib.ic_encode_profiles(int(device), nsub, nchan, nbin, _ptr(cube), Q_BIG_ENDIAN if big_endian else 0,
                                _ptr(q), _ptr(scl), _ptr(offs))
    if rc != 0:
        raise NativeError("ic_encode_profiles: %s (rc=%d)" % (_err(lib), rc))
    return q, scl, offs


def rotate_profiles(cube, delay, sign=1, device=0, any_length=None):
    """Fractional dedispersion of a (nsub, nchan, nbin) cube on the GPU: the FFT
    phase rotation by +delay (sign 1, dedisperse) or -delay (sign -1); delay
    (nchan,) per channel (ic_rotate_profiles) or (nsub, nchan) per profile
    (ic_rotate_profiles2).  any_length (None = the IC_ANY_NBIN switch):
    ic_rotate_profiles_any, which also serves any other nbin in 16..4096."""
    from .phase_rotation import any_length_enabled
    if any_length is None:
        any_length = any_length_enabled()
    lib = load_library()
    cube = np.ascontiguousarray(cube, dtype=np.float32)
    if cube.ndim != 3:
        raise ValueError("rotate_profiles: cube must be (nsub, nchan, nbin)")
    nsub, nchan, nbin = cube.shape
    out = np.empty_like(cube)
    if np.ndim(delay) == 2:
        d = np.ascontiguousarray(delay, dtype=np.float64).reshape(nsub, nchan)
        fn, name = lib.ic_rotate_profiles2, "ic_rotate_profiles2"
    else:
        d = np.ascontiguousarray(delay, dtype=np.float64).reshape(nchan)
        fn, name = lib.ic_rotate_profiles, "ic_rotate_profiles"
    if any_length:
        name = "ic_rotate_profiles_any"
        rc = lib.ic_rotate_profiles_any(int(device), nsub, nchan, nbin, _ptr(cube), _ptr(d), int(d.ndim == 2),
                                        int(sign), _ptr(out))
    else:
        rc = fn(int(device), nsub, nchan, nbin, _ptr(cube), _ptr(d), int(sign), _ptr(out))
    if rc != 0:
        raise NativeError("%s: %s (rc=%d)" % (name, _err(lib), rc))
    return out


def comprehensive_stats(data, weights, chanthresh=5.0, subintthresh=5.0, device=0, diagnostics=False,
                        rowstat_waves=8, rowstat_minlen=1024, detrend=None, data_f64=False, detrend_pieces=None):
    """comprehensive_stats (iterative_cleaner.py:181-226) on the GPU for the
    (nsub, nchan, nbin) data and (nsub, nchan) weights the reference masks and
    weights at :111-117; returns test [, (std, mean, ptp, fftmax)].
    rowstat_*: the row-median form (IC_OPT_ROWSTAT_WAVES / _MINLEN).
    detrend = (chan_order, subint_order[, rounds, clip]): the detrended scaling
    (ic_comprehensive_stats_detrend; detrend.py), with data_f64 the f64
    statistics of a psrchive build; returns test, (chan_coef (4, nchan, 4),
    subint_coef (4, nsub, 4)) [, (std, mean, ptp, fftmax)], ptp f64 with
    data_f64.  detrend_pieces = (chan, subint) (GpuSession.set_detrend_pieces;
    needs detrend): the piecewise kernels (ic_comprehensive_stats_detrend_pieces),
    the coefficients then (4, nchan, mc, 4) and (4, nsub, ms, 4)."""
    lib = load_library()
    data = np.ascontiguousarray(data, dtype=np.float32)
    if data.ndim != 3:
        raise ValueError("comprehensive_stats: data must be (nsub, nchan, nbin)")
    nsub, nchan, nbin = data.shape
    w = np.ascontiguousarray(weights, dtype=np.float32).reshape(nsub, nchan)
    test = np.empty((nsub, nchan), np.float64)
    if detrend is None and data_f64:
        raise ValueError("comprehensive_stats: data_f64 needs detrend")
    if detrend is None and detrend_pieces is not None:
        raise ValueError("comprehensive_stats: detrend_pieces needs detrend")
    if detrend is not None:
        t = tuple(detrend)
        co, so = t[:2]
        rounds, clip = (t[2] if len(t) > 2 else 4), (t[3] if len(t) > 3 else 5.0)
        sd, mn, pt, ff = (np.empty((nsub, nchan), np.float64) for _ in range(4))
        args = [int(device), nsub, nchan, nbin, _ptr(data), _ptr(w), float(chanthresh), float(subintthresh),
                _ptr(test), _ptr(sd), _ptr(mn), _ptr(pt), _ptr(ff), 1 if data_f64 else 0, int(co), int(so),
                int(rounds), float(clip)]
        if detrend_pieces is not None:
            chan, subint = detrend_pieces
            mc, cb = _piece_starts(chan, nsub)
            ms, sb = _piece_starts(subint, nchan)
            cc = np.empty((4, nchan, max(mc, 1), 4), np.float64)
            sc = np.empty((4, nsub, max(ms, 1), 4), np.float64)
            name = "ic_comprehensive_stats_detrend_pieces"
            rc = lib.ic_comprehensive_stats_detrend_pieces(*args, _ptr(cc), _ptr(sc), mc, _ptr(cb), ms, _ptr(sb))
        else:
            cc = np.empty((4, nchan, 4), np.float64)
            sc = np.empty((4, nsub, 4), np.float64)
            name = "ic_comprehensive_stats_detrend"
            rc = lib.ic_comprehensive_stats_detrend(*args, _ptr(cc), _ptr(sc))
        if rc != 0:
            raise NativeError("%s: %s (rc=%d)" % (name, _err(lib), rc))
        if not data_f64:
            pt = pt.astype(np.float32)   # exact: f32 values
        return (test, (cc, sc), (sd, mn, pt, ff)) if diagnostics else (test, (cc, sc))
    sd, mn, ff = (np.empty((nsub, nchan), np.float64) for _ in range(3)) if diagnostics else (None,) * 3
    pt = np.empty((nsub, nchan), np.float32) if diagnostics else None
    rc = lib.ic_comprehensive_stats_rowstat(int(device), nsub, nchan, nbin, _ptr(data), _ptr(w),
                                            float(chanthresh), float(subintthresh), _ptr(test), _ptr(sd),
                                            _ptr(mn), _ptr(pt), _ptr(ff), int(rowstat_waves), int(rowstat_minlen))
    if rc != 0:
        raise NativeError("ic_comprehensive_stats: %s (rc=%d)" % (_err(lib), rc))
    return (test, (sd, mn, pt, ff)) if diagnostics else test


def check_residual_arrays(shape, q, scl, offs, what):
    """The destination of an asynchronous residual download, handed over as it
    is (not copied): q C-contiguous int16 (native or '>i2') of the session's
    shape, scl / offs C-contiguous f32 (nsub, nchan)."""
    nsub, nchan, nbin = shape
    f32 = np.dtype(np.float32)
    if (not isinstance(q, np.ndarray) or q.dtype.kind != "i" or q.dtype.itemsize != 2
            or q.shape != (nsub, nchan, nbin) or not q.flags.c_contiguous):
        raise ValueError("%s needs C-contiguous int16 (native or '>i2') samples of shape %s"
                         % (what, (nsub, nchan, nbin)))
    for a in (scl, offs):
        if not isinstance(a, np.ndarray) or a.dtype != f32 or a.shape != (nsub, nchan) or not a.flags.c_contiguous:
            raise ValueError("%s needs C-contiguous float32 %s scl / offs arrays" % (what, (nsub, nchan)))


class PinnedArray:
    """Page-locked host memory (ic_host_alloc) viewed as a numpy array, so that
    ic_upload_async copies overlap the cleaning of the previous archive."""

    def __init__(self, shape, dtype=np.float32):
        self.lib = load_library()
        dt = np.dtype(dtype)
        n = int(np.prod(shape)) * dt.itemsize
        p = C.c_void_p()
        if self.lib.ic_host_alloc(n, C.byref(p)) != 0:
            raise NativeError("ic_host_alloc: %s" % _err(self.lib))
        self.ptr = p
        buf = (C.c_char * max(n, 1)).from_address(p.value)
        self.array = np.frombuffer(buf, dtype=dt, count=int(np.prod(shape))).reshape(shape)

    def close(self):
        if getattr(self, "ptr", None):
            self.array = None
            self.lib.ic_host_free(self.ptr)
            self.ptr = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------- channel shards

def shard_layout(nsub, nchan, world):
    """([(c0, c1)] per rank, [(s0, s1)] per rank) from ic_shard_layout (C++),
    the rule of iterative_cleaner_amd/shards.py."""
    lib = load_library()
    cr = np.zeros(2 * world, np.int32)
    rr = np.zeros(2 * world, np.int32)
    rc = lib.ic_shard_layout(int(nsub), int(nchan), int(world), _ptr(cr), _ptr(rr))
    if rc != 0:
        raise NativeError("ic_shard_layout: %s (rc=%d)" % (_err(lib), rc))
    return ([(int(cr[2 * r]), int(cr[2 * r + 1])) for r in range(world)],
            [(int(rr[2 * r]), int(rr[2 * r + 1])) for r in range(world)])


def rccl_unique_id() -> bytes:
    """128-byte RCCL unique id (ncclGetUniqueId through ic_rccl_unique_id), made
    by rank 0 and handed once to every rank of a native-RCCL shard group."""
    lib = load_library()
    buf = (C.c_char * 128)()
    rc = lib.ic_rccl_unique_id(C.cast(buf, C.c_void_p))
    if rc != 0:
        raise NativeError("ic_rccl_unique_id: %s (rc=%d)" % (_err(lib), rc))
    return bytes(buf.raw)


def rccl_set_library(path):
    """Load `path` instead of the ROCm install's librccl (ic_rccl_set_library;
    None = the default).  Process-wide, before the first RCCL use."""
    lib = load_library()
    rc = lib.ic_rccl_set_library(None if path is None else os.fsencode(path))
    if rc != 0:
        raise NativeError("ic_rccl_set_library: %s (rc=%d)" % (_err(lib), rc))


def rccl_set_init_timeout(ms):
    """How long ic_session_create_rccl waits for every rank to join (ms)."""
    lib = load_library()
    rc = lib.ic_rccl_set_init_timeout(int(ms))
    if rc != 0:
        raise NativeError("ic_rccl_set_init_timeout: %s (rc=%d)" % (_err(lib), rc))


class ShardGroup:
    """In-process shard group (ic_group_create): `world` shard sessions driven
    by `world` host threads of this process, exchanging by device copies."""

    def __init__(self, world):
        self.lib = load_library()
        self.world = int(world)
        h = C.c_void_p()
        if self.lib.ic_group_create(self.world, C.byref(h)) != 0:
            raise NativeError("ic_group_create: %s" % _err(self.lib))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.ic_group_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class ShardSession(GpuSession):
    """Channel shard `rank` of `world` of one archive (global shape in the
    arguments; uploads and per-profile outputs are the shard's channel slice).
    Exchanges go through `group` (a ShardGroup: in-process), `comm` (an object
    with ``ops()`` returning a CommOps, e.g. dist.TorchComm: host callbacks) or
    `rccl_id` (rank 0's rccl_unique_id(): the library's own RCCL communicator,
    every collective issued from C++ on the session stream).
    shard_detrend=True opts in to detrending on shards (ic_shard_enable_detrend)
    before detrend= / detrend_pieces= are applied; every rank of the group must
    pass it with the same detrend settings, and detrend_pieces then cut the
    archive's whole subint lines (global nchan)."""

    _create_name = "ic_session_create_shard"

    def __init__(self, nsub, nchan, nbin, rank, world, group=None, comm=None, rccl_id=None, shard_detrend=False,
                 **kw):
        if sum(x is not None for x in (group, comm, rccl_id)) != 1:
            raise ValueError("ShardSession needs exactly one of group / comm / rccl_id")
        if rccl_id is not None and len(rccl_id) != 128:
            raise ValueError("rccl_id must be the 128 bytes of rccl_unique_id()")
        self.rank, self.world = int(rank), int(world)
        self.group, self.comm, self.rccl_id = group, comm, rccl_id
        chans, rows = shard_layout(nsub, nchan, world)
        self.chan_range = chans[self.rank]
        self.row_range = rows[self.rank]
        self.global_shape = (int(nsub), int(nchan), int(nbin))
        self._delay = None
        detrend, pieces = kw.pop("detrend", None), kw.pop("detrend_pieces", None)
        super().__init__(nsub, nchan, nbin, **kw)
        try:
            if shard_detrend:
                self._check(self.lib.ic_shard_enable_detrend(self.h), "ic_shard_enable_detrend")
            if detrend is not None:
                self.set_detrend(*detrend)
            if pieces is not None:
                self.set_detrend_pieces(*pieces)
            c0, c1 = self.chan_range
            self.shape = (int(nsub), c1 - c0, int(nbin))
            if self._delay is not None:   # the shard's own channels
                self.set_delays(self._delay)
        except Exception:
            self.close()
            raise

    def _initial_delays(self, delay):
        self._delay = delay

    def _create(self, device, h):
        if self.group is not None:
            self._create_name = "ic_session_create_grouped"
            return self.lib.ic_session_create_grouped(C.byref(self.params), device, self.group.h,
                                                      self.rank, C.byref(h))
        if self.rccl_id is not None:
            self._create_name = "ic_session_create_rccl"
            self._id_buf = C.create_string_buffer(self.rccl_id, 128)
            return self.lib.ic_session_create_rccl(C.byref(self.params), device, self.rank, self.world,
                                                   C.cast(self._id_buf, C.c_void_p), C.byref(h))
        self._ops = self.comm.ops()
        return self.lib.ic_session_create_shard(C.byref(self.params), device, self.rank,
                                                self.world, C.byref(self._ops), C.byref(h))

    def _check(self, rc, what):
        if rc < 0 and self.comm is not None and getattr(self.comm, "error", None):
            raise NativeError("%s: %s (rc=%d); transport: %s"
                              % (what, _err(self.lib), rc, self.comm.error))
        return super()._check(rc, what)
