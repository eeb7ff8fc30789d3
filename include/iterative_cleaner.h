/*
 * iterative_cleaner.h — C-ABI of libicgpu.so, the MI355X (gfx950) surgical
 * RFI-cleaning loop.
 *
 * The reference has no FFI layer; its drop-in boundary is the Python function
 * clean(ar, args, arch) (/root/reference/iterative_cleaner.py:65).  The
 * entry points below replace the body of its cleaning loop,
 * iterative_cleaner.py:83-146 (template :88-94, fit-cube prep :96-100,
 * remove_profile_inplace :101/:259-288, dededisperse :104, apply_weights
 * :111-117/:291-297, comprehensive_stats :120/:181-256, set_weights_archive
 * :122-125/:300-305, convergence :127-146).  The Python host
 * (iterative_cleaner_amd/cleaner.py) keeps the reference's CLI, clean()
 * signature, prints, log and file side effects, and binds these symbols with
 * ctypes (INTEGRATION.md shows the binding).
 *
 * Conventions
 *   - plain pointers and sizes only; host arrays are caller-owned and copied;
 *   - return 0 on success, a negative IC_E* code on error; the message of the
 *     last error on the calling thread is ic_last_error();
 *   - one session per host thread; sessions on different devices may run
 *     concurrently (every call is synchronous on the session's HIP stream).
 *
 * Layouts: cube[s][c][b] float32 (nsub, nchan, nbin), profile-contiguous, in
 * the DISPERSED frame, already pscrunched (total intensity); weights[s][c]
 * float32; shift[c] = dedispersion delay in bins (ded[i] = raw[(i+shift)%nbin]).
 */
#ifndef ITERATIVE_CLEANER_H
#define ITERATIVE_CLEANER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IC_ABI_VERSION 9

#define IC_OK 0
#define IC_EINVAL -1   /* bad argument / shape                         */
#define IC_EHIP -2     /* HIP runtime error                            */
#define IC_ENOMEM -3   /* device or host allocation failed             */
#define IC_ESTATE -4   /* call out of order (e.g. run before upload)   */
#define IC_ECOMM -5    /* a shard exchange failed (or a peer aborted)  */

/* Loop parameters: args Namespace of iterative_cleaner.py:16-42.
 * nbin: a power of two in 64..8192 runs the templated diagnostics kernels
 * (k_diag_p2 / k_diag_cl; at 8192 a profile is shared by eight waves), a
 * mixed-radix length (see dedisp_mode) k_diag_mr, and any other length from
 * 129 to 4096 (odd ones to 2048) k_diag_czt, whose fftmax is a chirp-z
 * transform; all of these serve the diagnostics fork.  What is left (below
 * 129, odd above 2048, beyond 4096) runs the generic direct-DFT k_diag,
 * unforked, as far as its per-profile LDS need allows
 * (ic_session_create says how many bytes a refused length would take: every
 * power of two above 8192 is refused that way).  With IC_DEDISP_FFT the
 * length must also be one the rotation serves (see dedisp_mode below).
 * nsub, nchan <= 16384. */
typedef struct {
    int32_t nsub, nchan, nbin;
    int32_t max_iter;          /* -m                                          */
    double chanthresh;         /* -c  (iterative_cleaner.py:19, default 5)     */
    double subintthresh;       /* -s  (:23, default 5)                         */
    int32_t pr_on;             /* pulse_region != [0,0,1] (:280)               */
    double pr_factor;          /* pulse_region[0] (:283)                       */
    int32_t pr_start, pr_end;  /* slice(int(pr[1]), int(pr[2])).indices(nbin) */
    double baseline_duty;      /* archive stand-in remove_baseline duty (0.15) */
    int32_t fit_mode;          /* IC_FIT_EXACT (default) or IC_FIT_CLOSED       */
    int32_t data_f64;          /* psrchive get_data dtype: 0 = f32
                                  (default), 1 = f64: apply_weights and the masked
                                  statistics then run in f64 (iterative_cleaner.py:
                                  111-112, 206-209): X = f64(R) * f64(w), f64 mean
                                  sum and ptp, ptp scaled in f64.  The samples must
                                  still be f32 values (the archive's amplitudes).  */
    int32_t dedisp_mode;       /* IC_DEDISP_SHIFT (default), IC_DEDISP_FFT or the
                                  opt-in IC_DEDISP_FFT_ANY                         */
    int32_t input_dedispersed; /* 1: the uploaded cube is the archive as stored
                                  DEDISPERSED (psrchive get_dedispersed()): the
                                  reference's dedisperse (:91, :100) is then a
                                  no-op and only the residual's dededisperse (:104)
                                  rotates.  IC_DEDISP_FFT(_ANY) only (with integer shifts
                                  the host rolls the cube back to the dispersed
                                  frame, which is exact); 0 otherwise.            */
} ic_params;

/* ic_params.fit_mode.
 *   IC_FIT_EXACT   scipy.optimize.leastsq(a*T - p, [1.0]) emulated bit for bit
 *                  (MINPACK lmdif, n = 1; iterative_cleaner.py:277-278): the
 *                  reference's arithmetic, zap masks identical to it.
 *   IC_FIT_CLOSED  the closed-form least-squares amplitude
 *                  a = sum_i T_i p_i / sum_i T_i^2 (f64 numpy pairwise sums; the
 *                  products T_i p_i of the dedispersed profile summed in the
 *                  stored, dispersed sample order j = (i + shift) mod nbin
 *                  since round 6; a = 0 when the template is all zero;
 *                  info = 1, or 5 (residual zeroed) when a is not finite), fused
 *                  with the residual and the diagnostics in one sweep of the raw
 *                  cube: the HBM-bound fast mode of the north star.  It is NOT
 *                  the reference's arithmetic: amplitudes differ from leastsq in
 *                  the last bits, and rarely a profile's zap decision flips. */
#define IC_FIT_EXACT 0
#define IC_FIT_CLOSED 1

/* ic_params.dedisp_mode: how dedisperse / dededisperse (iterative_cleaner.py:91,
 * :100, :104) move a channel's samples.
 *   IC_DEDISP_SHIFT  integer rotation by shift[c] bins (ded[i] = raw[(i+shift)%nbin]),
 *                    the archive stand-in's default.
 *   IC_DEDISP_FFT    psrchive's FFT phase rotation by a fractional delay
 *                    (ic_set_delays: delay[c] bins per channel; ic_set_delays2:
 *                    delay[s][c] per profile, psrchive's per-Integration folding
 *                    period): forward real FFT, harmonic k times
 *                    exp(+-2 pi i k delay / nbin), inverse real FFT, in IEEE
 *                    f32 (psrchive's precision) and the arithmetic order
 *                    written in iterative_cleaner_amd/phase_rotation.py
 *                    (bit-identical to it and to the C oracle; within 4 f32
 *                    epsilons of the profile's largest |sample| of numpy's f64
 *                    irfft(rfft(x) * phasor); parity with real psrchive
 *                    unpinned).  nbin must be a power of
 *                    two in 64..8192 (either fit_mode, f32 or f64 data,
 *                    per-channel or per-profile delays), or a mixed-radix
 *                    length: a multiple of 8 in 64..4096 whose half has only
 *                    the prime factors 2, 3 and 5 (72, 96, 120, 200, 1000, 1200,
 *                    1536, 2000, 3000, 4000, ...: IC_FIT_EXACT only, f32 or f64
 *                    data, either kind of delays; the statistics of these
 *                    lengths run in a mixed-radix diagnostics kernel of their
 *                    own, in both dedispersion modes).  Any other length, and
 *                    IC_FIT_CLOSED at a mixed-radix length, is refused with
 *                    IC_EINVAL by ic_session_create.  The shift arrays of the
 *                    uploads are then unused (pass zeros).
 *   IC_DEDISP_FFT_ANY  opt-in: IC_DEDISP_FFT in every respect (delays,
 *                    ic_set_delays / ic_set_delays2 / ic_upload_delays_async,
 *                    input_dedispersed), and at every length IC_DEDISP_FFT
 *                    serves the very same kernels and bits.  Any other nbin in
 *                    16..4096, odd and prime lengths included, is rotated by a
 *                    chirp-z (Bluestein) transform of its own written f32
 *                    order (phase_rotation.py rotate_czt, bit-identical to it;
 *                    within 5.5 f32 epsilons of the profile's largest |sample|
 *                    of numpy's f64 rotation): IC_FIT_EXACT only.  The
 *                    statistics of these lengths run in k_diag_czt (an f64
 *                    chirp-z transform for fftmax, with the diagnostics
 *                    fork) from 129 bins, odd lengths to 2048, and in the
 *                    generic direct-DFT kernel otherwise, as they do with
 *                    integer shifts.  nbin < 16, nbin > 4096
 *                    outside IC_DEDISP_FFT's set, and IC_FIT_CLOSED at a
 *                    chirp-z or mixed-radix length are refused with IC_EINVAL.
 *                    IC_DEDISP_FFT itself refuses exactly what it did. */
#define IC_DEDISP_SHIFT 0
#define IC_DEDISP_FFT 1
#define IC_DEDISP_FFT_ANY 2

/* Library / device info. */
int ic_abi_version(void);
int ic_device_count(void);

/* Session lifetime.  device: HIP ordinal. */
int ic_session_create(const ic_params *params, int device, void **session);
void ic_session_destroy(void *session);

/* Upload the cube (host pointers; one H2D copy).  Replaces the archive data
 * read by iterative_cleaner.py:97-100 (fit cube) and :88-93 (template). */
int ic_upload(void *session, const float *cube, const float *w0, const int32_t *shift);

/* Full-polarisation upload: data [nsub][npol][nchan][nbin] f32 as the archive
 * holds it (psrchive get_data), pscrunched ON THE DEVICE to the total intensity
 * f32(pol0 + pol1) (npol >= 2; npol == 1: pol0), the pscrunch of
 * iterative_cleaner.py:70/:89/:100 (archive.py pscrunch).  The host then never
 * pscrunches a copy of the archive. */
int ic_upload_pols(void *session, const float *data, int npol, const float *w0, const int32_t *shift);

/* Same from device pointers already resident in HBM on the session's device
 * (e.g. torch-ROCm tensors): a device-to-device copy, no PCIe. */
int ic_upload_device(void *session, const float *d_cube, const float *d_w0,
                     const int32_t *d_shift);

/* Batch pipelining (config C4: many archives of one shape per GPU).  Queue the
 * host->device copy of the NEXT archive on the session's copy stream and return
 * at once; the next ic_run waits for the copy and cleans that archive.  Two input
 * slots: at most two uploads may be pending, so the pattern
 *     ic_upload_async(a0); for k: { ic_upload_async(a[k+1]); ic_run(); }
 * overlaps every archive's copy with the previous archive's cleaning.  The host
 * arrays of an upload must stay untouched until the ic_run that consumes it
 * returns, and must be page-locked (ic_host_alloc) for the copy to overlap.
 * ic_upload / ic_upload_device fail with IC_ESTATE while uploads are pending.
 * Replaces the per-archive reload of iterative_cleaner.py:60 (main loop). */
int ic_upload_async(void *session, const float *cube, const float *w0, const int32_t *shift);
int ic_host_alloc(size_t bytes, void **ptr);
void ic_host_free(void *ptr);

/* Quantised uploads: the samples as a fold-mode PSRFITS archive stores them,
 * decoded on the device, so that 2 bytes per sample cross the bus instead of 4.
 *   q     [nsub][npol][nchan][nbin] int16, the DATA column (host byte order, or
 *         with IC_Q_BIG_ENDIAN in flags the FITS order: each sample's two bytes
 *         are then swapped on the device)
 *   scl,
 *   offs  [nsub][npol][nchan] f32, DAT_SCL / DAT_OFFS
 *   nsum  1: the cube is polarisation 0 (Intensity; Stokes, I = pol 0);
 *         2: pol 0 + pol 1 (AA+BB: PPQQ, Coherence); nsum <= npol
 * Only the first nsum polarisations of each subint are copied (strided copies,
 * as ic_upload_pols).  The session's cube becomes, sample for sample,
 *   d_p = f32(f32(q_p) * scl_p + offs_p)          (psrfits.py decode)
 *   nsum 1: d_0        nsum 2: f32(d_0 + d_1)     (archive.py pscrunch)
 * with the multiply, the add and the polarisation add each rounded to IEEE f32
 * on its own (no fused multiply-add): bit-identical to decoding and
 * pscrunching on the host and calling ic_upload.  w0 and shift as ic_upload; on
 * a shard session nchan is the shard's slice.  The first quantised upload into
 * an input slot allocates its staging on the device (nsum * (2 nbin + 8) bytes
 * per profile), kept for reuse until the session is destroyed; IC_ENOMEM if
 * that fails.  IC_EINVAL: a null pointer, npol < 1, nsum not 1 or 2,
 * nsum > npol, unknown flag bits, a shift outside [0, nbin).
 *
 * ic_upload_quantised is synchronous (IC_ESTATE while asynchronous uploads are
 * pending).  ic_upload_quantised_async follows ic_upload_async's rules (two
 * slots, first in first out, the page-locked host arrays untouched until the
 * consuming ic_run returns) and may be mixed with it in one queue; the decode
 * runs on the copy stream behind its copy, so it overlaps the cleaning of the
 * archive before it. */
#define IC_Q_BIG_ENDIAN 1
int ic_upload_quantised(void *session, const int16_t *q, const float *scl, const float *offs, int npol, int nsum,
                        int flags, const float *w0, const int32_t *shift);
int ic_upload_quantised_async(void *session, const int16_t *q, const float *scl, const float *offs, int npol,
                              int nsum, int flags, const float *w0, const int32_t *shift);
/* The same decode alone: out [nsub][nchan][nbin] f32 on the host.  Synchronous. */
int ic_decode_profiles(int device, int nsub, int npol, int nsum, int nchan, int nbin, const int16_t *q,
                       const float *scl, const float *offs, int flags, float *out);

/* Quantised downloads: the reverse, PSRFITS int16 samples encoded on the
 * device, so that 2 nbin + 8 bytes per profile leave the GPU instead of 4 nbin.
 * Each profile of nbin f32 samples d is encoded on its own (psrfits.py quantise),
 * every step a separate IEEE operation:
 *   mn, mx = the profile's minimum and maximum, NaN if any sample is NaN (numpy)
 *   offs   = f32(0.5 * (f64(mx) + f64(mn)))
 *   scl    = f32((f64(mx) - f64(mn)) / 65534.0); 1.0f unless scl > 0 and finite
 *   x      = (f64(d) - f64(offs)) / f64(scl)   an f64 subtraction and a true
 *            division: no fused multiply-add, no reciprocal, no f32 shortcut
 *   q      = int16(clamp(rint(x), -32767, 32767))   round half to even; a NaN x
 *            gives 0, +-inf clamp like any large value; -32768 is never produced
 * q, scl and offs carry the bits psrfits.quantise gives the same samples, with
 * one exception: numpy does not fix the sign of the minimum / maximum of zeros
 * of mixed sign, so for a profile that holds only such zeros the sign of the
 * zero offs is not pinned (its q and scl are: 0 and 1).  A NaN scl / offs
 * equals the host's as a NaN, not in sign or payload.
 *   flags  0, or IC_Q_BIG_ENDIAN: each sample's two bytes swapped on the
 *          device, the FITS order, ready for the DATA column
 *   q      [nsub][nchan][nbin] int16;  scl, offs  [nsub][nchan] f32
 * IC_EINVAL: a null pointer, unknown flag bits, a shape that is not positive
 * (checked before any device is touched).
 *
 * ic_encode_profiles: the encode alone, in [nsub][nchan][nbin] f32 on the host.
 * Synchronous.
 * ic_get_residual_quantised: the last iteration's residual, the cube
 * ic_get_residual returns (a shard: its channel slice), encoded on the device;
 * the f32 cube never reaches the host.  With integer shifts (nbin <= 8192) one
 * kernel forms each row and encodes it and no f32 cube exists at all; with
 * IC_DEDISP_FFT(_ANY) the rotated rows pass through a session-owned f32 cube.
 * IC_ESTATE before a completed iteration and on a failed session.  The first
 * call allocates the int16 / scale / offset staging on the device (2 nbin + 8
 * bytes per profile; FFT modes: the f32 cube too), kept until
 * ic_session_destroy; IC_ENOMEM if that fails.  It is
 * ic_get_residual_quantised_async followed by ic_residual_wait. */
int ic_encode_profiles(int device, int nsub, int nchan, int nbin, const float *in, int flags, int16_t *q,
                       float *scl, float *offs);
int ic_get_residual_quantised(void *session, int flags, int16_t *q, float *scl, float *offs);
/* Queue the last run's residual, encoded exactly as ic_get_residual_quantised
 * encodes it, and its download into q/scl/offs (page-locked for the copy to
 * overlap); returns when queued.  IC_ESTATE with no completed iteration.
 * The encode runs on the session's stream, the copies on a download stream of
 * the session's own (created at first use), so a following ic_run and the
 * uploads of later archives proceed while the samples travel; an asynchronous
 * upload into the input slot the encode still reads waits for the encode.
 * q/scl/offs must stay allocated, and are undefined, until ic_residual_wait
 * (or ic_session_destroy) returns.  A further call before the wait is allowed:
 * its encode waits until the earlier download has left the staging, and one
 * ic_residual_wait then covers both. */
int ic_get_residual_quantised_async(void *session, int flags, int16_t *q, float *scl, float *offs);
/* Wait until the queued residual download (if any) has landed; IC_OK when none
 * is pending.  A wait that exceeds IC_OPT_SYNC_TIMEOUT_MS fails the session. */
int ic_residual_wait(void *session);

/* Run the cleaning loop to convergence or max_iter (iterative_cleaner.py:83-146).
 * Outputs (host, any may be NULL):
 *   test_out        [nsub*nchan] f64 : avg_test_results of the last loop (:120)
 *   weights_out     [nsub*nchan] f32 : weights of the last loop (:125, :128)
 *   loops_out       [1]              : `loops` (:139, :146)
 *   changed_out     [max_iter]       : "Differences to previous weights" (:129)
 *   nzero_out       [max_iter]       : zero-weight count -> "RFI fraction" (:130)
 *   n_iter_out      [1]              : loop iterations executed
 *   converged_out   [1]              : 1 if the loop stopped on a repeated mask
 *                                      (:135-140), 0 if it hit max_iter (:143) */
int ic_run(void *session, double *test_out, float *weights_out, int32_t *loops_out,
           int32_t *changed_out, int32_t *nzero_out, int32_t *n_iter_out, int32_t *converged_out);

/* Fractional delays of the session's channels (dedisp_mode IC_DEDISP_FFT):
 * delay_bins [nchan] f64 (a shard: its nchan_loc channels), in bins, finite;
 * dedisperse moves sample j + delay to j.  Required before ic_run; kept until
 * changed. */
int ic_set_delays(void *session, const double *delay_bins);
/* The same with one delay per profile: delay_bins [nsub*nchan] f64 (a shard:
 * [nsub][nchan_loc]), profile (s, c) at s*nchan + c — psrchive dedisperses each
 * Integration with its own folding period (delay_s,c = DM delay of channel c /
 * period_s * nbin).  The phasors exp(2 pi i k delay / nbin) are then evaluated
 * per profile on the device by the same f64 formula the channel table uses, so
 * rows that are all equal give exactly ic_set_delays' results (and take its
 * table). */
int ic_set_delays2(void *session, const double *delay_bins);
/* Delays that travel with an asynchronous upload (batches of archives with
 * fractional delays: every archive has its own).  Binds delay_bins to the
 * NEWEST pending asynchronous upload, the last ic_upload_async or
 * ic_upload_quantised_async: per_profile 0 takes delay_bins [nchan] f64,
 * 1 takes [nsub*nchan] (a shard: its local channel counts), as ic_set_delays
 * and ic_set_delays2.  When ic_run consumes that upload the delays become the
 * session's, exactly as if ic_set_delays (per_profile 1: ic_set_delays2) had
 * been called with them just before that ic_run: they stay in force for
 * re-runs and synchronous uploads until a later upload with delays is consumed
 * or ic_set_delays[2] is called; an upload without attached delays leaves the
 * session's delays as they are.  Rows that are all equal give the bits of
 * per_profile 0 with that row (and take its table).
 *
 * The work is queued on the session's copy stream behind that upload's copies:
 * one host->device copy of the delays into a buffer of the upload's input slot
 * and, for per-channel delays, the kernel that builds the slot's phasor table
 * from them (the table ic_set_delays builds, by the same kernel); the upload
 * counts as arrived only after both, so all of it overlaps the cleaning of the
 * archive before.  delay_bins follows ic_upload_async's rule: untouched until
 * the consuming ic_run returns, page-locked for the copy to overlap.  The
 * slot's buffers (the table, nchan * (nbin/2 + 1) * 2 floats, and nsub * nchan
 * doubles) are allocated at first need and kept until ic_session_destroy.
 *   IC_ESTATE  the session is not IC_DEDISP_FFT(_ANY); no upload is pending; the
 *              newest pending upload already has delays; the session has failed
 *   IC_EINVAL  a null pointer; per_profile not 0 or 1; a delay that is not
 *              finite (checked on the host, at the call): nothing is queued,
 *              the upload stays pending without delays and takes them from a
 *              later call
 *   IC_ENOMEM  the slot's buffers cannot be allocated */
int ic_upload_delays_async(void *session, const double *delay_bins, int per_profile);

/* dedisperse (sign +1) or dededisperse (sign -1) a cube [nsub][nchan][nbin] f32
 * by the FFT phase rotation on the GPU (the operation IC_DEDISP_FFT applies at
 * iterative_cleaner.py:91/:100/:104).  Synchronous; in and out may alias. */
int ic_rotate_profiles(int device, int nsub, int nchan, int nbin, const float *in, const double *delay_bins,
                       int sign, float *out);
/* The same with per-profile delays delay_bins [nsub*nchan] (ic_set_delays2). */
int ic_rotate_profiles2(int device, int nsub, int nchan, int nbin, const float *in, const double *delay_bins,
                        int sign, float *out);
/* The same under IC_DEDISP_FFT_ANY's rule (opt-in): the lengths the two calls
 * above serve keep their kernels and bits, any other nbin in 16..4096 takes the
 * chirp-z rotation.  per_profile 0: delay_bins [nchan], 1: [nsub*nchan]. */
int ic_rotate_profiles_any(int device, int nsub, int nchan, int nbin, const float *in, const double *delay_bins,
                           int per_profile, int sign, float *out);

/* The last iteration's residual cube (:101-108), dispersed frame, unweighted,
 * f32 [nsub][nchan][nbin] — what --unload_res writes (:161-162). */
int ic_get_residual(void *session, float *out);

/* Profiles whose fit status was not 1-4 in each iteration of the last ic_run
 * (the reference prints "Bad status for least squares fit when removing
 * profile." once per such profile and loop, iterative_cleaner.py:284-285, and
 * zeroes its residual).  Fills up to n entries; returns the iteration count. */
int ic_get_bad_fits(void *session, int32_t *per_iter, int n);

/* Last iteration's internals for parity checks (any may be NULL):
 * template T [nbin], fit amplitude/status [P] (:278), diagnostics [P] (:206-217). */
int ic_get_template(void *session, float *T);
int ic_get_fit(void *session, double *amp, int32_t *info);
int ic_get_diagnostics(void *session, double *std_o, double *mean_o, float *ptp_o,
                       double *fftmax_o);
/* The same with ptp in f64 (the data_f64 loop's ptp is an f64 value). */
int ic_get_diagnostics_f64(void *session, double *std_o, double *mean_o, double *ptp_o,
                           double *fftmax_o);

/* Per-launch timing of the last ic_run (HIP events on the session stream):
 * fills up to n entries of {kernel id, milliseconds summed over the run,
 * launches}; returns the number of kernel ids. */
typedef struct {
    int32_t kernel;
    int32_t launches;
    double ms;
} ic_kernel_time;
int ic_get_kernel_times(void *session, ic_kernel_time *out, int n);
const char *ic_kernel_name(int kernel);
int ic_set_timing(void *session, int enabled);
/* Restrict the timing to one kernel id (ic_kernel_name ids; -1 = every kernel,
 * the default): two HIP events per launch cost ~5 us, so a timed region that
 * must stay representative times only the kernel it prices. */
int ic_set_timing_kernel(void *session, int kernel);

/* Statistics of the last ic_run (measurement; see DESIGN.md roofline). */
typedef struct {
    int32_t iterations;          /* cleaning loops executed                        */
    int32_t fit_rounds;          /* k_fit_pass launches, summed over iterations    */
    int64_t fit_profile_sweeps;  /* profiles swept by k_fit_pass, summed (x nbin x 4 B = fit bytes) */
    int64_t fit_tail_sweeps;     /* profile sweeps done by k_fit_tail (the last few thousand profiles) */
    int32_t window_moves;        /* subint baseline windows that moved between iterations */
    int32_t near_threshold;      /* last iteration: profiles whose test value lies within 1e-9 of
                                    the zap threshold 1.0, where fftmax's last bits (not
                                    bit-identical to numpy's pocketfft) could decide the zap */
    int64_t reserved0;           /* 0 (round 4's persistent-lanes counters; that schedule was
                                    removed in round 5) */
    int64_t reserved1;           /* 0 */
} ic_run_stats;
int ic_get_run_stats(void *session, ic_run_stats *out);

/* Schedule options of a session.  They choose how the work of the loop is
 * scheduled, never its arithmetic: every setting gives the same bits (the GPU
 * tests hold each schedule equal to the default and to the oracle).  Set after
 * ic_session_create; read by the following ic_run calls.  The library reads
 * no environment variables.  ic_set_option fails with IC_EINVAL for an unknown
 * option or a value out of range (given below), and on a session the option
 * cannot serve.
 *   IC_OPT_FIT_TAIL        profiles left when k_fit_tail takes over the exact
 *                          fit (one wave per profile), >= 0, 0 = never; 8192
 *                          (4096 for sessions of >= 2^20 profiles, else 12288
 *                          for nbin >= 2048)
 *   IC_OPT_DIAG_FORK       fit round after which the diagnostics of the fitted
 *                          profiles run on a second stream, 0..64, 0 = no fork;
 *                          3 (4 for nbin >= 2048 with integer dedispersion)
 *                          (exact fit only)
 *   IC_OPT_FORK_DELAY      rounds between that round and the forked pass, 0..8;
 *                          1 (2 for nbin >= 2048)
 *   IC_OPT_TEMPLATE_INCR   1 = incremental template stage (integer
 *                          dedispersion), 0 = full template passes; 1
 *   IC_OPT_FIT_TILED       1 = tiled fit cube (integer dedispersion),
 *                          0 = row-major; 1
 *   IC_OPT_ROWSTAT_WAVES   waves per row median/MAD line: 0 (one wave), 4 or 8; 8
 *   IC_OPT_ROWSTAT_MINLEN  shortest row that takes them, 1..16384; 1024
 *   IC_OPT_DIAG_CHAIN      1 = chain-layout diagnostics kernel at nbin 1024,
 *                          2048, 4096; 0 = the row-layout kernel (which every
 *                          other power of two in 64..8192 takes either way); 1
 *   IC_OPT_FIT_SCHEDULE    how the exact fit is scheduled: IC_FIT_ROUNDS (the
 *                          only value since round 5) = rounds of a sweep kernel
 *                          over every profile with a pending data request and a
 *                          state kernel, k_fit_tail for the last profiles
 *   IC_OPT_TAIL_SPLIT      with the fork: at the hand-over to k_fit_tail the
 *                          fork round's survivors already fitted are measured
 *                          on the second stream beside the tail, only the
 *                          tail's profiles after it: IC_TAIL_SPLIT_OFF, _ON, or
 *                          _AUTO (on for nbin >= 2048); IC_TAIL_SPLIT_AUTO
 *   IC_OPT_ROT_STATS       FFT dedispersion at nbin 1024 (f32 data): 1 = the
 *                          residual's inverse rotation measures its rows in the
 *                          same kernel (the rotated residual never goes to
 *                          HBM), 0 = it writes them and a statistics pass reads
 *                          them back; 1
 *   IC_OPT_GRID_CAP        a test and tuning knob: the most blocks a kernel
 *                          that walks its profiles (or samples) in a grid-stride
 *                          loop is launched with, 1..65536, 0 = the launchers'
 *                          own grids; 0.  A small cap makes a small archive take
 *                          every such loop through many trips per block.
 *   IC_OPT_SYNC_TIMEOUT_MS longest host wait for the GPU, >= 1 ms; 600000.  A
 *                          wait that runs out fails its call with IC_EHIP and
 *                          marks the session failed: every later call on it
 *                          but ic_session_destroy fails with IC_ESTATE, and
 *                          destroy then leaks its device memory (its kernels may
 *                          still be running) instead of freeing it. */
#define IC_OPT_FIT_TAIL 1
#define IC_OPT_DIAG_FORK 2
#define IC_OPT_FORK_DELAY 3
#define IC_OPT_TEMPLATE_INCR 4
#define IC_OPT_FIT_TILED 5
#define IC_OPT_ROWSTAT_WAVES 6
#define IC_OPT_ROWSTAT_MINLEN 7
#define IC_OPT_DIAG_CHAIN 8
#define IC_OPT_SYNC_TIMEOUT_MS 9
#define IC_OPT_FIT_SCHEDULE 10
/* 11, 12: IC_OPT_FIT_LANE_WAVES, IC_OPT_FIT_LATE_LANES until round 4 (removed
 * with the lanes schedule) */
#define IC_OPT_TAIL_SPLIT 13
#define IC_OPT_ROT_STATS 14
#define IC_OPT_GRID_CAP 15
#define IC_TAIL_SPLIT_OFF 0
#define IC_TAIL_SPLIT_ON 1
#define IC_TAIL_SPLIT_AUTO 2
#define IC_FIT_ROUNDS 0
int ic_set_option(void *session, int option, int64_t value);
int ic_get_option(void *session, int option, int64_t *value);
/* = ic_set_option(session, IC_OPT_FIT_TAIL, threshold) */
int ic_set_fit_tail(void *session, int64_t threshold);

const char *ic_last_error(void);

/* remove_profile1d (iterative_cleaner.py:275-288) on the GPU for nprof given
 * profiles [nprof][nbin] f32 against the template T [nbin] f32: the amplitude
 * (:278; fit_mode as ic_params.fit_mode) and status per profile, and the f32
 * residual a*T - p (zeros for a status outside 1-4, :284-286).  Outputs may be
 * NULL (not all).  Synchronous. */
int ic_fit_profiles(int device, int nprof, int nbin, const float *T, const float *profiles, int fit_mode,
                    double *amp_out, int32_t *info_out, float *resid_out);

/* comprehensive_stats (iterative_cleaner.py:181-226) alone, on the GPU, for
 * the data the reference hands it (:111-117): data [nsub][nchan][nbin] f32 and
 * weights [nsub][nchan] f32; the kernel forms X = f32(data * w), masked where
 * w == 0, computes the four diagnostics (:206-217), their channel / subint
 * median-MAD scaling (:219-224) and test [nsub*nchan] f64 = the median of the
 * four (:225).  std/mean/ptp/fftmax outputs may be NULL.  Synchronous. */
int ic_comprehensive_stats(int device, int nsub, int nchan, int nbin, const float *data, const float *weights,
                           double chanthresh, double subintthresh, double *test_out, double *std_out,
                           double *mean_out, float *ptp_out, double *fftmax_out);
/* The same with the row-median form of IC_OPT_ROWSTAT_WAVES / _MINLEN. */
int ic_comprehensive_stats_rowstat(int device, int nsub, int nchan, int nbin, const float *data,
                                   const float *weights, double chanthresh, double subintthresh, double *test_out,
                                   double *std_out, double *mean_out, float *ptp_out, double *fftmax_out,
                                   int rowstat_waves, int rowstat_minlen);

/* ------------------------------------------------------------------------
 * Detrended scaling (opt-in; the definition is iterative_cleaner_amd/detrend.py).
 * Before a diagnostic is scaled by its channel's (a line over the subints) or
 * its subint's (a line over the channels) median and MAD, a polynomial trend of
 * the line is removed: abscissa x_j = (2j - (n-1)) / (n-1), order chan_order /
 * subint_order in 0..3 (0: that direction is not detrended), normal equations
 * over the line's members summed as 64 chains and a halving tree, solved by
 * elimination without pivoting, up to `rounds` (1..8) fits, each but the last
 * followed by a clip of the members to |e - median(e)| <= clip * MAD(e) (clip a
 * finite value > 0) of the residuals e; a line with a non-finite valid value,
 * with no more members than the order, or with a refused pivot keeps a zero
 * trend.  The scalers then run on d' = dtype(f64(d) - p(x)) as they run on d.
 * The reference has no such step; it is modelled on coast_guard's
 * iterative_detrend, and parity with coast_guard is UNPINNED (not available):
 * detrend.py is the pin, and the kernels follow it bit for bit.
 *
 * ic_set_detrend: after create; holds for the ic_runs that follow; (0, 0, ..)
 * switches it off, and a session on which it is off or was never called
 * launches and computes exactly what it always did.  IC_EINVAL for a value out
 * of range and on a channel-shard session that has not opted in
 * (ic_shard_enable_detrend, below).  It is no ic_set_option option: those
 * never change the arithmetic.
 * ic_get_trends: the last iteration's coefficients a_0..a_3 per line,
 * chan_coef [4][nchan][4] and subint_coef [4][nsub][4] (diagnostics in the
 * order std, mean, ptp, fftmax); either may be NULL.  IC_ESTATE before a
 * completed iteration or while detrending is off.
 * ic_comprehensive_stats_detrend: ic_comprehensive_stats with the detrended
 * scaling; data_f64 as ic_params.data_f64 (ptp_out is f64: f32 values unless
 * data_f64); chan_coef / subint_coef as ic_get_trends, may be NULL. */
int ic_set_detrend(void *session, int chan_order, int subint_order, int rounds, double clip);
int ic_get_trends(void *session, double *chan_coef, double *subint_coef);
int ic_comprehensive_stats_detrend(int device, int nsub, int nchan, int nbin, const float *data, const float *weights,
                                   double chanthresh, double subintthresh, double *test_out, double *std_out,
                                   double *mean_out, double *ptp_out, double *fftmax_out, int data_f64,
                                   int chan_order, int subint_order, int rounds, double clip, double *chan_coef,
                                   double *subint_coef);

/* ------------------------------------------------------------------------
 * Piecewise detrending (opt-in, on top of the detrended scaling; the definition
 * is the piecewise part of iterative_cleaner_amd/detrend.py).  The lines of a
 * direction are cut into pieces at strictly ascending starts b_0 = 0 < b_1 < ..
 * < b_{m-1} < n (1 <= m <= 512; piece q is [b_q, b_{q+1}), the last one ends
 * at n), the same for every line and diagnostic of that direction.  Every
 * piece has its own abscissa x = (2i - (L-1)) / (L-1) over its local index i
 * and length L (L == 1: 0) and is fitted on its own, from its own members, with
 * the sums, the elimination and the order of the whole-line fit.  A piece with
 * no more members than the order, or with a refused pivot, is retired: its
 * coefficients are +0.0 from that round on, and the other pieces go on.  The
 * members, the residuals' median and MAD, the clip and the stop rules stay
 * those of the whole line; a line with a non-finite valid value keeps a zero
 * trend in every piece.  d' of an entry uses its own piece's polynomial.  The
 * entries of a retired piece therefore meet the scaler undetrended (a subband
 * with too few live channels is likely to be zapped); no lower order is tried.
 * With one piece per direction every output equals the whole-line form's bit
 * for bit.  Modelled on coast_guard's breakpoints / numpieces (its detrend's
 * `bp` and `numpieces`, the surgical cleaner's chan_/subint_breakpoints and
 * _numpieces), stated from memory: parity with coast_guard is UNPINNED.
 *
 * ic_set_detrend_pieces: after create, in any order with ic_set_detrend; holds
 * for the ic_runs that follow.  chan_*: the channel lines (over the subints,
 * n = nsub); subint_*: the subint lines (over the channels, n = the session's
 * nchan).  npieces == 0 with a NULL pointer: one piece in that direction.  A
 * call with a direction non-zero selects the piecewise kernels for detrended
 * runs (with one piece each as well); (0, NULL, 0, NULL) goes back to the
 * whole-line kernels.  While detrending is off, pieces change nothing.
 * IC_EINVAL: starts[0] != 0, starts not strictly ascending, a start >= n,
 * npieces outside 0..512, a NULL pointer with npieces > 0, a channel-shard
 * session that has not opted in (ic_shard_enable_detrend; there n of the
 * subint lines is the archive's nchan, not the shard's).  IC_ENOMEM (from the
 * run) when the pieces' buffers cannot be had.
 * ic_get_trends_pieces: chan_coef [4][nchan][mc][4], subint_coef
 * [4][nsub][ms][4] (mc, ms: the directions' piece counts); either may be NULL.
 * IC_ESTATE as ic_get_trends, and when no pieces are set.  ic_get_trends
 * itself returns IC_ESTATE while a direction has more than one piece.
 * ic_comprehensive_stats_detrend_pieces: ic_comprehensive_stats_detrend with
 * pieces (always the piecewise kernels); the coefficient outputs as
 * ic_get_trends_pieces. */
int ic_set_detrend_pieces(void *session, int chan_npieces, const int32_t *chan_starts, int subint_npieces,
                          const int32_t *subint_starts);
int ic_get_trends_pieces(void *session, double *chan_coef, double *subint_coef);
int ic_comprehensive_stats_detrend_pieces(int device, int nsub, int nchan, int nbin, const float *data,
                                          const float *weights, double chanthresh, double subintthresh,
                                          double *test_out, double *std_out, double *mean_out, double *ptp_out,
                                          double *fftmax_out, int data_f64, int chan_order, int subint_order,
                                          int rounds, double clip, double *chan_coef, double *subint_coef,
                                          int chan_npieces, const int32_t *chan_starts, int subint_npieces,
                                          const int32_t *subint_starts);

/* ------------------------------------------------------------------------
 * Detrended scaling on channel shards (opt-in on top of the two above; the
 * shard sessions are described below).  A channel line lies whole on its
 * shard; a subint line is fitted by the row's owner, which already holds the
 * whole row, and every iteration then all-gathers one slot per rank with the
 * owned rows' median, MAD and coefficients: rows_pad * (8 + 16 ms) doubles,
 * rows_pad = ceil(nsub / world), ms = the subint pieces (1 when unpieced).
 * 1024 subints on 8 ranks with 512 pieces: 8.4 MB per slot, 67 MB gathered on
 * every rank.  The result equals the unsharded detrended clean bit for bit.
 *
 * ic_shard_enable_detrend: on a shard session, ic_set_detrend,
 * ic_set_detrend_pieces, ic_get_trends and ic_get_trends_pieces are legal from
 * then on; on an unsharded session IC_OK and nothing else.  EVERY rank of a
 * group must call it and then set the same orders, rounds, clip and pieces:
 * ranks that disagree exchange different sizes (the transport fails, or
 * blocks until its timeout).  The library issues no exchange of its own to
 * check the agreement, so a shard run without detrending issues exactly the
 * exchanges it always did.
 * ic_set_detrend_pieces on such a session: subint_starts are the starts of the
 * archive's whole subint lines (validated against the archive's nchan, and the
 * same on every rank); chan_starts against nsub as ever.
 * ic_get_trends[_pieces] on such a session: chan_coef holds the shard's own
 * channels, [4][nchan_r][mc][4]; subint_coef all nsub rows, [4][nsub][ms][4],
 * identical on every rank.
 * The slots are exchange buffers: with ic_comm_ops the host's alloc / release
 * are called from the first detrended ic_run after enabling (and after a change
 * of pieces), not only from the create call. */
int ic_shard_enable_detrend(void *session);

/* ------------------------------------------------------------------------
 * Standard template (opt-in): clean against a supplied profile of the pulsar
 * instead of the template the loop builds from the archive itself.  The written
 * definition is iterative_cleaner_amd/std_template.py, which the kernels
 * (k_std_ccf, k_std_peak, k_std_install) follow bit for bit; the ABI version
 * stays 9 (additions only).
 *
 * ic_set_std_template: T [nbin] f32 is the standard, used as given (no x10000,
 * no normalisation: the fit's amplitude absorbs the scale); align is how it is
 * brought onto the archive's pulse phase in every run:
 *   IC_ALIGN_NONE  as given (no cross-correlation is made);
 *   IC_ALIGN_INT   rolled by the lag of the cross-correlation peak with the
 *                  archive's own first template (the original samples, exact);
 *   IC_ALIGN_FRAC  rotated by lag + the parabola's sub-bin part, by the FFT
 *                  phase rotation of ic_rotate_profiles2; only at the lengths
 *                  that rotation serves (IC_EINVAL elsewhere, naming IC_ALIGN_INT).
 * T == NULL clears it: the session is back to the iterative template, bit for
 * bit.  IC_EINVAL: nbin != the session's, nbin < 4, a non-finite value, a
 * constant profile, an unknown align.  The standard is kept across uploads (a
 * batch lane sets it once); the alignment is redone for every archive, on the
 * session's stream, with no host read.  A failed alignment (a non-finite
 * correlation, e.g. from a NaN sample in the archive, no positive peak, or a
 * trough deeper than the peak: an anti-correlated standard) is not an error of
 * the run: the standard is then used as given and aligned = 0
 * is reported.
 * ic_run with a standard set is ONE pass: nothing in an iteration depends on
 * the previous mask, so if iteration 1 changes the weights and max_iter >= 2,
 * iteration 2 is reported without being launched (loops = 2, converged = 1,
 * changed[1] = 0, nzero[1] = nzero[0], the same bad-fit count); an unchanged
 * mask ends with loops = 1 and max_iter = 1 with loops = 1, not converged, as
 * ever.  ic_get_template then returns the template in use: the aligned
 * standard.  Every other mode (closed-form fit, data_f64, both dedispersion
 * modes, detrended scaling, quantised uploads, residuals) is unchanged.
 * On channel shards every rank must set the same standard and mode; each rank
 * aligns for itself against the same scrunched template and gets the same
 * bits, the result equals one GPU's.  Ranks that disagree are detected: the
 * counters' all-reduce of every shard run carries two more words, a hash of
 * the standard and mode, or zeros where none is set, and ic_run fails with
 * IC_EINVAL on a rank whose words differ from the sum's share (different
 * standards, different modes, or a standard on only some ranks).
 * ic_get_std_alignment: the last run's aligned (0 / 1), lag (bins) and shift
 * (bins, lag + sub-bin part; IC_ALIGN_INT reports it too); any may be NULL;
 * all zero with IC_ALIGN_NONE.  IC_ESTATE without a standard or before a run.
 * ic_align_template: a one-shot of the same kernels: S the standard, A the
 * template to align against, out [nbin] the template the loop would install. */
#define IC_ALIGN_NONE 0
#define IC_ALIGN_INT 1
#define IC_ALIGN_FRAC 2
int ic_set_std_template(void *session, const float *T, int nbin, int align);
int ic_get_std_alignment(void *session, int32_t *aligned, int32_t *lag, double *shift);
int ic_align_template(int device, int nbin, const float *S, const float *A, int align, float *out, int32_t *aligned,
                      int32_t *lag, double *shift);

/* Opt-in hot-bin repair (iterative_cleaner_amd/hotbins.py is the written
 * definition; k_hotbins follows it bit for bit).  Before the loop reads an
 * uploaded cube, every profile's off-pulse bins are clipped against their
 * median and MAD (up to `rounds` rounds) and the few bins that stand out are
 * set to the median of the bins that stay, so that an impulsive interferer in
 * two or three bins no longer costs the whole profile.  The on-pulse window
 * [on_start, on_end) is given in the dedispersed frame (0 <= on_start < nbin,
 * 0 <= on_end <= nbin; on_end <= on_start wraps; its length is (on_end -
 * on_start) mod nbin, so equal ends, and also (0, nbin), mean no window, never
 * the whole profile); a
 * stored bin j of channel c is on-pulse iff (j - o) mod nbin lies in it, o =
 * shift[c], 0 with input_dedispersed, or rint(delay) mod nbin with fractional
 * delays (the window then one bin wider on each side).  Fewer than 8 off-pulse
 * bins are refused.  Profiles with w0 == 0 or a non-finite off-pulse sample are
 * left alone (count 0); a profile with more than |O| / 4 hot bins is left to
 * the surgical cleaner (count -1).  On-pulse bins are neither read nor written.
 * ic_set_hotbins: threshold (finite, > 0; in scaled MADs) switches it on for
 * the uploads consumed from here on, threshold <= 0 switches it off (the other
 * arguments are then ignored); rounds 1..8.  Switched on after a run has
 * already read the current upload, it leaves that upload alone and starts with
 * the next one.  It changes arithmetic, so it is
 * no ic_set_option option.  Off, a session launches and computes exactly what
 * it did without it.  The pass runs once per upload, on the session stream at
 * the start of the first ic_run that consumes it; a later ic_run of the same
 * upload reads the repaired cube and keeps the counts and the list.  Channel
 * shards treat their own slices; nothing is exchanged.
 * ic_get_hotbins: count [P] (bins repaired, 0, or -1 = over the cap) and / or
 * total (the sum of the positive counts); either may be NULL.
 * ic_get_hotbin_list: the repaired bins in CSR layout: the positive counts are
 * the row lengths, profiles ascending, bins ascending within a profile.
 * Both: IC_ESTATE while the feature is off or before a run consumed an upload
 * with it on; the list: IC_EINVAL if cap < total.
 * ic_hotbins_profiles: a one-shot of the same kernels on nprof profiles: in
 * [nprof][nbin], w [nprof], offsets [nprof] (o of each profile, any integer;
 * NULL = 0), widen 0 / 1; out [nprof][nbin] (may be NULL), count [nprof], bins
 * [cap] (may be NULL with cap 0), *total always written; IC_EINVAL if bins is
 * given and cap < total (out and count are then still valid). */
int ic_set_hotbins(void *session, double threshold, int on_start, int on_end, int rounds);
int ic_get_hotbins(void *session, int32_t *count, int64_t *total);
int ic_get_hotbin_list(void *session, int32_t *bins, int64_t cap);
int ic_hotbins_profiles(int device, int nprof, int nbin, const float *in, const float *w, const int32_t *offsets,
                        int widen, double threshold, int on_start, int on_end, int rounds, float *out,
                        int32_t *count, int32_t *bins, int64_t cap, int64_t *total);

/* Opt-in dynamic spectrum (iterative_cleaner_amd/dynspec.py is the written
 * definition; k_dynspec follows it bit for bit): the pulsar's flux and its
 * uncertainty per (subint, channel) by a template fit with a free baseline, as
 * psrchive's psrflux takes it from a cleaned archive (that parity is not
 * pinned).  Per profile the inputs are the dedispersed f32 samples x of the
 * cube the last ic_run consumed (raw gathered by the integer shifts; rot(raw)
 * with the FFT dedispersion modes; an input stored dedispersed as it is;
 * hot-bin-repaired where that mode is on), the template T as ic_get_template
 * returns it and the last iteration's weight w.  No baseline is removed first
 * and the pulse region plays no part.  With t = f64(T) - mean(T) and Stt = sum
 * t^2:  amp = sum(t x) / Stt,  base = mean(x) - amp mean(T),  err = sqrt(sum(((x
 * - mean(x)) - amp t)^2) / (nbin - 2)) / sqrt(Stt); every sum in f64 in the one
 * order dynspec.py writes down (64 chains, then a halving tree), no fused
 * operations.  A profile with w == 0 gets amp = err = base = +0.0 and its
 * samples are never read; non-finite samples and a constant template are not
 * special-cased.
 * ic_get_dynspec: synchronous; amp / err / base [nsub * nchan] each, any may be
 * NULL.  IC_ESTATE before a completed iteration and on a failed session;
 * IC_EINVAL for nbin < 4.  It serves every mode ic_run serves, may be called
 * repeatedly, and launches nothing during ic_run: a session that never calls it
 * launches and computes exactly what it did without it.  Its scratch (3
 * doubles per profile and nbin + 2) is allocated at the first call and kept
 * until ic_session_destroy.  On a channel shard it returns the shard's [nsub]
 * [nchan_loc] slice; nothing is exchanged (the template is the same on every
 * rank).  Its kernel is timed as "k_dynspec" (ic_get_kernel_times).
 * ic_dynspec_profiles: a one-shot of the same kernels on nprof dedispersed
 * profiles [nprof][nbin] with the template T [nbin] and weights w [nprof];
 * 4 <= nbin <= 32768. */
int ic_get_dynspec(void *session, double *amp, double *err, double *base);
int ic_dynspec_profiles(int device, int nprof, int nbin, const float *T, const float *profiles, const float *w,
                        double *amp, double *err, double *base);

/* ------------------------------------------------------------------------
 * Channel-sharded cleaning of ONE archive across `world` shards (config C3,
 * SURVEY.md §8(e)).  The reference cleans an archive in one process
 * (iterative_cleaner.py:83-146); these entry points split the same loop by
 * channel blocks.  Rank r owns the channels of one node of the canonical
 * super-block tree (archive.py sb_tree / shards.py channel_shards) and the
 * subint rows [r*nsub/world, (r+1)*nsub/world) of the row medians.  Per
 * iteration a shard exchanges: the template's per-subint channel-sum roots,
 * each row sent to its row owner (two all-to-alls, nsub*nbin f64 out per rank),
 * the owners' windows and fscrunch rows (two small all-gathers), its
 * diagnostics rows with the row owners (one all-to-all), the row medians/MADs
 * (one all-gather of 8*rows doubles) and the convergence counters (one
 * all-reduce).  Results are bit-identical to an
 * unsharded session.  world must be a power of two <= the number of 256-channel
 * super-blocks.
 *
 * A shard session takes the GLOBAL shape in ic_params; ic_upload /
 * ic_upload_device take the shard's channel slice: cube [nsub][nchan_loc][nbin],
 * w0 [nsub][nchan_loc], shift [nchan_loc]; per-profile outputs of ic_run and
 * the ic_get_* calls are the shard's [nsub][nchan_loc] slice, while loops,
 * changed and nzero are global.  Every shard of a group must call ic_run
 * together (collectives inside).
 * ------------------------------------------------------------------------ */

/* Channel ranges [chan_ranges[2r], chan_ranges[2r+1]) and row ranges of every
 * rank (arrays of 2*world int32). */
int ic_shard_layout(int nsub, int nchan, int world, int32_t *chan_ranges, int32_t *row_ranges);

/* Host-provided transport (one process per GPU; e.g. torch.distributed over
 * RCCL/xGMI).  All exchange buffers are obtained through alloc() so that the
 * host owns them.  Collectives are issued in stream order on `stream` (the
 * session's hipStream_t) and return 0 on success.
 *   allgather:  recv[r*bytes .. (r+1)*bytes) = rank r's send, every r
 *   alltoallv:  send = blocks for ranks 0..world-1 (send_bytes[r] each, back to
 *               back); recv = blocks from ranks 0..world-1 (recv_bytes[r])
 *   allreduce_sum_i32: in place */
typedef struct {
    void *ctx;
    int (*alloc)(void *ctx, size_t bytes, void **dev_ptr);
    int (*release)(void *ctx, void *dev_ptr);
    int (*allgather)(void *ctx, const void *send, void *recv, size_t bytes, void *stream);
    int (*alltoallv)(void *ctx, const void *send, const size_t *send_bytes, void *recv,
                     const size_t *recv_bytes, void *stream);
    int (*allreduce_sum_i32)(void *ctx, int32_t *buf, size_t n, void *stream);
} ic_comm_ops;

/* Shard `rank` of `world` on HIP device `device`, exchanging through `ops`
 * (copied; ops->ctx must outlive the session). */
int ic_session_create_shard(const ic_params *params, int device, int rank, int world, const ic_comm_ops *ops,
                            void **session);

/* Native RCCL transport (one process per GPU, RCCL over xGMI): rank 0 calls
 * ic_rccl_unique_id and the host hands the 128 id bytes to every rank once
 * (e.g. through the torch.distributed store); each rank then creates its shard
 * with them on its own device.  Every exchange is an RCCL collective (all-to-all
 * as grouped sends / receives) issued by the library on the session stream: no
 * host callback per exchange.  A failing shard aborts its communicator and
 * returns its error; a peer learns of it from RCCL (an error from its own
 * collective, or RCCL's asynchronous error while the library waits on the
 * GPU: IC_ECOMM), or at worst from IC_OPT_SYNC_TIMEOUT_MS (IC_EHIP).
 * The communicator is created non-blocking and polled: a rank that never
 * joins (it failed before ic_session_create_rccl) makes its peers' creation
 * fail with IC_ECOMM after the init timeout instead of blocking them forever.
 * librccl is loaded on first use (/opt/rocm/lib/librccl.so.1); IC_ECOMM if it
 * is missing. */
int ic_rccl_unique_id(void *id_out /* 128 bytes */);
int ic_session_create_rccl(const ic_params *params, int device, int rank, int world, const void *unique_id,
                           void **session);
/* The librccl file to load instead of the ROCm install's (another RCCL build,
 * or a test stub exporting the same nccl* symbols); NULL restores the
 * default.  Process-wide; must precede the first RCCL use of the process
 * (IC_ESTATE after it, unless the path is the one already loaded). */
int ic_rccl_set_library(const char *path);
/* How long ic_session_create_rccl waits for every rank to join, in ms (>= 1;
 * process-wide; default 600000). */
int ic_rccl_set_init_timeout(int64_t ms);

/* In-process shard group: `world` shards driven by `world` host threads of one
 * process (one or several devices), exchanging by device-to-device / peer
 * copies.  Destroy the group after all its sessions; a session that a host's
 * error path destroys after its group is still destroyed safely (the group's
 * memory lives until its last session is gone), but no session may be created
 * on, or run with, a destroyed group. */
int ic_group_create(int world, void **group);
void ic_group_destroy(void *group);
int ic_session_create_grouped(const ic_params *params, int device, void *group, int rank, void **session);

#ifdef __cplusplus
}
#endif
#endif /* ITERATIVE_CLEANER_H */
