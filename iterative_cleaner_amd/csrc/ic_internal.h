// ic_internal.h — shared declarations between the host session (ic_session.hip)
// and the gfx950 kernel units (ic_template.hip, ic_codec.hip, ic_fit.hip,
// ic_diag.hip, ic_rotate.hip, ic_linestats.hip, ic_shards.hip, ic_stdtemplate.hip,
// ic_hotbins.hip, ic_dynspec.hip).
// Not part of the public C-ABI.
#pragma once
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace icgpu {

// Kernel timing on the dispatch packet itself.  The session's LAUNCH macro
// parks a start/stop event pair here; the first IC_GGL of the launch wrapper
// it calls dispatches through hipExtLaunchKernelGGL, whose packet records
// both timestamps, so a timed kernel costs no extra marker packets (C2, the
// bench's timed region with k_fit_pass timed: 27.74 ms per clean with a
// hipEventRecord pair around each launch, 27.62 with the packet's own).
// Further kernels of the same wrapper are counted in `extra`; the session
// then ends the interval with a marker after the wrapper.
struct PendingTiming {
    hipEvent_t a = nullptr, b = nullptr;
    int used = 0, extra = 0;
};
extern thread_local PendingTiming g_timing;
#define IC_GGL(K, GRID, BLOCK, SHM, ST, ...)                                                                 \
    do {                                                                                                    \
        if (::icgpu::g_timing.a && !::icgpu::g_timing.used) {                                               \
            ::icgpu::g_timing.used = 1;                                                                     \
            hipExtLaunchKernelGGL(K, GRID, BLOCK, SHM, ST, ::icgpu::g_timing.a, ::icgpu::g_timing.b, 0,      \
                                  __VA_ARGS__);                                                             \
        } else {                                                                                            \
            if (::icgpu::g_timing.a) ++::icgpu::g_timing.extra;                                             \
            hipLaunchKernelGGL(K, GRID, BLOCK, SHM, ST, __VA_ARGS__);                                       \
        }                                                                                                   \
    } while (0)

constexpr int kSuperBlock = 256;    // canonical channel super-block (archive.py SUPER_BLOCK)
inline int super_blocks(int nchan) { return (nchan + kSuperBlock - 1) / kSuperBlock; }
constexpr int kMaxLeaves = 256;     // pairwise-sum leaves (nbin <= 32768)
constexpr int kFitTile = 32;        // bins per k_fit_pass LDS tile (fit cube row padding)
constexpr size_t kLdsBlockMax = 160 * 1024;   // dynamic LDS one block may ask for: all of a gfx950 CU's
constexpr size_t kLdsBudget = 150 * 1024;     // launchers shrink groups per block to fit this: the static LDS (k_diag's PwPlan) comes on top

// Tiled fit cube (dtiled): profiles in groups of 64 (one k_fit_pass wave),
// each group stored as ldD/32 tiles of [64 profiles][32 bins] (8 KiB), so a
// wave's 32-bin step of its 64 rows is one contiguous 8-KiB block instead of
// 64 lines 4 KiB apart.  Element (k, i) of a cube with row length ldD
// (a multiple of 32, profiles padded to a multiple of 64):
__host__ __device__ inline size_t dt_ofs(size_t k, int i, int ldD)
{
    return (((k >> 6) * (size_t)(ldD >> 5) + (size_t)(i >> 5)) << 11) + ((k & 63) << 5) + (size_t)(i & 31);
}
// element (k, i) of the fit cube in either layout
__host__ __device__ inline size_t d_ofs(size_t k, int i, int ldD, int dtiled)
{
    return dtiled ? dt_ofs(k, i, ldD) : k * (size_t)ldD + (size_t)i;
}

// Canonical combine of super-block partials (archive.py sb_tree): the halving
// tree over n leaves, evaluated as a post-order stack program: push leaf j,
// then merge the two top entries merges[j] times.  n <= kMaxSbLeaves (nchan <=
// 16384); the stack never holds more than 1 + log2(n) <= 7 entries.
constexpr int kMaxSbLeaves = 64;
struct SbPlan {
    int32_t n;
    uint8_t merges[kMaxSbLeaves];
};

// Row/column geometry of a channel shard's exchanges (world <= kMaxShards):
// rank r owns channels [chan0[r], chan0[r+1]) and subint rows [row0[r], row0[r+1]).
constexpr int kMaxShards = 64;
struct ShardGeom {
    int32_t world, rank, nsub, nchan_g;
    int32_t chan0[kMaxShards + 1];
    int32_t row0[kMaxShards + 1];
};

// bytes of one exchange block of n elements of esz bytes (32 = std+mean+fft+ptp),
// padded so that every block, and the f64 fields inside it, start 8-aligned
__host__ __device__ inline size_t shard_block_bytes(size_t n, size_t esz) { return ((n * esz + 7) / 8) * 8; }

// numpy pairwise-summation plan for one nbin (numpy loops_utils.h.src order):
// leaves in address order, then a post-order list of internal adds.
struct PwPlan {
    int32_t n;
    int32_t nleaf;
    int32_t nops;
    int32_t root;                   // slot of the final value
    int32_t leaf_start[kMaxLeaves];
    int32_t leaf_len[kMaxLeaves];
    int32_t op_a[kMaxLeaves];       // slot ids; slot nleaf+o is the o-th op result
    int32_t op_b[kMaxLeaves];
};

enum KernelId {
    K_CHAN_PARTIALS = 0,
    K_WINDOW,
    K_BASE,
    K_FSCRUNCH,
    K_TSCRUNCH,
    K_FIT_PASS,
    K_FIT_STATE,
    K_DIAG,
    K_LINESTATS,
    K_COMBINE,
    K_RESIDUAL,
    K_FIT_TAIL,
    K_SB_TREE,
    K_SHARD_PACK,     // pack / assemble / unpack of shard exchanges
    K_EXCHANGE,       // the collectives themselves (host transport or peer copies)
    K_TNORM,          // fit_mode 1: sum(T*T)
    K_ROTATE,         // fractional dedispersion (FFT phase rotation)
    K_RESIDUAL_Q,     // the residual formed and encoded to int16 in one pass
    K_STD_ALIGN,      // standard template: k_std_ccf and k_std_peak
    K_STD_INSTALL,    // standard template: k_std_install
    K_HOTBINS,        // hot-bin repair: k_hotbins
    K_HOTBIN_SCAN,    // ... and the row starts of its hit list: k_hotbin_scan
    K_DYNSPEC,        // dynamic spectrum (ic_get_dynspec): k_dynspec
    K_COUNT
};

// lmdif per-profile state (structure of arrays, device memory)
struct FitStateArrays {
    double *x, *fnorm, *par, *delta, *diag, *xnorm, *acnorm, *J0, *f0, *aj, *r, *Jn0, *qtf, *gnorm,
        *x2, *pnorm, *wa1, *xa;
    int32_t *iter, *nfev, *mode, *slow;
    // sweep outputs (k_fit_pass -> k_fit_state): the norms carry the flags in
    // their sign bits (fnorm: the A sweep took the exact path; acnorm: J(1) ==
    // T in round 0), o_sum the dot of a B sweep (or round 0's fused one).
    // The two norms are stored as one double2 (fnorm, acnorm) per profile,
    // ((double2 *)o_fnorm)[k], over the o_fnorm and o_acnorm arrays (adjacent,
    // 2 x 8P bytes): one 16-B store per A sweep
    double *o_fnorm, *o_acnorm, *o_sum;
    float *p0;            // first sample of every profile's fit-cube row (round 0)
    const double *T64;    // the iteration's template (k_fit_state recomputes f0 / J0 from it)
    // the first outer iteration's profile-independent qrfac (k_fit_prep): U = {valid, acnorm, aj, Jn0}
    double *U;
};

struct LineStatsArgs {
    int nsub, nchan;
    const uint8_t *valid;
    const double *std_d, *mean_d, *fft_d;
    const double *ptp_d;            // ptp (f32 values unless data_f64)
    int ptp_f32;                    // 1: ptp lines use f32 arithmetic (numpy.ma on f32 data)
    double *col_med, *col_mad;      // [4][nchan]
    double *row_med, *row_mad;      // [4][nsub]
    // row-median form (session options IC_OPT_ROWSTAT_WAVES / _MINLEN, checked
    // when set): grp_waves waves per line (0 = one wave per line, 4 or 8) for
    // rows of >= grp_minlen values
    int grp_waves = 8, grp_minlen = 1024;
};

// Detrended scaling (ic_set_detrend; detrend.py): the orders of the two
// directions, the clipping rounds, and the lines' coefficients
struct TrendArgs {
    int chan_order, subint_order, rounds;
    double clip;
    double *col_coef;   // [4][nchan][4]
    double *row_coef;   // [4][nsub][4]
};

// Piecewise detrending (ic_set_detrend_pieces; detrend.py): a direction's lines
// are cut at the same starts, and every piece is fitted on its own abscissa.
// With pieces the coefficient arrays of TrendArgs are [4][nchan][col_np][4] and
// [4][nsub][row_np][4].  "col": the channel lines (over the subints, n = nsub);
// "row": the subint lines (over the channels, n = nchan).
constexpr int kMaxPieces = 512;   // the pieces' coefficients live in LDS: 512 x 32 B
struct PieceArgs {
    int col_np, row_np;                       // pieces per line, 1..kMaxPieces
    const int32_t *col_starts, *row_starts;   // [np + 1]: the starts, then n
    const int16_t *col_piece, *row_piece;     // [nsub], [nchan]: the piece of an entry
};

// Grid cap (session option IC_OPT_GRID_CAP): the launchers whose grid is
// min(blocks the work needs, a constant) launch min(that, grid_cap) blocks when
// grid_cap > 0, so that a small archive drives every grid-stride loop through
// many trips.  0 = the grids as they are.
inline unsigned cap_grid(size_t grid, int grid_cap)
{
    return (unsigned)(grid_cap > 0 && grid > (size_t)grid_cap ? (size_t)grid_cap : grid);
}
// the launchers' ceiling division, and the block size of the lane-per-bin
// kernels: whole waves, at most 256 threads
inline unsigned cdiv(size_t a, size_t b) { return (unsigned)((a + b - 1) / b); }
inline int bin_block(int nbin) { return nbin >= 256 ? 256 : ((nbin + 63) / 64) * 64; }

// ---- launch wrappers (each below its kernels, in the unit of its stage); all
// asynchronous on `st` ----
// valid[k] = (w0[k] != 0), W[k] = hist0[k] = w0[k]: once per run (k_valid)
hipError_t launch_valid(hipStream_t st, const float *w0, uint8_t *valid, float *W, float *hist0, size_t P);
// mode 0: part = sum W*ded; 1: part2 = sum W*f32(ded-base) + wpart; 2: both;
// 3: mode 1 + the fit cube D[k][i] = f32(ded-base) (row stride ldD).
// flags: only subints with flags[s] != 0 (nullptr: all)
hipError_t launch_chan_partials(hipStream_t st, int mode, const float *raw, const float *W, const int32_t *shift,
                                const float *base, const int32_t *flags, int nsub, int nchan, int nbin,
                                double *part, double *part2, double *wpart, float *D = nullptr, int ldD = 0,
                                int dtiled = 0, uint8_t *exA = nullptr, uint8_t *exF = nullptr);
// exA / exF (optional): per column [s][sb][i] 1 = its part / part2 sum is
// exact in any order with weights 0 / 1 (k_chan_partials' ExTrack), the
// condition for launch_chan_delta.  Iteration >= 2 (Wn = this iteration's weights, Wo = the
// previous one's): part, part2 (carried levels) and wpart moved from Wo to Wn
// through the changed channels only; inexact columns summed again in full.
// rawF (FFT dedispersion): part2's terms are f32(rawF - base) instead of
// f32(raw - base) (part's stay raw's).
hipError_t launch_chan_delta(hipStream_t st, const float *raw, const int32_t *shift, const float *base,
                             const float *Wn, const float *Wo, int nsub, int nchan, int nbin, double *part,
                             double *part2, double *wpart, const uint8_t *exA, const uint8_t *exF,
                             const float *rawF = nullptr);
// flags != nullptr: flags[s] = window of subint s moved (win updated in place)
// element (s, leaf, i) of `part` is part[s*ss + leaf*sl + i]; the leaves are
// combined with `plan` (single device: the nsb super-blocks; sharded: the
// gathered shard roots)
hipError_t launch_window(hipStream_t st, const double *part, long ss, long sl, const SbPlan &plan, int nsub,
                         int nbin, int width, int32_t *win, int32_t *flags);
// dynamic LDS of k_window (nbin doubles + per-thread partials)
size_t window_lds_bytes(int nbin);
// flags != nullptr: only subints with flags[s] != 0
hipError_t launch_base(hipStream_t st, const float *raw, const int32_t *shift, const int32_t *win,
                       const int32_t *flags, int nsub, int nchan, int nbin, int width, float *base, int grid_cap = 0);
// total intensity in place: raw[i] = f32(raw[i] + pol1[i])  (archive.py pscrunch)
hipError_t launch_pscrunch(hipStream_t st, float *raw, const float *pol1, size_t n, int grid_cap = 0);
// PSRFITS int16 samples q [nsub][nsum][nchan][nbin] (big_endian: as FITS stores
// them) with scl / offs [nsub][nsum][nchan] -> raw [nsub][nchan][nbin]:
// f32(f32(q) * scl + offs), the two polarisations added for nsum 2 (psrfits.py
// decode, archive.py pscrunch)
hipError_t launch_decode_q(hipStream_t st, const int16_t *q, const float *scl, const float *offs, int nsub, int nchan,
                           int nbin, int nsum, bool big_endian, float *raw, int grid_cap = 0);
// the reverse: in [nprof][nbin] f32 -> PSRFITS int16 samples q [nprof][nbin]
// (big_endian: as FITS stores them) with scl / offs [nprof], bit for bit
// psrfits.py quantise (k_encode_q); nprof < 2^31, the sample index is a size_t
hipError_t launch_encode_q(hipStream_t st, const float *in, int nprof, int nbin, bool big_endian, int16_t *q,
                           float *scl, float *offs, int grid_cap = 0);
// num (s, leaf, i) = part[s*ss + leaf*sl + i], weight (s, leaf) = wpart[s*wss + leaf*wsl]
hipError_t launch_fscrunch(hipStream_t st, const double *part, long ss, long sl, const double *wpart, long wss,
                           long wsl, const SbPlan &plan, int nsub, int nbin, float *F, float *wf);
// shard root of the local super-block partials, one row of ostr doubles per
// subint: out[s*ostr + i] = tree(part[s][*][i]), out[s*ostr + nbin] =
// tree(wpart[s][*]) (wpart may be null)
hipError_t launch_sb_tree(hipStream_t st, const double *part, const double *wpart, const SbPlan &plan, int nsub,
                          int nbin, long ostr, double *out);
// windows / fscrunch rows all-gathered from the row owners -> full arrays
hipError_t launch_unpack_windows(hipStream_t st, const ShardGeom &g, int blk, const int32_t *recv, int32_t *win,
                                 int32_t *flags);
hipError_t launch_unpack_fscrunch(hipStream_t st, const ShardGeom &g, int rows_pad, long blk, int nbin,
                                  const float *recv, float *F, float *wf);
// diagnostics rows -> per-destination blocks [std|mean|fft|ptp (f64)] x rows_d x nchan_loc
// (valid == true: the single u8 field `valid` instead)
hipError_t launch_pack_rows(hipStream_t st, const ShardGeom &g, int nchan_loc, const double *std_d,
                            const double *mean_d, const double *fft_d, const double *ptp_d, const uint8_t *valid,
                            unsigned char *send, int grid_cap = 0);
// per-source blocks -> owned rows [rows_own][nchan_g] of each field
hipError_t launch_assemble_rows(hipStream_t st, const ShardGeom &g, const unsigned char *recv, double *std_r,
                                double *mean_r, double *fft_r, double *ptp_r, uint8_t *valid_r, int grid_cap = 0);
// gathered [world][8 * rows_pad] (rank p: med [4][rows_p], mad [4][rows_p]) -> row_med/row_mad [4][nsub]
hipError_t launch_unpack_rowstats(hipStream_t st, const ShardGeom &g, int rows_pad, const double *recv,
                                  double *row_med, double *row_mad);
// gathered detrended row statistics [world][rows_pad * (8 + 16 ms)] (rank p: med
// [4][rows_p], mad [4][rows_p], coefficients [4][rows_p][ms][4]) -> row_med / row_mad
// [4][nsub], row_coef [4][nsub][ms][4]
hipError_t launch_unpack_rowtrends(hipStream_t st, const ShardGeom &g, int rows_pad, int ms, const double *recv,
                                   double *row_med, double *row_mad, double *row_coef, int grid_cap = 0);
// buf[i] = sum_r gathered[r][i]
hipError_t launch_sum_i32(hipStream_t st, const int32_t *gathered, int world, int n, int32_t *buf);
// T2 (optional): [2 nbin] receives T64[0..nbin) twice
hipError_t launch_tscrunch(hipStream_t st, const float *F, const float *wf, int nsub, int nbin, float *T,
                           double *T64, double *T2 = nullptr);
hipError_t launch_fit_init(hipStream_t st, const FitStateArrays &S, long P, int32_t *z32 = nullptr,
                           int nz32 = 0, uint8_t *late = nullptr);
// S.U from the template (one block; before round 0 of every fit)
hipError_t launch_fit_prep(hipStream_t st, const FitStateArrays &S, const double *T64, int nbin);
// Round counters of the exact fit (Session::rcount, int32 words): [0, 2K) the
// packed list counts of every round (u64: [63:32] B requests at the list's
// end, [31:0] A requests at its front), [2K, 3K) the blocks of each round's
// k_fit_state that finished (u32), then the tail's sweep counter (u64, zeroed
// once per run).  k_fit_init zeroes the first 3K words every iteration.
constexpr int kMaxRounds = 1024;   // lmdif rounds per fit (maxfev = 400 bounds it far below)
constexpr int kRoundWords = 3 * kMaxRounds;
// list == nullptr: all P profiles (round 0); else the list written by the
// previous round's k_fit_state, partitioned by request: nctr -> its packed
// counts (above), their sum <= bound (the host sizes grids from a count it
// already knows: counts only shrink).
// m[k] = v for the profiles of a round list (at most `bound` entries)
hipError_t launch_mark_list(hipStream_t st, const int32_t *list, const unsigned long long *nctr, long P, long bound,
                            uint8_t *m, uint8_t v);
hipError_t launch_fit_pass(hipStream_t st, const float *D, const double *T64, long P, int nbin, int ldD,
                           int dtiled, const int32_t *list, const unsigned long long *nctr, long bound,
                           const FitStateArrays &S, bool round0);
// ctr: zeroed device word, packed [63:32] B survivors, [31:0] A survivors
// (the next round's nctr); done: zeroed word counting the finished blocks;
// host_n: host-mapped int the last block writes the survivor total to.
// round0 (launch_fit_pass): the first round (list == nullptr: every profile
// at x = 1, the fused first B sweep).
hipError_t launch_fit_state(hipStream_t st, const FitStateArrays &S, long P, const int32_t *list,
                            const unsigned long long *nctr, long bound, double *amp, int32_t *info,
                            int32_t *next_list, unsigned long long *ctr, unsigned *done, int32_t *host_n,
                            uint8_t *late = nullptr);
hipError_t launch_fit_tail(hipStream_t st, const float *D, const double *T64, long P, int nbin, int ldD,
                           int dtiled, const int32_t *list, const unsigned long long *nctr, long bound,
                           const FitStateArrays &S, double *amp, int32_t *info, unsigned long long *sweeps,
                           int grid_cap = 0);
// The power-of-two profile lengths with a templated diagnostics kernel
// (k_diag_p2<N>) and a rotation (k_rotate<N>).  This list is the one place the
// range lives: the launchers' dispatch, the host checks and the error texts
// derive from it, so a further length is an entry here plus whatever its
// instantiation needs (group_tree's wave count, RotCfg).
#define IC_P2_SIZES(X) X(64) X(128) X(256) X(512) X(1024) X(2048) X(4096) X(8192)
#define IC_P2_ENTRY(N) N,
constexpr int kP2Sizes[] = {IC_P2_SIZES(IC_P2_ENTRY)};   // ascending
#undef IC_P2_ENTRY
constexpr int kP2Min = kP2Sizes[0], kP2Max = kP2Sizes[sizeof(kP2Sizes) / sizeof(kP2Sizes[0]) - 1];
inline bool p2_supported(int nbin)
{
    for (int n : kP2Sizes)
        if (n == nbin) return true;
    return false;
}

// The mixed-radix set MR of the rotation (k_rotate_mr; phase_rotation.py
// mr_supported): kMrMin <= nbin <= kMrMax, a multiple of 8 (rows and half rows
// stay 16-byte addressable: RotateArgs' strides are multiples of 4), nbin/2 =
// 2^a 3^b 5^c, not a power of two (those are k_rotate<N>'s).  Like IC_P2_SIZES
// this is the one place the set lives; the checks and error texts derive from
// it.  The diagnostics of these lengths are k_diag_mr's (a half-length FFT of
// the same stages).
constexpr int kMrMin = 64, kMrMax = 4096;
constexpr int kMrMaxStages = 12;            // Stockham stages of FFT_{nbin/2} (4096: 5)
constexpr size_t kMrLdsBytes = 64 * 1024;   // k_rotate_mr's LDS per block (one wave at 4096)
inline bool mr_supported(int nbin)
{
    if (nbin < kMrMin || nbin > kMrMax || (nbin & 7) || !(nbin & (nbin - 1))) return false;
    int m = nbin / 2;
    const int primes[3] = {2, 3, 5};
    for (const int f : primes)
        while (m % f == 0) m /= f;
    return m == 1;
}
// the Stockham stages of FFT_{nbin/2} in the definition's order
// (phase_rotation.py stage_radices): radix 8 while three or more power-of-two
// levels remain, then 4 or 2, then the 3s, then the 5s; 4 bits per stage
// (k_rotate_mr and k_diag_mr take the same fields).  Returns the stage count,
// 0 for a length outside the set.
inline int mr_plan(int nbin, unsigned long long *radices)
{
    int m = nbin / 2, lg = 0, nst = 0;
    unsigned long long r = 0;
    const auto push = [&](int R) {
        if (nst < kMrMaxStages) r |= (unsigned long long)R << (4 * nst);
        ++nst;
    };
    while (m % 2 == 0) {
        m /= 2;
        ++lg;
    }
    for (; lg >= 3; lg -= 3) push(8);
    if (lg) push(1 << lg);
    const int odd[2] = {3, 5};
    for (const int f : odd)
        while (m % f == 0) {
            m /= f;
            push(f);
        }
    *radices = r;
    return m == 1 && nst <= kMrMaxStages ? nst : 0;
}
// The opt-in chirp-z rotation (dedisp_mode IC_DEDISP_FFT_ANY, k_rotate_czt;
// phase_rotation.py rotate_czt): every nbin in kCztMin..kCztMax that neither
// set above holds, odd and prime lengths included.  A DFT of length n as a
// circular convolution of length L = czt_length(n), the smallest power of two
// >= 2 n - 1 (Bluestein), whose FFT_L are the Stockham stages of mr_plan(2 L).
constexpr int kCztMin = 16, kCztMax = 4096;
inline bool czt_supported(int nbin)
{
    return nbin >= kCztMin && nbin <= kCztMax && !p2_supported(nbin) && !mr_supported(nbin);
}
inline int czt_length(int nbin)
{
    int L = 1;
    while (L < 2 * nbin - 1) L *= 2;
    return L;
}
// floats of the per-length tables (RotateArgs.czt): f32 pairs [L] tw =
// exp(-2 pi i q / L), [L] the filter B, [nbin] the chirp w
inline size_t czt_table_floats(int nbin) { return 2 * (2 * (size_t)czt_length(nbin) + (size_t)nbin); }
// The chirp-z statistics FFT (k_diag_czt, in both dedispersion modes;
// diag_czt.py): the lengths of czt_supported, narrowed by kDiagCztMin, below
// which the generic k_diag's direct DFT is faster per launch (measured: 0.67
// against 0.75 ms at 127 bins, 1.04 against 0.79 at 129; DESIGN.md,
// "Diagnostics at the other lengths"), and by the odd lengths above kDiagCztOddMax, whose
// convolution length 8192 needs a 144-KiB work array per profile.  Lengths
// outside it keep the generic k_diag.  This is the one place the set lives:
// launch_diag, diag_list_supported, diag_lds_bytes and the session's table
// allocation read it.  The transform is a DFT of nbin/2 complex points for an
// even nbin and of nbin real points for an odd one.
constexpr int kDiagCztMin = 129, kDiagCztOddMax = 2048;
inline bool diag_czt_supported(int nbin)
{
    return czt_supported(nbin) && nbin >= kDiagCztMin && !((nbin & 1) && nbin > kDiagCztOddMax);
}
inline int diag_czt_points(int nbin) { return (nbin & 1) ? nbin : nbin / 2; }
inline int diag_czt_length(int nbin) { return czt_length(diag_czt_points(nbin)); }
// f64 pairs of the per-length tables (DiagArgs.czt): [L] tw = exp(-2 pi i q / L),
// [L] the filter B / L, [m] the chirp w, L = diag_czt_length, m = diag_czt_points
inline size_t diag_czt_table_entries(int nbin)
{
    return 2 * (size_t)diag_czt_length(nbin) + (size_t)diag_czt_points(nbin);
}
#define IC_CZT_NBIN_FMT "; IC_DEDISP_FFT_ANY also serves any other nbin in %d..%d"
#define IC_CZT_NBIN_ARGS ::icgpu::kCztMin, ::icgpu::kCztMax
// the lengths the FFT dedispersion serves, for the error texts:
// fail(..., "... needs " IC_ROT_NBIN_FMT " (nbin=%d)", IC_ROT_NBIN_ARGS, nbin)
#define IC_ROT_NBIN_FMT                                                                            \
    "a power-of-two nbin in %d..%d, or a multiple of 8 in %d..%d whose half has only the prime factors 2, 3 and 5"
#define IC_ROT_NBIN_ARGS ::icgpu::kP2Min, ::icgpu::kP2Max, ::icgpu::kMrMin, ::icgpu::kMrMax

// Diagnostics kernels (k_diag_p2<N> / k_diag_cl<N> for the power-of-two nbin
// above, k_diag_mr for the mixed-radix set, k_diag_czt for the other lengths in
// 129..4096 (diag_czt_supported: 250, 500, 997, 2500, ...), the generic k_diag
// for what is left: 100, 125, the odd lengths above 2048).  mode: DIAG_EXACT = residual from the exact fit's amp/info and
// the fit cube D (row stride ldD); DIAG_CLOSED = fit_mode 1, the closed-form
// amplitude sum(T*p)/TT from raw + base (written to amp/info), then the same
// residual; DIAG_STATS = comprehensive_stats of the rows of D alone (no shift).
// tw: exp(-2 pi i q/nbin), q < nbin; tw_p2 (power-of-two nbin only): see p2_twiddles()
// DIAG_FIT = the closed-form amplitude alone (amp/info) of the rows of D (no
// shift, no level): fit_mode 1 with fractional dedispersion, whose residual is
// then rotated back and measured in DIAG_STATS; power-of-two nbin only.
// list / nctr / skip: the power-of-two, mixed-radix and chirp-z kernels in
// DIAG_EXACT and DIAG_STATS, k_diag_cl in its modes (diag_list_supported); the
// generic k_diag measures every profile.
enum DiagMode { DIAG_EXACT = 0, DIAG_CLOSED = 1, DIAG_STATS = 2, DIAG_FIT = 3 };
struct DiagArgs {
    int mode;
    const float *D;
    int ldD;
    const float *raw, *base;
    const double *T64, *TT;
    const double *T2;   // [2 nbin]: T64[0..nbin) twice (k_diag_cl's wrap-free gather), or null
    double *amp;
    int32_t *info;
    const float *w0;
    const int32_t *shift;
    const double2 *tw, *tw_p2;
    const PwPlan *plan;
    int nsub, nchan, nbin;
    int pr_on;
    double pr_factor;
    int pr_start, pr_end;
    double *std_o, *mean_o, *fft_o, *ptp_o;
    int data_f64;      // psrchive get_data returns f64: X = f64(R) * f64(w), f64 mean and ptp
    int dtiled;        // D is the tiled fit cube (dt_ofs); DIAG_STATS inputs are row-major
    // only the profiles of a list (the fork of the exact fit's diagnostics):
    // list + packed count as the fit rounds' (RoundList); nullptr = all
    const int32_t *list = nullptr;
    const unsigned long long *nctr = nullptr;
    const uint8_t *skip = nullptr;   // != nullptr: profiles with skip[k] != 0 are left out
    int chain = 1;   // 0: the row-layout k_diag_p2 at nbin 1024/2048/4096 too (IC_OPT_DIAG_CHAIN)
    int grid_cap = 0;   // > 0: at most this many blocks (IC_OPT_GRID_CAP; read by the launcher only)
    // k_diag_czt's per-length tables (diag_czt_table_entries); required where
    // diag_czt_supported(nbin), unused elsewhere
    const double2 *czt = nullptr;
};
hipError_t launch_diag(hipStream_t st, const DiagArgs &a);
// the diagnostics kernel launch_diag picks for `a` takes a profile list
bool diag_list_supported(const DiagArgs &a);
// late != nullptr (launch_fit_state): late[k] = 1 for every survivor of the
// round (the fork round; the flags were zeroed before it)
// dynamic LDS the generic k_diag needs for one wave (0 for the power-of-two kernels)
size_t diag_lds_bytes(int nbin);
// *TT = numpy pairwise sum of T64[i]^2 over nbin (plan), nleaf_ub >= plan leaves/ops
hipError_t launch_tnorm(hipStream_t st, const double *T64, const PwPlan *plan, int nleaf_ub, double *TT);
// The line stage: medians / MADs of the four diagnostics along channel lines
// and subint lines into a's col_* / row_*.  which: bit 0 = column lines (length
// nsub), bit 1 = row lines (length nchan).  trend != nullptr: the detrended form
// (k_linetrend), which also writes the lines' coefficients into *trend and
// takes the medians / MADs of the detrended lines; pieces != nullptr (only with
// trend): the piecewise form (k_linetrend_pw)
hipError_t launch_lines(hipStream_t st, const LineStatsArgs &a, const TrendArgs *trend, const PieceArgs *pieces,
                        int which);
// combine scales the entries (detrended with *trend, if given) with the stage's
// medians / MADs: test values, weights and the convergence counters.
// counters: [0] changed, [1] zero weights, [2] fit statuses outside 1-4 (info
// may be null), [3] test values within 1e-9 of 1.0, [4+h] new weights !=
// history h (iterative_cleaner.py:127-141)
struct CombineArgs {
    LineStatsArgs ls;                       // the stage's diagnostics and line statistics
    const int32_t *info;
    const float *w0;
    double chanthresh, subintthresh;
    double *test;
    float *W, *hist;
    int iter;
    int32_t *counters;
    int grid_cap;
    const TrendArgs *trend = nullptr;       // nullptr: plain (k_combine)
    const PieceArgs *pieces = nullptr;      // nullptr: whole lines; only with trend
    // a channel shard (only with trend; nchan_g == 0: not a shard): ls.nchan is
    // the shard's, its channels chan0 .. chan0 + nchan of nchan_g; trend->row_coef
    // (and the pieces' row tables) are whole subint lines', col_coef the shard's
    // channels'
    int chan0 = 0, nchan_g = 0;
};
hipError_t launch_combine(hipStream_t st, const CombineArgs &c);
// Phasor exp(+2 pi i k d / n) of harmonic k (0 <= k <= n/2) for a delay of d
// bins, n even (<= 8192; 1/n and 4/n are rounded factors unless n is a power
// of two): the phase rotation's multiplier
// (phase_rotation.py phasors; oracle orc_phasor).  One fixed sequence of
// separately rounded f64 operations, so that the host's per-channel table
// (ic_set_delays), the device's per-profile evaluation (ic_set_delays2) and
// the two restatements agree bit for bit:
//   the delay is split (Veltkamp, 2^13 + 1) into dh (40 significant bits) and
//   dl, so k dh and k dl are exact; t = k dh - n rint(k dh (1/n)) is exact and
//   |t| <= n/2 (an ulp of the quotient beyond it when n is no power of two); y = (t + k dl) 4/n counts quarter turns (one rounding); with
//   q = rint(y), z = y - q (exact, |z| <= 1/2), the angle is (pi/2)(q + z):
//   sin and cos of (pi/2) z by their Taylor polynomials in z^2 (through z^17
//   and z^16, Horner; truncation < 1e-17), then the quadrant q mod 4.
// ic_phasor0 is within 2.3e-16 of the exact phasor (measured against x87 long
// double); ic_phasor, the definition, takes it directly for k < 64 and for
// multiples of 64, and otherwise forms it as the product of its two parts,
// P(k) = P0(k mod 64) P0(k - k mod 64), one complex multiply of separately
// rounded operations ((a.x b.x - a.y b.y), (a.x b.y + a.y b.x)): a profile's
// n/2 + 1 phasors then need 64 + n/128 polynomial evaluations instead of one
// each (k_rotate's per-profile delays), within 7e-16 of the exact phasor for a
// power-of-two n, 1e-15 otherwise.
__host__ __device__ inline double2 ic_phasor0(int k, double d, int n)
{
    const double c = d * 8193.0;
    const double dh = c - (c - d);
    const double dl = d - dh;
    const double kk = (double)k, nn = (double)n;
    const double xh = kk * dh, xl = kk * dl;
    const double t = xh - nn * rint(xh * (1.0 / nn));
    const double y = (t + xl) * (4.0 / nn);
    const double q = rint(y);
    const double z = y - q;
    const double w = z * z;
    // (-1)^j (pi/2)^(2j+1) / (2j+1)!  and  (-1)^j (pi/2)^(2j) / (2j)!
    double sp = 0x1.aaec32af93359p-38;
    sp = -0x1.6fadb9f155744p-31 + w * sp;
    sp = 0x1.e8f434d018d63p-25 + w * sp;
    sp = -0x1.e3074fde8871fp-19 + w * sp;
    sp = 0x1.50783487ee782p-13 + w * sp;
    sp = -0x1.32d2cce62bd86p-8 + w * sp;
    sp = 0x1.466bc6775aae2p-4 + w * sp;
    sp = -0x1.4abbce625be53p-1 + w * sp;
    sp = 0x1.921fb54442d18p+0 + w * sp;
    const double sn = z * sp;
    double cp = 0x1.20c62c2f2d7f5p-34;
    cp = -0x1.b6e24f44b128fp-28 + w * cp;
    cp = 0x1.f9d38a3763cc3p-22 + w * cp;
    cp = -0x1.a6d1f2a204a8cp-16 + w * cp;
    cp = 0x1.e1f506891babbp-11 + w * cp;
    cp = -0x1.55d3c7e3cbffap-6 + w * cp;
    cp = 0x1.03c1f081b5ac4p-2 + w * cp;
    cp = -0x1.3bd3cc9be45dep+0 + w * cp;
    cp = 1.0 + w * cp;
    switch ((int)q & 3) {
    case 0: return make_double2(cp, sn);
    case 1: return make_double2(-sn, cp);
    case 2: return make_double2(-cp, -sn);
    default: return make_double2(sn, -cp);
    }
}
__host__ __device__ inline double2 ic_phasor_mul(double2 a, double2 b)
{
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__host__ __device__ inline double2 ic_phasor(int k, double d, int n)
{
    const int lo = k & 63, hi = k - lo;
    if (lo == 0 || hi == 0) return ic_phasor0(k, d, n);
    return ic_phasor_mul(ic_phasor0(lo, d, n), ic_phasor0(hi, d, n));
}

// Fractional dedispersion (dedisp_mode IC_DEDISP_FFT; phase_rotation.py):
// out[p] = rot(f32(in[p] - base[p])) by the channel's phasors, sign +1 =
// dedisperse, -1 = dededisperse.  Rows p = s*nchan + c of ld_in / ldo floats;
// out2 (optional) receives a second copy (row strides multiples of 4:
// 16-byte row accesses); in and out2 may be fit cubes in the tiled layout
// (in_tiled / out2_tiled: d_ofs, strides multiples of 32); flags: only subints
// with flags[s] != 0; late: only profiles with (late[p] != 0) == late_sel (the
// diagnostics fork's two passes).  in may equal out (each row is read whole
// before it is written).  nbin a power of two, 64 .. 8192 (IC_P2_SIZES:
// k_rotate<N>), or a mixed-radix length (mr_supported: k_rotate_mr, which
// honours everything here but the fused statistics), or, with the czt tables
// given, any other length in 16 .. 4096 (czt_supported: k_rotate_czt, likewise).
struct RotateArgs {
    const float *in;
    long ld_in;
    const float *base;          // [P] or nullptr (0)
    const float *ph;            // [nchan][nbin/2 + 1][2]: f32(ic_phasor(k, delay[c], nbin))
    const double *delay2;       // [P] per-profile delays (ic_set_delays2): phasors
                                // ic_phasor(k, delay2[p], nbin) evaluated in the kernel, ph unused
    int identity;               // the rotation is the identity (an archive stored
                                // dedispersed, sign +1): out = f32(in - base), no FFT
    int sign;
    const double2 *tw;          // [nbin]: exp(-2 pi i q / nbin)
    const int32_t *flags;       // [nsub] or nullptr (all)
    int nsub, nchan, nbin;
    float *out;
    long ldo;
    float *out2;
    long ldo2;
    // residual input (amp != nullptr): row p is f32(amp[p] * T64[i] - in[i])
    // (x pr_factor on [pr_start, pr_end)), or 0 when info[p] is outside 1-4
    // (k_residual's arithmetic); base is then unused
    const double *T64, *amp;
    const int32_t *info;
    int pr_on;
    double pr_factor;
    int pr_start, pr_end;
    int in_tiled, out2_tiled;
    const uint8_t *late;
    int late_sel;
    // list (optional): rotate only the profiles of this round list (RoundList:
    // A requests from the front, B from the end, counts packed in *nctr)
    const int32_t *list;
    const unsigned long long *nctr;
    // statistics of the rotated rows (std_o != nullptr; residual input, sign
    // -1, rotate_stats_supported): instead of writing row p to out, the kernel
    // measures X = f32(row * w0[p]) as k_diag's DIAG_STATS pass would (ic.py:
    // 111-117, :206-212) and writes std / mean / ptp / fftmax of p; out unused
    const float *w0;
    const double2 *tw_p2;       // k_diag_p2's twiddle table (p2_twiddles); unused at a mixed-radix nbin
    double *std_o, *mean_o, *ptp_o, *fft_o;
    int grid_cap;               // > 0: at most this many blocks (IC_OPT_GRID_CAP; read by the launcher only)
    // the chirp-z rotation (czt_supported(nbin), IC_DEDISP_FFT_ANY): the
    // per-length tables (czt_table_floats: tw of L, B, chirp), or nullptr: such
    // an nbin is then refused.  Its rows may have any stride and alignment (the
    // strides' multiple-of-4 condition is the other kernels'); tw, tw_p2 and
    // the fused statistics are unused.
    const float *czt;
};
hipError_t launch_rotate(hipStream_t st, const RotateArgs &a);
// RotateArgs.ph built on the device from delay [nchan] f64 (device memory):
// ph[c][k] = f32(ic_phasor(k, delay[c], nbin)), k <= nbin/2
hipError_t launch_phasor_table(hipStream_t st, const double *delay, int nchan, int nbin, float *ph,
                               int grid_cap = 0);
bool rotate_supported(int nbin);
// the residual rotation can carry the statistics (RotateArgs.std_o): f32 rows
// whose rotation keeps a profile in one wave's registers (nbin 1024)
bool rotate_stats_supported(int nbin, bool data_f64);
// D == nullptr: fit-cube rows formed from raw and base (fit_mode 1)
hipError_t launch_residual(hipStream_t st, const float *D, const float *raw, const float *base, const double *T64,
                           const double *amp, const int32_t *info, const int32_t *shift, int nsub, int nchan,
                           int nbin, int ldD, int dtiled, int pr_on, double pr_factor, int pr_start, int pr_end,
                           float *R, int grid_cap = 0);
// launch_residual and launch_encode_q in one pass (k_residual_q): the rows of
// launch_residual, never written as f32, -> q [P][nbin] int16 (big_endian: as
// FITS stores them) with scl / offs [P], bit for bit what launch_encode_q makes
// of launch_residual's cube.  A row is held in LDS: nbin <= kResidualQMaxBin
// (longer rows take the two launches).
constexpr int kResidualQMaxBin = 8192;
struct ResidualQArgs {
    const float *D;             // fit cube, or nullptr: rows from raw and base (fit_mode 1)
    const float *raw, *base;
    const double *T64, *amp;
    const int32_t *info, *shift;
    int nsub, nchan, nbin;
    int ldD, dtiled;
    int pr_on;
    double pr_factor;
    int pr_start, pr_end;
    bool big_endian;
    int16_t *q;
    float *scl, *offs;
    int grid_cap;               // > 0: at most this many blocks (IC_OPT_GRID_CAP)
};
hipError_t launch_residual_q(hipStream_t st, const ResidualQArgs &a);

// Standard template (ic_set_std_template; std_template.py): the alignment modes
// (the public IC_ALIGN_*), the record k_std_peak writes - its shift is also the
// device-resident delay the `frac` rotation reads (RotateArgs.delay2) - and the
// launchers of ic_stdtemplate.hip.
constexpr int kAlignNone = 0, kAlignInt = 1, kAlignFrac = 2;
struct StdAlignRec {
    double shift;       // lag + the parabola's sub-bin part; 0.0 after a failed alignment
    int32_t aligned;    // 1: a positive finite peak was found
    int32_t lag;        // first argmax of the cross-correlation; 0 after a failed alignment
};
// dynamic LDS of k_std_ccf: S and A as f32
size_t std_ccf_lds_bytes(int nbin);
// c[k] = sum_i f64(A[i]) * (f64(S[(i - k) mod nbin]) - m), ascending i; m: the
// mean of f64(S) summed in ascending index (host)
hipError_t launch_std_ccf(hipStream_t st, const float *S, const float *A, int nbin, double m, double *c,
                          int grid_cap = 0);
hipError_t launch_std_peak(hipStream_t st, const double *c, int nbin, StdAlignRec *rec);
// T [nbin], T64 [ldD] (zero tail), T2 [2 nbin] (optional) from S as given
// (kAlignNone; rec and R unused), S gathered by rec->lag (kAlignInt) or R, the
// rotated standard, when rec->aligned, else S (kAlignFrac)
hipError_t launch_std_install(hipStream_t st, const float *S, const float *R, const StdAlignRec *rec, int mode,
                              int nbin, int ldD, float *T, double *T64, double *T2, int grid_cap = 0);

// Hot-bin repair (ic_set_hotbins; hotbins.py): the off-pulse bins of every
// profile are clipped against their median and MAD and the few that stand out
// are set to the survivors' median, in place (ic_hotbins.hip).  A stored bin j
// of profile k is on-pulse iff ((j - o_k) mod nbin - win_start) mod nbin <
// win_len, win_* the window already widened and clamped (win_len 0: none).
// o_k comes from one of: off32 (int32, any value), offd (f64, rint'ed), or 0;
// per_profile 0: indexed by the channel k % nchan, 1: by k.
constexpr int kHotMaxBin = 8192;      // one block of 8 waves holds 16 samples per lane
constexpr int kHotMinOff = 8;         // fewer off-pulse bins are refused
constexpr int kHotMaxRounds = 8;
struct HotBinArgs {
    float *cube;                // [P][nbin], repaired in place
    const float *w0;            // [P]
    const int32_t *off32;
    const double *offd;
    int per_profile;
    long P;
    int nchan, nbin;
    int win_start, win_len;
    double threshold;
    int rounds;
    int32_t *count;             // [P]: bins repaired, 0, or -1 (over the cap)
    uint32_t *mask;             // [P][mask_words(nbin)]: bit j of a profile's words = bin j repaired
    int grid_cap;
};
inline int hot_mask_words(int nbin) { return (nbin + 31) / 32; }
// detect and repair: count and mask written for every profile
hipError_t launch_hotbins(hipStream_t st, const HotBinArgs &a);
// the hit list from count and mask (a mask row is defined only where count >
// 0): offs[k] = the sum of the positive counts before k, *total their sum (part:
// hotbin_scan_parts(P) words of scratch, a block's sum each); then
// bins[offs[k] ..) = the set bits of profile k, ascending, the entries below cap
size_t hotbin_scan_parts(long P);
hipError_t launch_hotbin_scan(hipStream_t st, const int32_t *count, long P, int64_t *part, int64_t *offs,
                              int64_t *total);
hipError_t launch_hotbin_fill(hipStream_t st, const int32_t *count, const uint32_t *mask, const int64_t *offs, long P,
                              int nbin, int32_t *bins, int64_t cap, int grid_cap = 0);

// Dynamic spectrum (ic_get_dynspec; dynspec.py): the free-baseline template fit
// of every dedispersed profile, after a run (ic_dynspec.hip).  x: the raw cube
// [P][nbin] with shift [nchan] (profile k reads channel k % nchan's; bin i of
// the dedispersed profile is x[(i + shift) % nbin]), or rows already
// dedispersed (shift == nullptr).  tt: launch_dynspec_prep's [2 + nbin] doubles
// (mT, Stt, then t).  Profiles with w == 0 get zeros and their rows are not
// read.  amp / err / base [P]: any may be null.
constexpr int kDynMinBin = 4;          // fewer bins are refused
constexpr int kDynRegMaxBin = 8192;    // up to here a row stays in one wave's registers between the passes
struct DynspecArgs {
    const float *x;
    const int32_t *shift;
    const float *w;
    const double *tt;
    long P;
    int nchan, nbin;
    double *amp, *err, *base;
    int grid_cap;
};
hipError_t launch_dynspec_prep(hipStream_t st, const float *T, int nbin, double *tt);
hipError_t launch_dynspec(hipStream_t st, const DynspecArgs &a);

}  // namespace icgpu
