// ic_template.hip -- the template stage of the surgical-cleaning loop
// (iterative_cleaner.py:88-100: baseline, scrunches, template, and the fit
// cube that comes out of the same read), with its launchers.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see Makefile).
// -ffp-contract=off is load-bearing: every f64/f32 operation below must be an
// individually rounded IEEE op in the order written, so that results equal
// numpy / scipy (MINPACK) bit-for-bit.  Explicit fma() is never used on an
// exact path.
//
// Kernels (per cleaning iteration, in launch order):
//   k_valid          (once per run) validity and the first weights from w0
//   k_chan_partials  canonical-order channel sums (archive.py chan_sum) of
//                    W*ded (baseline total) or W*f32(ded-base) (fscrunch)
//   k_chan_delta     the same sums moved through the changed channels only
//   k_window         per-subint off-pulse window: first argmin of circular
//                    window sums (archive.py window_argmin)
//   k_base           per-profile window mean -> f32 baseline
//   k_fscrunch       combine super-block partials -> F[s][i], wf[s]
//   k_sb_tree        (channel shards) local super-block partials -> shard root
//   k_tscrunch       weighted mean over subints, *10000 -> T (ic.py:94)
#include <algorithm>
#include <math.h>

#include "ic_wave.h"

namespace icgpu {

// ============================================================ template stage

// once per run: valid = (w0 != 0); the weights and the first history entry start at w0
__global__ void k_valid(const float *w0, uint8_t *valid, float *W, float *hist0, size_t P)
{
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < P) {
        const float w = w0[k];
        valid[k] = (w != 0.0f);
        W[k] = w;
        hist0[k] = w;
    }
}

// part[s][sb][i] = sum_{c in sb, ascending} W[s,c] * x[s,c,i]   (f64, from 0.0)
// x = ded (base == nullptr) or f32(ded - base[s,c]);  wpart[s][sb] = sum W.
// One lane per bin; lanes of a wave read 64 consecutive (rotated) bins.
// Canonical-order channel partial sums over one super-block, lane per bin:
//   MODE 0: part  = sum_c W*ded                     (baseline window total)
//   MODE 1: part2 = sum_c W*f32(ded - base), wpart  (fscrunch)
//   MODE 2: both, in one read of the cube (base = the previous iteration's)
//   MODE 3: MODE 1 that also writes the fit cube D[k][i] = f32(ded - base)
//           (iteration 1: base = base0, W = w0: the fit cube of ic.py:96-100 comes
//           out of the same read of the cube)
// flags != nullptr: only subints with flags[s] != 0 (a moved window) run.
// the fit cube is written once and read by the next kernels' sweeps, not by
// this one: non-temporal stores keep the write stream out of the way (C2
// -0.14 ms per clean; non-temporal raw loads here cost +0.5 ms)
__device__ __forceinline__ void st_fitcube(float *p, float v)
{
    __builtin_nontemporal_store(v, p);
}

// Exactness of a super-block column (the incremental template stage,
// k_chan_delta), for archives whose weights are 0 or 1: the column's terms
// are its values v_c (f64 from f32) over EVERY channel c of the super-block,
// whatever its current weight.  With biased f32 exponents emin / emax of the
// nonzero ones (subnormals as 1), every v_c is an integer multiple of
// 2^(emin - 150) and 256 |v_c| < 2^(emax - 118); if emax - emin <= 21 every
// partial sum of any subset of them, in any order and with any signs, is an
// f64 integer multiple of 2^(emin - 150) below 2^(53 + emin - 150): exact.
// The canonical sequential sum then equals the exact sum, and so does an old
// sum plus the terms that entered minus those that left.  ExTrack keeps the
// largest and smallest nonzero magnitude as bit patterns (4 VALU ops per
// value; an Inf / NaN value is a larger pattern than any finite one and fails
// the test).  Fractional weights: k_chan_delta ignores the flags.
struct ExTrack {
    unsigned mx = 0u, mn = 0xffffffffu;   // max |v| bits, min (|v| bits - 1): zero -> 0xffffffff
    __device__ __forceinline__ void add(float v)
    {
        const unsigned a = __float_as_uint(v) & 0x7fffffffu;
        mx = max(mx, a);
        mn = min(mn, a - 1u);
    }
    __device__ __forceinline__ uint8_t exact() const
    {
        if (mx >= 0x7f800000u) return 0;   // Inf / NaN
        if (mn == 0xffffffffu) return 1;   // all zero
        const int emax = max((int)(mx >> 23), 1), emin = max((int)((mn + 1u) >> 23), 1);
        return emax - emin <= 21 ? 1 : 0;
    }
};

template <int MODE>
__global__ __launch_bounds__(256) void k_chan_partials(
    const float *__restrict__ raw, const float *__restrict__ W, const int32_t *__restrict__ shift,
    const float *__restrict__ base, const int32_t *__restrict__ flags, int nsub, int nchan, int nbin, int nsb,
    double *__restrict__ part, double *__restrict__ part2, double *__restrict__ wpart, float *__restrict__ D,
    int ldD, int dtiled, uint8_t *__restrict__ exA, uint8_t *__restrict__ exF)
{
    constexpr bool A = MODE == 0 || MODE == 2, F = MODE != 0, WD = MODE == 3;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int sb = blockIdx.y;
    const int s = blockIdx.z;
    if (flags && flags[s] == 0) return;
    const int c0 = sb * kSuperBlock;
    const int c1 = min(c0 + kSuperBlock, nchan);
    // column exactness (ExTrack) of this pass's sums (A: exA, F: exF)
    const bool tA = A && exA, tF = F && exF;
    ExTrack xa, xf;
    if (i < nbin) {
        double acc = 0.0, acc2 = 0.0;
        const size_t krow = (size_t)s * nchan;
        // batches of 16 channels: all 16 row loads are issued before the
        // (sequential, canonical-order) accumulation consumes them
        constexpr int B = 16;
        int c = c0;
        for (; c + B <= c1; c += B) {
            float xv[B], wv[B], bv[B];
#pragma unroll
            for (int q = 0; q < B; ++q) {
                int j = i + shift[c + q];
                if (j >= nbin) j -= nbin;
                xv[q] = raw[(krow + c + q) * nbin + j];
                wv[q] = W[krow + c + q];
                bv[q] = F ? base[krow + c + q] : 0.0f;
            }
#pragma unroll
            for (int q = 0; q < B; ++q) {
                const double w = (double)wv[q];
                const float d = xv[q] - bv[q];
                if (A) acc = acc + w * (double)xv[q];
                if (F) acc2 = acc2 + w * (double)d;
                if (WD) st_fitcube(D + d_ofs(krow + c + q, i, ldD, dtiled), d);
                if (tA) xa.add(xv[q]);
                if (tF) xf.add(d);
            }
        }
        for (; c < c1; ++c) {
            const size_t k = krow + c;
            int j = i + shift[c];
            if (j >= nbin) j -= nbin;
            const float x = raw[k * nbin + j];
            const double w = (double)W[k];
            const float d = F ? x - base[k] : 0.0f;
            if (A) acc = acc + w * (double)x;
            if (F) acc2 = acc2 + w * (double)d;
            if (WD) st_fitcube(D + d_ofs(k, i, ldD, dtiled), d);
            if (tA) xa.add(x);
            if (tF) xf.add(d);
        }
        const size_t col = ((size_t)s * nsb + sb) * nbin + i;
        if (A) part[col] = acc;
        if (F) part2[col] = acc2;
        if (tA) exA[col] = xa.exact();
        if (tF) exF[col] = xf.exact();
    }
    if (F && blockIdx.x == 0 && threadIdx.x == 0) {
        double a = 0.0;
        for (int c = c0; c < c1; ++c) a = a + (double)W[(size_t)s * nchan + c];
        wpart[(size_t)s * nsb + sb] = a;
    }
}

// Incremental template stage (iteration >= 2, integer dedispersion): the
// window totals `part` and the fscrunch partials `part2` of every super-block
// column move from the previous weights Wo to the current Wn by the terms of
// the channels whose weight changed: old + (sum of Wn v - Wo v over them),
// exact for columns whose flag (ExTrack, set by the last full pass) holds;
// the other columns, and every column of a super-block with a weight other
// than 0 or 1, are summed again in canonical order over all channels.  part2
// uses the carried levels: subints whose window moves are summed again
// afterwards (k_chan_partials mode 1, flagged).  wpart is summed again (256
// weights).  One block per (bin range, super-block, subint); a block whose
// super-block has no changed channel does nothing.
// BPT bins per thread (bin i0 + 256 b, b < BPT): the change list and the
// block's fixed costs serve BPT times the columns, and BPT times the loads are
// in flight per batch of channels.
// SPLIT (FFT dedispersion): part's terms come from raw (the rotated raw cube)
// and part2's from rawF (the rotated baselined rows Tc, base = 0); otherwise
// both from raw, part2's as f32(raw - base).
template <int BPT, bool SPLIT>
__global__ __launch_bounds__(256) void k_chan_delta(const float *__restrict__ raw, const float *__restrict__ rawF,
                                                    const int32_t *__restrict__ shift,
                                                    const float *__restrict__ base, const float *__restrict__ Wn,
                                                    const float *__restrict__ Wo, int nchan, int nbin, int nsb,
                                                    double *__restrict__ part, double *__restrict__ part2,
                                                    double *__restrict__ wpart, const uint8_t *__restrict__ exA,
                                                    const uint8_t *__restrict__ exF)
{
    __shared__ int chg[kSuperBlock];
    __shared__ int fix[256 * BPT];           // columns summed again: bin | 1 << 16 (part) | 1 << 17 (part2)
    __shared__ double tA[kSuperBlock], tF[kSuperBlock];
    __shared__ int wcnt[4], wfrac[4], wfix[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i0 = blockIdx.x * 256 * BPT + threadIdx.x;
    const int sb = blockIdx.y, s = blockIdx.z;
    const int c0 = sb * kSuperBlock, c1 = min(c0 + kSuperBlock, nchan);
    const size_t krow = (size_t)s * nchan;
    const size_t col0 = ((size_t)s * nsb + sb) * nbin;
    // the changed channels of the super-block, in ascending order
    int n, frac, nones;
    {
        const int c = c0 + (int)threadIdx.x;
        const float wn = c < c1 ? Wn[krow + c] : 0.0f, wo = c < c1 ? Wo[krow + c] : 0.0f;
        const bool ch = __float_as_uint(wn) != __float_as_uint(wo);
        const bool fr = !(wn == 0.0f || wn == 1.0f) || !(wo == 0.0f || wo == 1.0f);
        const unsigned long long m = __ballot(ch);
        const unsigned long long m1 = __ballot(wn == 1.0f);
        const bool fw = __any(fr);
        if (lane == 0) {
            wcnt[wave] = __popcll(m);
            wfrac[wave] = fw ? 1 : 0;
            wfix[wave] = __popcll(m1);
        }
        __syncthreads();
        int off = 0;
        for (int w = 0; w < wave; ++w) off += wcnt[w];
        if (ch) chg[off + __popcll(m & ((1ull << lane) - 1ull))] = c;
        n = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        frac = wfrac[0] | wfrac[1] | wfrac[2] | wfrac[3];
        nones = wfix[0] + wfix[1] + wfix[2] + wfix[3];
        __syncthreads();
    }
    if (n == 0) return;
    constexpr int B = 16 / BPT;   // channels per batch: 16 loads in flight per thread
    if (frac) {
        // a weight other than 0 / 1: every column in canonical order (k_chan_partials' sums)
#pragma unroll
        for (int b = 0; b < BPT; ++b) {
            const int i = i0 + 256 * b;
            if (i >= nbin) continue;
            double acc = 0.0, acc2 = 0.0;
            int c = c0;
            for (; c + 16 <= c1; c += 16) {
                float xv[16], wv[16], bv[16];
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    int j = i + shift[c + q];
                    if (j >= nbin) j -= nbin;
                    xv[q] = raw[(krow + c + q) * nbin + j];
                    wv[q] = Wn[krow + c + q];
                    bv[q] = SPLIT ? rawF[(krow + c + q) * nbin + j] - base[krow + c + q] : base[krow + c + q];
                }
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const double w = (double)wv[q];
                    const float d = SPLIT ? bv[q] : xv[q] - bv[q];
                    acc = acc + w * (double)xv[q];
                    acc2 = acc2 + w * (double)d;
                }
            }
            for (; c < c1; ++c) {
                int j = i + shift[c];
                if (j >= nbin) j -= nbin;
                const float x = raw[(krow + c) * nbin + j];
                const double w = (double)Wn[krow + c];
                const float d = (SPLIT ? rawF[(krow + c) * nbin + j] : x) - base[krow + c];
                acc = acc + w * (double)x;
                acc2 = acc2 + w * (double)d;
            }
            part[col0 + i] = acc;
            part2[col0 + i] = acc2;
        }
    } else {
        bool okA[BPT], okF[BPT];
        double dA[BPT], dF[BPT];
#pragma unroll
        for (int b = 0; b < BPT; ++b) {
            const int i = i0 + 256 * b;
            okA[b] = i < nbin && exA[col0 + i];
            okF[b] = i < nbin && exF[col0 + i];
            dA[b] = dF[b] = 0.0;
        }
        for (int q0 = 0; q0 < n; q0 += B) {
            float xv[B][BPT], fv[SPLIT ? B : 1][BPT], bv[B], wnv[B], wov[B];
#pragma unroll
            for (int q = 0; q < B; ++q) {
                const int c = chg[min(q0 + q, n - 1)];
                bv[q] = base[krow + c];
                wnv[q] = Wn[krow + c];
                wov[q] = Wo[krow + c];
                const float *row = raw + (krow + c) * nbin;
                const int sc = shift[c];
#pragma unroll
                for (int b = 0; b < BPT; ++b) {
                    const int i = min(i0 + 256 * b, nbin - 1);
                    int j = i + sc;
                    if (j >= nbin) j -= nbin;
                    xv[q][b] = row[j];
                    if (SPLIT) fv[SPLIT ? q : 0][b] = rawF[(krow + c) * nbin + j];
                }
            }
#pragma unroll
            for (int q = 0; q < B; ++q) {
                if (q0 + q < n) {
                    const double wn = (double)wnv[q], wo = (double)wov[q];
#pragma unroll
                    for (int b = 0; b < BPT; ++b) {
                        const float d = (SPLIT ? fv[SPLIT ? q : 0][b] : xv[q][b]) - bv[q];
                        dA[b] = dA[b] + (wn * (double)xv[q][b] - wo * (double)xv[q][b]);
                        dF[b] = dF[b] + (wn * (double)d - wo * (double)d);
                    }
                }
            }
        }
        int need[BPT];
#pragma unroll
        for (int b = 0; b < BPT; ++b) {
            const int i = i0 + 256 * b;
            need[b] = 0;
            if (i < nbin) {
                if (okA[b]) part[col0 + i] = part[col0 + i] + dA[b];
                if (okF[b]) part2[col0 + i] = part2[col0 + i] + dF[b];
                need[b] = (okA[b] ? 0 : 1 << 16) | (okF[b] ? 0 : 1 << 17);
            }
        }
        // inexact columns: the whole block sums each again, one channel per
        // thread, then one thread adds the 256 terms in canonical order
        int nfix = 0;
#pragma unroll
        for (int b = 0; b < BPT; ++b) {
            const unsigned long long m = __ballot(need[b] != 0);
            if (lane == 0) wfix[wave] = __popcll(m);
            __syncthreads();
            int off = nfix;
            for (int w = 0; w < wave; ++w) off += wfix[w];
            if (need[b]) fix[off + __popcll(m & ((1ull << lane) - 1ull))] = need[b] | (i0 + 256 * b);
            nfix += wfix[0] + wfix[1] + wfix[2] + wfix[3];
            __syncthreads();
        }
        for (int f = 0; f < nfix; ++f) {
            const int e = fix[f], ib = e & 0xffff;
            const int c = c0 + (int)threadIdx.x;
            if (c < c1) {
                int j = ib + shift[c];
                if (j >= nbin) j -= nbin;
                const float x = raw[(krow + c) * nbin + j];
                const double w = (double)Wn[krow + c];
                const float d = (SPLIT ? rawF[(krow + c) * nbin + j] : x) - base[krow + c];
                tA[threadIdx.x] = w * (double)x;
                tF[threadIdx.x] = w * (double)d;
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                double acc = 0.0, acc2 = 0.0;
                for (int q = 0; q < c1 - c0; ++q) {
                    acc = acc + tA[q];
                    acc2 = acc2 + tF[q];
                }
                if (e & (1 << 16)) part[col0 + ib] = acc;
                if (e & (1 << 17)) part2[col0 + ib] = acc2;
            }
            __syncthreads();
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        // weights 0 / 1 only: the sequential sum is the count of ones, exactly
        double a = (double)nones;
        if (frac) {
            a = 0.0;
            for (int c = c0; c < c1; ++c) a = a + (double)Wn[krow + c];
        }
        wpart[(size_t)s * nsb + sb] = a;
    }
}

// Canonical super-block combine (archive.py sb_tree) as a post-order stack
// program (SbPlan): the stack lives in registers (static indices only), top
// at st[0].
template <typename Get>
__device__ __forceinline__ double sb_eval(const SbPlan &pl, Get get)
{
    double st[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) st[k] = 0.0;
    for (int j = 0; j < pl.n; ++j) {
#pragma unroll
        for (int k = 7; k > 0; --k) st[k] = st[k - 1];
        st[0] = get(j);
        for (int m = 0; m < (int)pl.merges[j]; ++m) {
            st[0] = st[1] + st[0];   // left subtree + right subtree
#pragma unroll
            for (int k = 1; k < 7; ++k) st[k] = st[k + 1];
        }
    }
    return st[0];
}

// numpy argmin combine: first NaN wins; otherwise smaller value, then lower index.
__device__ __forceinline__ bool argmin_better(double va, int ia, double vb, int ib)
{
    const bool na = isnan(va), nb = isnan(vb);
    if (na || nb) {
        if (na && nb) return ia < ib;
        return na;
    }
    if (va < vb) return true;
    if (vb < va) return false;
    return ia < ib;
}

// One block per subint: tot[i] = sb_tree over the leaves of part; m[j] =
// sum_{k<width} tot[(j+k)%n]; win[s] = first argmin.
// flags != nullptr: flags[s] = (window moved), win[s] updated in place.
// kWindowThreads threads, so each window sum (a width-long in-order chain) has
// its own thread up to nbin = 1024.  The argmin order (NaN first, then value,
// then index) is total, so the result does not depend on the block size.
constexpr int kWindowThreads = 1024;
__global__ __launch_bounds__(kWindowThreads) void k_window(const double *__restrict__ part, long ss, long sl, SbPlan plan,
                                                int nbin, int width, int32_t *__restrict__ win,
                                                int32_t *__restrict__ flags)
{
    extern __shared__ double sh[];
    double *tot = sh;                       // nbin
    double *bv = sh + nbin;                 // blockDim
    int *bi = (int *)(bv + blockDim.x);     // blockDim
    const int s = blockIdx.x;
    for (int i = threadIdx.x; i < nbin; i += blockDim.x) {
        const double *src = part + (size_t)s * ss + i;
        tot[i] = sb_eval(plan, [&](int j) { return src[(size_t)j * sl]; });
    }
    __syncthreads();
    double best = 0.0;
    int besti = -1;
    for (int j = threadIdx.x; j < nbin; j += blockDim.x) {
        double m = 0.0;
        int q = j;
        for (int k = 0; k < width; ++k) {
            m = m + tot[q];
            if (++q == nbin) q = 0;
        }
        if (besti < 0 || argmin_better(m, j, best, besti)) {
            best = m;
            besti = j;
        }
    }
    bv[threadIdx.x] = best;
    bi[threadIdx.x] = besti;
    __syncthreads();
    for (int off = blockDim.x / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            const int o = threadIdx.x + off;
            if (bi[o] >= 0 && (bi[threadIdx.x] < 0 ||
                               argmin_better(bv[o], bi[o], bv[threadIdx.x], bi[threadIdx.x]))) {
                bv[threadIdx.x] = bv[o];
                bi[threadIdx.x] = bi[o];
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (flags) {
            const int moved = win[s] != bi[0];
            flags[s] = moved;
            if (moved) atomicAdd(&flags[gridDim.x], 1);   // flags[nsub]: moves counter
        }
        win[s] = bi[0];
    }
}

// base[k] = f32( (sum_{t<width} f64(ded[(win+t)%n])) / width ), sequential in t.
// Per-profile baseline level: f32(sum_seq f64(x_j) / width) over the subint's
// window, in the dedispersed frame (Appendix C stand-in; oracle orc_baseline).
// Four profiles per wave, 16 lanes each: a lane issues its window loads in
// batches of 8 before adding them, so one memory latency serves four profiles
// (one profile per wave left the kernel bound by a full latency per profile).
// The sequential f64 sum of f32 values is computed in parallel when that is
// provably exact: every x_j is an integer multiple of 2^(emin-150) and
// |sum| < width * 2^(emax-126), so when ceil(log2 width) + emax - emin + 24 <=
// 53 every partial sum, in any order, is representable and the result equals
// the sequential one bit for bit.  Otherwise (rare: values spanning > 2^21, or
// Inf/NaN) the profile's 16 lanes walk the window in order.
// V4 (nbin % 4 == 0, 16-B aligned rows): the lanes read the aligned float4s
// that cover the window (which wraps on a float4 boundary) and keep the
// elements inside it; the exact path does not depend on the order of the adds.
template <bool V4>
__global__ __launch_bounds__(256) void k_base(const float *__restrict__ raw, const int32_t *__restrict__ shift,
                                              const int32_t *__restrict__ win, const int32_t *__restrict__ flags,
                                              int nsub, int nchan, int nbin, int width, float *__restrict__ base)
{
    constexpr int GL = 16, BATCH = 8;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int grp = lane / GL, gl = lane % GL;
    const long P = (long)nsub * nchan;
    const int lgw = 32 - __clz(max(width - 1, 1));   // ceil(log2(width)), >= 1
    for (long k0 = ((long)blockIdx.x * 4 + wave) * 4; k0 < P; k0 += (long)gridDim.x * 16) {
        const long k = k0 + grp;
        // window unchanged: base unchanged
        const bool act = k < P && !(flags && flags[k / nchan] == 0);
        double acc = 0.0;
        int emax = 0, emin = 255, q0 = 0;
        const float *row = raw + (size_t)(act ? k : 0) * nbin;
        if (act) {
            q0 = win[k / nchan] + shift[k % nchan];
            if (q0 >= nbin) q0 -= nbin;
            if constexpr (V4) {
                const float4 *row4 = (const float4 *)row;
                const int nq = nbin >> 2, a = q0 >> 2, off = q0 & 3;
                const int nf = (off + width + 3) >> 2;   // float4s covering the window
                constexpr int B4 = 4;
                for (int m0 = gl; m0 < nf; m0 += GL * B4) {
                    float4 xv[B4];
#pragma unroll
                    for (int u = 0; u < B4; ++u) {
                        const int m = m0 + GL * u;
                        int qi = a + m;
                        if (qi >= nq) qi -= nq;
                        xv[u] = m < nf ? row4[qi] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    }
#pragma unroll
                    for (int u = 0; u < B4; ++u) {
                        const int e0 = 4 * (m0 + GL * u) - off;   // window offset of the first element
                        const float xs[4] = {xv[u].x, xv[u].y, xv[u].z, xv[u].w};
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            const float x = (e0 + c >= 0 && e0 + c < width) ? xs[c] : 0.0f;
                            acc = acc + (double)x;
                            const int be = max((int)((__float_as_uint(x) >> 23) & 0xffu), 1);
                            if (x != 0.0f) {
                                emax = max(emax, be);
                                emin = min(emin, be);
                            }
                        }
                    }
                }
            } else
            for (int j0 = gl; j0 < width; j0 += GL * BATCH) {
                float xv[BATCH];
#pragma unroll
                for (int u = 0; u < BATCH; ++u) {
                    const int j = j0 + GL * u;
                    int q = q0 + j;
                    if (q >= nbin) q -= nbin;
                    xv[u] = j < width ? row[q] : 0.0f;
                }
#pragma unroll
                for (int u = 0; u < BATCH; ++u) {
                    const float x = xv[u];
                    acc = acc + (double)x;
                    const int be = max((int)((__float_as_uint(x) >> 23) & 0xffu), 1);
                    if (x != 0.0f) {
                        emax = max(emax, be);
                        emin = min(emin, be);
                    }
                }
            }
        }
        for (int off = GL / 2; off > 0; off >>= 1) {   // within the 16-lane group
            acc = acc + __shfl_xor(acc, off);
            emax = max(emax, __shfl_xor(emax, off));
            emin = min(emin, __shfl_xor(emin, off));
        }
        if (act && emax != 0 && lgw + emax - emin + 24 > 53) {
            acc = 0.0;   // in order (every lane of the group walks the same values)
            for (int j = 0; j < width; ++j) {
                int q = q0 + j;
                if (q >= nbin) q -= nbin;
                acc = acc + (double)row[q];
            }
        }
        if (act && gl == 0) base[k] = (float)(acc / (double)width);
    }
}

// F[s][i] = f32(num/wsum) (0 if wsum == 0); wf[s] = f32(wsum); num and wsum
// are the canonical trees over the leaves
__global__ __launch_bounds__(256) void k_fscrunch(const double *__restrict__ part, long ss, long sl,
                                                  const double *__restrict__ wpart, long wss, long wsl, SbPlan plan,
                                                  int nbin, float *__restrict__ F, float *__restrict__ wf)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int s = blockIdx.y;
    if (i >= nbin) return;
    const double *src = part + (size_t)s * ss + i;
    const double *wsrc = wpart + (size_t)s * wss;
    const double num = sb_eval(plan, [&](int j) { return src[(size_t)j * sl]; });
    const double wsum = sb_eval(plan, [&](int j) { return wsrc[(size_t)j * wsl]; });
    F[(size_t)s * nbin + i] = (wsum != 0.0) ? (float)(num / wsum) : 0.0f;
    if (i == 0) wf[s] = (float)wsum;
}

// Shard root of local super-block partials [s][nsb_loc][nbin] (channel shards):
// out[s*ostr + i] = sb_tree(part[s][*][i]); out[s*ostr + nbin] = sb_tree(wpart[s][*])
// (wpart optional; ostr >= nbin + 1 then): one row per subint, so the rows a
// rank owns are one contiguous all-to-all block.
__global__ __launch_bounds__(256) void k_sb_tree(const double *__restrict__ part, const double *__restrict__ wpart,
                                                 SbPlan plan, int nbin, long ostr, double *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int s = blockIdx.y;
    const int n = plan.n;
    if (i < nbin) {
        const double *src = part + (size_t)s * n * nbin + i;
        out[(size_t)s * ostr + i] = sb_eval(plan, [&](int j) { return src[(size_t)j * nbin]; });
    }
    if (wpart && i == 0) {
        const double *w = wpart + (size_t)s * n;
        out[(size_t)s * ostr + nbin] = sb_eval(plan, [&](int j) { return w[j]; });
    }
}

// T[i] = f32( f32(sum_s wf*F / sum_s wf) * 10000 )
__global__ __launch_bounds__(256) void k_tscrunch(const float *__restrict__ F, const float *__restrict__ wf,
                                                  int nsub, int nbin, float *__restrict__ T,
                                                  double *__restrict__ T64, double *__restrict__ T2)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nbin) return;
    double wt = 0.0, num = 0.0;
    // batches of 16 subints: the 16 loads are in flight together, then the
    // sums run in subint order (the chain is latency-bound with 16 blocks)
    constexpr int B = 16;
    int s = 0;
    for (; s + B <= nsub; s += B) {
        float fv[B], wv[B];
#pragma unroll
        for (int q = 0; q < B; ++q) {
            wv[q] = wf[s + q];
            fv[q] = F[(size_t)(s + q) * nbin + i];
        }
#pragma unroll
        for (int q = 0; q < B; ++q) {
            const double w = (double)wv[q];
            wt = wt + w;
            const double t = w * (double)fv[q];
            num = num + t;
        }
    }
    for (; s < nsub; ++s) {
        const double w = (double)wf[s];
        wt = wt + w;
        const double t = w * (double)F[(size_t)s * nbin + i];
        num = num + t;
    }
    const float t = (wt != 0.0) ? (float)(num / wt) : 0.0f;
    const float tt = t * 10000.0f;
    T[i] = tt;
    T64[i] = (double)tt;
    if (T2) {
        T2[i] = (double)tt;
        T2[i + nbin] = (double)tt;
    }
}

// ============================================================ launchers

hipError_t launch_valid(hipStream_t st, const float *w0, uint8_t *valid, float *W, float *hist0, size_t P)
{
    IC_GGL(k_valid, dim3(cdiv(P, 256)), dim3(256), 0, st, w0, valid, W, hist0, P);
    return hipGetLastError();
}

hipError_t launch_chan_partials(hipStream_t st, int mode, const float *raw, const float *W, const int32_t *shift,
                                const float *base, const int32_t *flags, int nsub, int nchan, int nbin,
                                double *part, double *part2, double *wpart, float *D, int ldD, int dtiled,
                                uint8_t *exA, uint8_t *exF)
{
    const int nsb = super_blocks(nchan);
    const int bs = bin_block(nbin);
    dim3 grid(cdiv(nbin, bs), nsb, nsub);
    if (mode == 3 && (!D || ldD < nbin || (dtiled && ldD % 32 != 0))) return hipErrorInvalidValue;
#define IC_CP(M)                                                                                                  \
    IC_GGL(k_chan_partials<M>, grid, dim3(bs), 0, st, raw, W, shift, base, flags, nsub, nchan, nbin, \
                       nsb, part, part2, wpart, D, ldD, dtiled, exA, exF)
    if (mode == 0)
        IC_CP(0);
    else if (mode == 1)
        IC_CP(1);
    else if (mode == 2)
        IC_CP(2);
    else
        IC_CP(3);
#undef IC_CP
    return hipGetLastError();
}

size_t window_lds_bytes(int nbin) { return (size_t)nbin * 8 + kWindowThreads * (8 + 4); }

hipError_t launch_chan_delta(hipStream_t st, const float *raw, const int32_t *shift, const float *base,
                             const float *Wn, const float *Wo, int nsub, int nchan, int nbin, double *part,
                             double *part2, double *wpart, const uint8_t *exA, const uint8_t *exF,
                             const float *rawF)
{
    const int nsb = super_blocks(nchan);
    if (!exA || !exF) return hipErrorInvalidValue;
    // 256 threads: one per channel of the super-block (the change list), then one per bin
    // bins per thread by nbin (C5 template stage 4.55 -> 4.32 ms per clean against 1)
    const int bpt = nbin >= 1024 ? 4 : (nbin >= 512 ? 2 : 1);
#define IC_CD(BP, SP)                                                                                   \
    IC_GGL((k_chan_delta<BP, SP>), dim3(cdiv(nbin, 256 * BP), nsb, nsub), dim3(256), 0, st, raw, rawF, shift, \
           base, Wn, Wo, nchan, nbin, nsb, part, part2, wpart, exA, exF)
    if (rawF) {
        if (bpt == 4) IC_CD(4, true);
        else if (bpt == 2) IC_CD(2, true);
        else IC_CD(1, true);
    } else {
        if (bpt == 4) IC_CD(4, false);
        else if (bpt == 2) IC_CD(2, false);
        else IC_CD(1, false);
    }
#undef IC_CD
    return hipGetLastError();
}

hipError_t launch_window(hipStream_t st, const double *part, long ss, long sl, const SbPlan &plan, int nsub,
                         int nbin, int width, int32_t *win, int32_t *flags)
{
    if (plan.n < 1 || plan.n > kMaxSbLeaves) return hipErrorInvalidValue;
    const size_t shm = window_lds_bytes(nbin);
    if (shm > kLdsBlockMax) return hipErrorInvalidValue;
    IC_GGL(k_window, dim3(nsub), dim3(kWindowThreads), shm, st, part, ss, sl, plan, nbin, width, win, flags);
    return hipGetLastError();
}

hipError_t launch_base(hipStream_t st, const float *raw, const int32_t *shift, const int32_t *win, const int32_t *flags,
                       int nsub, int nchan, int nbin, int width, float *base, int grid_cap)
{
    const size_t P = (size_t)nsub * nchan;
    const unsigned grid = cap_grid(std::min<size_t>(cdiv(P, 16), 16384), grid_cap);
    if (nbin % 4 == 0 && ((uintptr_t)raw & 15) == 0 && width <= nbin)
        IC_GGL(k_base<true>, dim3(grid), dim3(256), 0, st, raw, shift, win, flags, nsub, nchan, nbin, width, base);
    else
        IC_GGL(k_base<false>, dim3(grid), dim3(256), 0, st, raw, shift, win, flags, nsub, nchan, nbin, width, base);
    return hipGetLastError();
}

hipError_t launch_fscrunch(hipStream_t st, const double *part, long ss, long sl, const double *wpart, long wss,
                           long wsl, const SbPlan &plan, int nsub, int nbin, float *F, float *wf)
{
    if (plan.n < 1 || plan.n > kMaxSbLeaves) return hipErrorInvalidValue;
    const int bs = bin_block(nbin);
    IC_GGL(k_fscrunch, dim3(cdiv(nbin, bs), nsub), dim3(bs), 0, st, part, ss, sl, wpart, wss, wsl, plan,
                       nbin, F, wf);
    return hipGetLastError();
}

hipError_t launch_sb_tree(hipStream_t st, const double *part, const double *wpart, const SbPlan &plan, int nsub,
                          int nbin, long ostr, double *out)
{
    if (plan.n < 1 || plan.n > kMaxSbLeaves) return hipErrorInvalidValue;
    if (ostr < nbin + (wpart ? 1 : 0)) return hipErrorInvalidValue;
    const int bs = bin_block(nbin);
    IC_GGL(k_sb_tree, dim3(cdiv(nbin, bs), nsub), dim3(bs), 0, st, part, wpart, plan, nbin, ostr, out);
    return hipGetLastError();
}

hipError_t launch_tscrunch(hipStream_t st, const float *F, const float *wf, int nsub, int nbin, float *T,
                           double *T64, double *T2)
{
    IC_GGL(k_tscrunch, dim3(cdiv(nbin, 64)), dim3(64), 0, st, F, wf, nsub, nbin, T, T64, T2);
    return hipGetLastError();
}

}  // namespace icgpu
