// ic_hotbins.hip -- opt-in hot-bin repair (ic_set_hotbins): before the loop
// reads an uploaded cube, the off-pulse bins of every profile are clipped
// against their median and MAD, and the few bins that stand out are set to the
// median of the bins that stay.  The written definition is
// iterative_cleaner_amd/hotbins.py; the kernels follow it bit for bit.
//
// Build: as the other units (-ffp-contract=off is load-bearing: lim =
// threshold * (1.4826 * mad) is two separately rounded f64 multiplies).
//
// Kernels (once per upload, before prepare; the cube is still row-major
// [P][nbin] whatever layout the fit cube takes later):
//   k_hotbins<W, NV>  detect and repair.  A profile sits in the registers of a
//                     group of W waves, NV samples per lane: one wave up to
//                     1024 bins (four independent waves per block), a block of
//                     2, 4 or 8 waves up to 8192.  One predicated read of the
//                     off-pulse samples, then count[k], the profile's bit mask
//                     (only where count > 0) and the repaired bins are written.
//   k_hotbin_sums,    offs[k] = the positive counts before k, in profile order,
//   k_hotbin_scan     and their total (blocks of 1024 profiles, integer adds)
//   k_hotbin_fill     bins[offs[k] ..) = the set bits of profile k, ascending:
//                     the list comes out ordered by (profile, bin), no atomics
//
// Medians are exact order statistics on order-preserving integer keys (u32 of
// the f32 samples, the u64 bit patterns of the non-negative f64 deviations),
// as the line statistics' are (ic_linestats.hip: key64 and its radix select on
// keys in LDS; that unit's device functions are not linkable from here, the
// library is built without relocatable device code).  With the keys in
// registers the select here walks the key's bits from the top, one compare
// and one scalar population count per sample and bit, and visits only the bits
// on which the live keys differ (the low mantissa bits of the deviations of f32
// data are all zero).
#include <algorithm>
#include <math.h>

#include "ic_wave.h"

namespace icgpu {

namespace {

typedef unsigned long long u64;

__device__ __forceinline__ uint32_t hot_key32(float v)
{
    const uint32_t b = __float_as_uint(v);
    return (b >> 31) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float hot_unkey32(uint32_t k)
{
    return __uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k);
}

// a wave-uniform value into scalar registers
__device__ __forceinline__ uint32_t hot_uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ u64 hot_uni(u64 v)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ int hot_clz(uint32_t v) { return __clz((int)v); }
__device__ __forceinline__ int hot_clz(u64 v) { return __clzll((long long)v); }

template <typename K> __device__ __forceinline__ K hot_wave_or(K v)
{
    for (int off = 32; off > 0; off >>= 1) v |= __shfl_xor(v, off);
    return v;
}
template <typename K> __device__ __forceinline__ K hot_wave_and(K v)
{
    for (int off = 32; off > 0; off >>= 1) v &= __shfl_xor(v, off);
    return v;
}
template <typename K> __device__ __forceinline__ K hot_wave_min(K v)
{
    for (int off = 32; off > 0; off >>= 1) {
        const K o = __shfl_xor(v, off);
        v = o < v ? o : v;
    }
    return v;
}

// Reductions over the W waves that hold one profile.  Every call is one
// barrier: the slots alternate between two halves, so a wave that runs ahead
// into the next call writes the other half, and it reaches the half read here
// again only behind the next call's barrier, which no wave passes before every
// wave has finished reading.  W == 1: nothing to do (and no LDS).
template <int W> struct HotGrp {
    u64 *s;   // [2][2 W]
    int wave, lane, par;
    __device__ __forceinline__ u64 *slots()
    {
        u64 *b = s + par * 2 * W;
        par ^= 1;
        return b;
    }
    // v wave-uniform
    __device__ __forceinline__ int sum(int v)
    {
        if (W == 1) return v;
        u64 *b = slots();
        if (lane == 0) b[wave] = (u64)(uint32_t)v;
        __syncthreads();
        int r = 0;
#pragma unroll
        for (int i = 0; i < W; ++i) r += (int)(uint32_t)b[i];
        return r;
    }
    __device__ __forceinline__ void or_and(u64 &o, u64 &n)
    {
        if (W == 1) return;
        u64 *b = slots();
        if (lane == 0) {
            b[wave] = o;
            b[W + wave] = n;
        }
        __syncthreads();
        o = b[0];
        n = b[W];
#pragma unroll
        for (int i = 1; i < W; ++i) {
            o |= b[i];
            n &= b[W + i];
        }
    }
    __device__ __forceinline__ u64 min(u64 v)
    {
        if (W == 1) return v;
        u64 *b = slots();
        if (lane == 0) b[wave] = v;
        __syncthreads();
        u64 r = b[0];
#pragma unroll
        for (int i = 1; i < W; ++i) r = b[i] < r ? b[i] : r;
        return r;
    }
};

// r-th smallest (0-based) of the live keys; at least r + 1 keys are live.  A
// sample that is not live (on-pulse, past nbin, or flagged) holds the key ~0,
// which no finite sample and no finite deviation maps to, so a plain "key <
// threshold" never counts it: per bit and sample one compare into a scalar
// mask, one scalar population count.  The bits every live key shares are taken
// as they are; the others are decided from the top: the bit is set iff fewer
// than r + 1 keys lie below (prefix | bit).  Uniform.
template <int W, int NV, typename K>
__device__ __forceinline__ K hot_select(const K (&key)[NV], unsigned live, int r, HotGrp<W> &g)
{
    constexpr int kBits = 8 * (int)sizeof(K);
    K o = 0, n = ~(K)0;
#pragma unroll
    for (int q = 0; q < NV; ++q)
        if ((live >> q) & 1u) {
            o |= key[q];
            n &= key[q];
        }
    u64 o64 = (u64)hot_wave_or(o), n64 = (u64)hot_wave_and(n);
    g.or_and(o64, n64);
    K diff = hot_uni((K)(o64 ^ n64));      // the bits on which live keys differ
    K prefix = hot_uni((K)n64) & ~diff;    // the bits they share
    while (diff) {
        const int b = kBits - 1 - hot_clz(diff);
        const K bit = (K)1 << b;
        const K t = prefix | bit;
        int below = 0;   // live keys under the threshold
#pragma unroll
        for (int q = 0; q < NV; ++q) below += __popcll(__ballot(key[q] < t));
        below = g.sum(below);
        if (r >= below) prefix = t;
        diff &= ~bit;
    }
    return prefix;
}

// the two middle keys of an even count n (ranks n/2 - 1 and n/2), or the middle
// one twice for an odd n
template <int W, int NV, typename K>
__device__ __forceinline__ void hot_middle(const K (&key)[NV], unsigned live, int n, HotGrp<W> &g, K &klo, K &khi)
{
    const int idx = n / 2;
    if (n & 1) {
        klo = khi = hot_select<W, NV, K>(key, live, idx, g);
        return;
    }
    klo = hot_select<W, NV, K>(key, live, idx - 1, g);
    // rank idx: klo again if it is repeated, else the next larger key (klo < ~0:
    // the keys that are not live are never "<= klo", and they are the largest)
    int le = 0;
    K nxt = ~(K)0;
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        le += __popcll(__ballot(key[q] <= klo));
        if (key[q] > klo && key[q] < nxt) nxt = key[q];
    }
    le = g.sum(le);
    nxt = hot_uni((K)g.min((u64)hot_wave_min(nxt)));
    khi = le > idx ? klo : nxt;
}

// median of f64(x_j) over the live samples: (a + b) * 0.5 for an even count
template <int W, int NV>
__device__ __forceinline__ double hot_median_x(const uint32_t (&kx)[NV], unsigned live, int n, HotGrp<W> &g)
{
    uint32_t klo, khi;
    hot_middle<W, NV, uint32_t>(kx, live, n, g, klo, khi);
    if (n & 1) return (double)hot_unkey32(klo);
    return ((double)hot_unkey32(klo) + (double)hot_unkey32(khi)) * 0.5;
}

constexpr int kHotWaveGroups = 4;   // W == 1: independent waves (profiles) per block

}  // namespace

template <int W, int NV>
__global__ __launch_bounds__(W == 1 ? 64 * kHotWaveGroups : 64 * W) void k_hotbins(HotBinArgs a)
{
    __shared__ u64 red[W == 1 ? 1 : 4 * W];
    const int lane = threadIdx.x & 63;
    const int wave = W == 1 ? 0 : (int)(threadIdx.x >> 6);           // the wave within its profile's group
    const int grp = W == 1 ? (int)(threadIdx.x >> 6) : 0;            // the group within the block
    constexpr int kGroups = W == 1 ? kHotWaveGroups : 1;
    const int tig = wave * 64 + lane;                                // thread within the group
    HotGrp<W> g{red, wave, lane, 0};
    const int nbin = a.nbin, words = (nbin + 31) >> 5;
    const int n_off = nbin - a.win_len, cap = n_off / 4;
    for (long k = (long)blockIdx.x * kGroups + grp; k < a.P; k += (long)gridDim.x * kGroups) {
        // the profile's offset o, then bin j is on-pulse iff ((j - o) mod nbin - start) mod nbin < len
        const long oi = a.per_profile ? k : k % a.nchan;
        long long ov = 0;
        if (a.off32)
            ov = a.off32[oi];
        else if (a.offd)
            ov = (long long)rint(a.offd[oi]);
        int o = (int)(ov % nbin);
        if (o < 0) o += nbin;
        float *row = a.cube + (size_t)k * nbin;
        uint32_t kx[NV];   // the live samples as keys (hot_unkey32 gives them back), ~0 elsewhere
        unsigned live = 0;
        int bad = 0;
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            const int j = q * 64 * W + tig;
            int t = j - o;
            if (t < 0) t += nbin;
            t -= a.win_start;
            if (t < 0) t += nbin;
            const bool off = j < nbin && t >= a.win_len;
            const float x = off ? row[j] : 0.0f;
            kx[q] = off ? hot_key32(x) : ~0u;
            live |= (unsigned)off << q;
            bad |= off && !isfinite(x);
        }
        const bool skip = a.w0[k] == 0.0f || g.sum(__any(bad) ? 1 : 0) != 0;
        unsigned hot = 0;
        int nflag = 0;
        if (!skip) {
            int nlive = n_off;
            for (int r = 0; r < a.rounds; ++r) {
                const double m = hot_median_x<W, NV>(kx, live, nlive, g);
                u64 kd[NV];   // the live deviations: non-negative, so the bit pattern orders them
#pragma unroll
                for (int q = 0; q < NV; ++q)
                    kd[q] = ((live >> q) & 1u) ? (u64)__double_as_longlong(fabs((double)hot_unkey32(kx[q]) - m))
                                               : ~0ull;
                u64 dlo, dhi;
                hot_middle<W, NV, u64>(kd, live, nlive, g, dlo, dhi);
                const double a0 = __longlong_as_double((long long)dlo), a1 = __longlong_as_double((long long)dhi);
                const double mad = (nlive & 1) ? a0 : (a0 + a1) * 0.5;
                if (mad == 0.0) break;
                const double s = 1.4826 * mad;
                const double lim = a.threshold * s;
                unsigned nh = 0;
                int c = 0;
#pragma unroll
                for (int q = 0; q < NV; ++q) {
                    const bool h = ((live >> q) & 1u) && __longlong_as_double((long long)kd[q]) > lim;
                    nh |= (unsigned)h << q;
                    c += __popcll(__ballot(h));
                }
                c = g.sum(c);
                if (c == 0) break;
                live &= ~nh;
                hot |= nh;
                nflag += c;
                nlive -= c;
#pragma unroll
                for (int q = 0; q < NV; ++q)
                    if ((nh >> q) & 1u) kx[q] = ~0u;
                if (nflag > cap) break;
            }
            if (nflag > 0 && nflag <= cap) {
                // the survivors' median, recomputed after the last removal
                const float fill = (float)hot_median_x<W, NV>(kx, live, nlive, g);
#pragma unroll
                for (int q = 0; q < NV; ++q) {
                    const int j = q * 64 * W + tig;
                    if ((hot >> q) & 1u) row[j] = fill;
                    // the profile's mask, every word of it: 64 bins of a wave are two words
                    const u64 hb = __ballot((hot >> q) & 1u);
                    const int w0 = (q * 64 * W + wave * 64) >> 5;
                    if (lane < 2 && w0 + lane < words)
                        a.mask[(size_t)k * words + w0 + lane] = (uint32_t)(hb >> (32 * lane));
                }
            }
        }
        if (tig == 0) a.count[k] = nflag > cap ? -1 : nflag;
    }
}

// The row starts, in two launches over blocks of 1024 profiles (a thread per
// profile).  k_hotbin_sums: block b's sum of positive counts -> part[b].
// k_hotbin_scan: block b adds up part[0 .. b) (every block for itself: at most
// a few thousand words from L2), scans its own 1024 counts and writes their
// starts; the last block also writes the total.  Integer adds: the same
// offsets however the blocks are scheduled.
constexpr int kHotScanThreads = 1024;
__device__ __forceinline__ long long hot_block_sum(long long v, long long *sh)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();   // sh may still be read from a call before
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    long long r = 0;
#pragma unroll
    for (int i = 0; i < kHotScanThreads / 64; ++i) r += sh[i];
    return r;
}
__global__ __launch_bounds__(kHotScanThreads) void k_hotbin_sums(const int32_t *__restrict__ count, long P,
                                                                 long long *__restrict__ part)
{
    __shared__ long long sh[kHotScanThreads / 64];
    const long k = (long)blockIdx.x * kHotScanThreads + threadIdx.x;
    const int32_t c = k < P ? count[k] : 0;
    const long long s = hot_block_sum(c > 0 ? c : 0, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}
__global__ __launch_bounds__(kHotScanThreads) void k_hotbin_scan(const int32_t *__restrict__ count, long P,
                                                                 const long long *__restrict__ part,
                                                                 int64_t *__restrict__ offs,
                                                                 int64_t *__restrict__ total)
{
    __shared__ long long sh[kHotScanThreads / 64];
    __shared__ long long wsum[kHotScanThreads / 64];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    long long before = 0;
    for (long b = t; b < (long)blockIdx.x; b += kHotScanThreads) before += part[b];
    before = hot_block_sum(before, sh);
    const long k = (long)blockIdx.x * kHotScanThreads + t;
    const int32_t c = k < P ? count[k] : 0;
    const long long v = c > 0 ? c : 0;
    long long incl = v;   // inclusive scan over the wave, then over the 16 waves
    for (int off = 1; off < 64; off <<= 1) {
        const long long u = __shfl_up(incl, off);
        if (lane >= off) incl += u;
    }
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    long long wbase = 0;
    for (int i = 0; i < wv; ++i) wbase += wsum[i];
    if (k < P) offs[k] = before + wbase + (incl - v);
    if (k == P - 1) *total = before + wbase + incl;
}

// A wave looks at 64 profiles' counts at once and then writes the rows of
// those that have one, a row per pass: lane l takes mask word l, l + 64, ...,
// and its bits go behind those of the lower lanes.
__global__ __launch_bounds__(256) void k_hotbin_fill(const int32_t *__restrict__ count,
                                                     const uint32_t *__restrict__ mask,
                                                     const int64_t *__restrict__ offs, long P, int nbin,
                                                     int32_t *__restrict__ bins, int64_t cap)
{
    const int lane = threadIdx.x & 63;
    const long nw = (long)gridDim.x * (blockDim.x >> 6);
    const long w = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int words = (nbin + 31) >> 5;
    for (long k0 = w * 64; k0 < P; k0 += nw * 64) {
        const long kk = k0 + lane;
        u64 have = __ballot(kk < P && count[kk] > 0);
        while (have) {
            const int l = __ffsll((long long)have) - 1;
            have &= have - 1;
            const long k = k0 + l;
            long long pos = offs[k];
            for (int wb = 0; wb < words; wb += 64) {
                const int wi = wb + lane;
                uint32_t bits = wi < words ? mask[(size_t)k * words + wi] : 0u;
                const int c = __popc(bits);
                int incl = c;
                for (int off = 1; off < 64; off <<= 1) {
                    const int v = __shfl_up(incl, off);
                    if (lane >= off) incl += v;
                }
                long long p = pos + (incl - c);
                while (bits) {
                    const int b = __ffs((int)bits) - 1;
                    bits &= bits - 1;
                    if (p < cap) bins[p] = wi * 32 + b;
                    ++p;
                }
                pos += __shfl(incl, 63);
            }
        }
    }
}

// ============================================================ launchers

template <int W, int NV> static hipError_t launch_hotbins_w(hipStream_t st, const HotBinArgs &a)
{
    constexpr int kGroups = W == 1 ? kHotWaveGroups : 1;
    const unsigned grid = cap_grid(std::min<size_t>(cdiv((size_t)a.P, kGroups), 256 * 16), a.grid_cap);
    IC_GGL((k_hotbins<W, NV>), dim3(grid), dim3(64 * W * kGroups), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_hotbins(hipStream_t st, const HotBinArgs &a)
{
    if (!a.cube || !a.w0 || !a.count || !a.mask || a.P < 1 || a.nchan < 1 || a.nbin < kHotMinOff ||
        a.nbin > kHotMaxBin || a.win_start < 0 || a.win_start >= a.nbin || a.win_len < 0 ||
        a.nbin - a.win_len < kHotMinOff || !(a.threshold > 0.0) || a.rounds < 1 || a.rounds > kHotMaxRounds)
        return hipErrorInvalidValue;
    const int n = a.nbin;
    if (n <= 128) return launch_hotbins_w<1, 2>(st, a);
    if (n <= 256) return launch_hotbins_w<1, 4>(st, a);
    if (n <= 512) return launch_hotbins_w<1, 8>(st, a);
    if (n <= 1024) return launch_hotbins_w<1, 16>(st, a);
    if (n <= 2048) return launch_hotbins_w<2, 16>(st, a);
    if (n <= 4096) return launch_hotbins_w<4, 16>(st, a);
    return launch_hotbins_w<8, 16>(st, a);
}

size_t hotbin_scan_parts(long P) { return (size_t)cdiv((size_t)P, kHotScanThreads); }

hipError_t launch_hotbin_scan(hipStream_t st, const int32_t *count, long P, int64_t *part, int64_t *offs,
                              int64_t *total)
{
    if (!count || !part || !offs || !total || P < 1) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)hotbin_scan_parts(P);
    IC_GGL(k_hotbin_sums, dim3(grid), dim3(kHotScanThreads), 0, st, count, P, (long long *)part);
    IC_GGL(k_hotbin_scan, dim3(grid), dim3(kHotScanThreads), 0, st, count, P, (const long long *)part, offs, total);
    return hipGetLastError();
}

hipError_t launch_hotbin_fill(hipStream_t st, const int32_t *count, const uint32_t *mask, const int64_t *offs, long P,
                              int nbin, int32_t *bins, int64_t cap, int grid_cap)
{
    if (!count || !mask || !offs || !bins || P < 1 || nbin < 1 || cap < 0) return hipErrorInvalidValue;
    const unsigned grid = cap_grid(std::min<size_t>(cdiv((size_t)P, 256), 2048), grid_cap);
    IC_GGL(k_hotbin_fill, dim3(grid), dim3(256), 0, st, count, mask, offs, P, nbin, bins, cap);
    return hipGetLastError();
}

}  // namespace icgpu
