// ic_linestats.hip -- per channel / subint median and MAD (ic.py:229-256) and
// the combine step (ic.py:221-225, :303-305, :127-141), with their launchers,
// and the opt-in detrended forms of both (k_linetrend, k_combine_dt; detrend.py),
// whole-line and piecewise (k_linetrend_pw, k_combine_pw).
// The non-inlined wave_* / grp_* selection functions live here with all
// their callers.
#include <algorithm>
#include <float.h>
#include <math.h>

#include "ic_wave.h"

namespace icgpu {

// ============================================================ medians

__device__ __forceinline__ unsigned long long key64(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double unkey64(unsigned long long k)
{
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}

// ---- per-line median / MAD: one wave per line, radix select ------------------
// Lines: columns (length nsub) of each diagnostic, or rows (length nchan);
// diag 0 std, 1 mean, 2 ptp (f32 arithmetic), 3 fft (plain: every entry valid).
// The valid values of the line go to wave-private LDS as order-preserving
// 64-bit keys (key64), compacted with a ballot.  Order statistics come from a
// most-significant-digit radix select: 8-bit digits from the highest bit where min and max differ,
// a 256-bin LDS histogram per digit, the target bin found by a DPP prefix scan.
// Once the chosen bin holds a single key, one compare-only scan returns it.
// numpy.ma median arithmetic: odd -> 0+mid, even -> ((0+lo)+hi)/2 in the
// dtype; any NaN -> NaN.

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v)
{
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v)
{
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off);
        v = o > v ? o : v;
    }
    return v;
}
__device__ __forceinline__ int wave_sum_i(int v)
{
    return wave_tree<64>(v, OpAdd());
}

// inclusive prefix sum over the 64 lanes (DPP row shifts + row broadcasts)
__device__ __forceinline__ int wave_incl_scan(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true);   // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, true);   // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, true);   // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, true);   // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);  // row_bcast:15 -> rows 1, 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);  // row_bcast:31 -> rows 2, 3
    return v;
}

// r-th smallest (0-based) of keys[0, n): uniform result
__device__ unsigned long long wave_select(const unsigned long long *keys, int n, int r, unsigned *hist, int lane)
{
    unsigned long long lo = ~0ull, hi = 0ull;
    for (int j = lane; j < n; j += 64) {
        const unsigned long long k = keys[j];
        lo = k < lo ? k : lo;
        hi = k > hi ? k : hi;
    }
    lo = wave_min_u64(lo);
    hi = wave_max_u64(hi);
    if (lo == hi) return lo;
    const int top = 63 - __clzll((long long)(lo ^ hi));
    int shift = (top / 8) * 8;
    unsigned long long prefix = shift + 8 >= 64 ? 0ull : (lo & (~0ull << (shift + 8)));
    for (; shift >= 0; shift -= 8) {
        const unsigned long long hmask = shift + 8 >= 64 ? 0ull : (~0ull << (shift + 8));
#pragma unroll
        for (int q = 0; q < 4; ++q) hist[lane * 4 + q] = 0u;
        wave_sync();
        for (int j = lane; j < n; j += 64) {
            const unsigned long long k = keys[j];
            if ((k & hmask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
        }
        wave_sync();
        const uint4 c4 = *(const uint4 *)&hist[lane * 4];
        const int sl = (int)(c4.x + c4.y + c4.z + c4.w);
        const int incl = wave_incl_scan(sl);
        const unsigned long long over = __ballot(incl > r);
        const int L = __ffsll((long long)over) - 1;   // lane holding the target bin
        int below = __shfl(incl - sl, L);
        const uint4 cl = *(const uint4 *)&hist[L * 4];
        int bin = L * 4;
        unsigned cb = cl.x;   // keys in the chosen bin
        if (r - below >= (int)cl.x) {
            below += cl.x;
            ++bin;
            cb = cl.y;
            if (r - below >= (int)cl.y) {
                below += cl.y;
                ++bin;
                cb = cl.z;
                if (r - below >= (int)cl.z) {
                    below += cl.z;
                    ++bin;
                    cb = cl.w;
                }
            }
        }
        r -= below;
        prefix |= (unsigned long long)bin << shift;
        if (cb == 1u && shift > 0) {   // a single key holds the prefix: one compare-only scan
            // one key left under the prefix: it is the answer, found in one
            // compare-only scan instead of the remaining digit passes
            const unsigned long long m = ~0ull << shift;
            unsigned long long f = 0ull;
            for (int j = lane; j < n; j += 64) {
                const unsigned long long k = keys[j];
                if ((k & m) == prefix) f = k;
            }
            return wave_max_u64(f);
        }
        wave_sync();
    }
    return prefix;
}

// median of keys[0, n) (n > 0, no NaN), dtype arithmetic
__device__ double wave_median(const unsigned long long *keys, int n, bool f32, unsigned *hist, int lane)
{
    const int idx = n / 2;
    if (n % 2) {
        const double m = unkey64(wave_select(keys, n, idx, hist, lane));
        return f32 ? (double)(0.0f + (float)m) : 0.0 + m;
    }
    const unsigned long long klo = wave_select(keys, n, idx - 1, hist, lane);
    // hi = rank idx: klo again if it is repeated, else the next larger key
    int le = 0;
    unsigned long long nxt = ~0ull;
    for (int j = lane; j < n; j += 64) {
        const unsigned long long k = keys[j];
        le += k <= klo;
        if (k > klo && k < nxt) nxt = k;
    }
    le = wave_sum_i(le);
    nxt = wave_min_u64(nxt);
    const unsigned long long khi = le > idx ? klo : nxt;
    const double lo = unkey64(klo), hi = unkey64(khi);
    if (f32) {
        const float t = (0.0f + (float)lo) + (float)hi;
        return (double)(t / 2.0f);
    }
    const double t = (0.0 + lo) + hi;
    return t / 2.0;
}

__global__ __launch_bounds__(256) void k_linestats(LineStatsArgs a, int rows, int len, int wpb, int per_wave)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lsm[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int line = blockIdx.x * wpb + wave;
    const int nl = 4 * (rows ? a.nsub : a.nchan);
    if (line >= nl || wave >= wpb) return;
    unsigned *hist = (unsigned *)(lsm + (size_t)wave * per_wave);
    unsigned long long *keys = (unsigned long long *)(lsm + (size_t)wave * per_wave + 1024);
    const int nline = rows ? a.nsub : a.nchan;
    const int diag = line / nline, idx = line % nline;
    const bool f32 = diag == 2 && a.ptp_f32, plain = diag == 3;
    // gather the valid values (ballot compaction keeps no particular order: the
    // selection does not need one)
    int cnt = 0, nan = 0;
    for (int q0 = 0; q0 < len; q0 += 64) {
        const int q = q0 + lane;
        double d = 0.0;
        bool v = false;
        if (q < len) {
            const size_t kk = rows ? (size_t)idx * a.nchan + q : (size_t)q * a.nchan + idx;
            v = plain ? true : (a.valid[kk] != 0);
            d = diag == 0 ? a.std_d[kk] : diag == 1 ? a.mean_d[kk] : diag == 2 ? a.ptp_d[kk] : a.fft_d[kk];
        }
        const unsigned long long m = __ballot(v);
        if (v) keys[cnt + __popcll(m & ((1ull << lane) - 1ull))] = key64(d);
        nan |= v && isnan(d);
        cnt += __popcll(m);
    }
    nan = __any(nan);
    wave_sync();
    double med = NAN, mad = NAN;
    if (cnt > 0 && !nan) {
        med = wave_median(keys, cnt, f32, hist, lane);
        // |d - med| in the dtype, in place
        int rnan = 0;
        for (int j = lane; j < cnt; j += 64) {
            const double d = unkey64(keys[j]);
            const double r = f32 ? (double)fabsf((float)d - (float)med) : fabs(d - med);
            rnan |= isnan(r);
            keys[j] = key64(r);
        }
        rnan = __any(rnan);
        wave_sync();
        if (!rnan) mad = wave_median(keys, cnt, f32, hist, lane);
    }
    if (lane == 0) {
        if (!rows) {
            a.col_med[diag * a.nchan + idx] = med;
            a.col_mad[diag * a.nchan + idx] = mad;
        } else {
            a.row_med[diag * a.nsub + idx] = med;
            a.row_mad[diag * a.nsub + idx] = mad;
        }
    }
}

// ---- long lines: W waves per line -------------------------------------------
// The rows (length nchan, a few thousand) are too few for one wave each to fill
// the chip (4*nsub waves), and early radix digits put most keys of a wave in
// one bin, so the LDS atomics serialise.  Here a block of W waves owns a line:
// wave w gathers its own slice of the line into its own key segment, the 256
// bins are shared by the block, and min/max/count/NaN flags are block
// reductions.  Order statistics do not depend on where a key sits, so the
// result is the one k_linestats computes.

template <int W> struct GrpRed {
    unsigned long long *s;   // 2*W slots
    int wave, lane;
    __device__ unsigned long long min_u64(unsigned long long v)
    {
        v = wave_min_u64(v);
        if (lane == 0) s[wave] = v;
        __syncthreads();
        unsigned long long r = s[0];
#pragma unroll
        for (int i = 1; i < W; ++i) r = s[i] < r ? s[i] : r;
        __syncthreads();
        return r;
    }
    __device__ unsigned long long max_u64(unsigned long long v)
    {
        v = wave_max_u64(v);
        if (lane == 0) s[wave] = v;
        __syncthreads();
        unsigned long long r = s[0];
#pragma unroll
        for (int i = 1; i < W; ++i) r = s[i] > r ? s[i] : r;
        __syncthreads();
        return r;
    }
    // min and max in one round trip
    __device__ void minmax_u64(unsigned long long &lo, unsigned long long &hi)
    {
        lo = wave_min_u64(lo);
        hi = wave_max_u64(hi);
        if (lane == 0) {
            s[wave] = lo;
            s[W + wave] = hi;
        }
        __syncthreads();
        lo = s[0];
        hi = s[W];
#pragma unroll
        for (int i = 1; i < W; ++i) {
            lo = s[i] < lo ? s[i] : lo;
            hi = s[W + i] > hi ? s[W + i] : hi;
        }
        __syncthreads();
    }
    __device__ int sum_i(int v) { return sum_uniform(wave_sum_i(v)); }
    // v already uniform across the wave
    __device__ int sum_uniform(int v)
    {
        if (lane == 0) s[wave] = (unsigned long long)(unsigned)v;
        __syncthreads();
        int r = 0;
#pragma unroll
        for (int i = 0; i < W; ++i) r += (int)(unsigned)s[i];
        __syncthreads();
        return r;
    }
};

// r-th smallest (0-based) over every wave's segment keys[0, n): uniform result
template <int W>
__device__ unsigned long long grp_select(GrpRed<W> &g, const unsigned long long *keys, int n, int r, unsigned *hist)
{
    const int lane = g.lane;
    unsigned long long lo = ~0ull, hi = 0ull;
    for (int j = lane; j < n; j += 64) {
        const unsigned long long k = keys[j];
        lo = k < lo ? k : lo;
        hi = k > hi ? k : hi;
    }
    g.minmax_u64(lo, hi);
    if (lo == hi) return lo;
    const int top = 63 - __clzll((long long)(lo ^ hi));
    int shift = (top / 8) * 8;
    unsigned long long prefix = shift + 8 >= 64 ? 0ull : (lo & (~0ull << (shift + 8)));
    for (; shift >= 0; shift -= 8) {
        const unsigned long long hmask = shift + 8 >= 64 ? 0ull : (~0ull << (shift + 8));
        for (int t = threadIdx.x; t < 256; t += 64 * W) hist[t] = 0u;
        __syncthreads();
        for (int j = lane; j < n; j += 64) {
            const unsigned long long k = keys[j];
            if ((k & hmask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
        }
        __syncthreads();
        const uint4 c4 = *(const uint4 *)&hist[lane * 4];
        const int sl = (int)(c4.x + c4.y + c4.z + c4.w);
        const int incl = wave_incl_scan(sl);
        const unsigned long long over = __ballot(incl > r);
        const int L = __ffsll((long long)over) - 1;
        int below = __shfl(incl - sl, L);
        const uint4 cl = *(const uint4 *)&hist[L * 4];
        int bin = L * 4;
        unsigned cb = cl.x;   // keys in the chosen bin
        if (r - below >= (int)cl.x) {
            below += cl.x;
            ++bin;
            cb = cl.y;
            if (r - below >= (int)cl.y) {
                below += cl.y;
                ++bin;
                cb = cl.z;
                if (r - below >= (int)cl.z) {
                    below += cl.z;
                    ++bin;
                    cb = cl.w;
                }
            }
        }
        r -= below;
        prefix |= (unsigned long long)bin << shift;
        if (cb == 1u && shift > 0) {   // uniform: every wave read the same bins
            const unsigned long long m = ~0ull << shift;
            unsigned long long f = 0ull;
            for (int j = lane; j < n; j += 64) {
                const unsigned long long k = keys[j];
                if ((k & m) == prefix) f = k;
            }
            return g.max_u64(f);   // its barriers also order the bin reads before any re-zeroing
        }
        __syncthreads();   // every wave has read the bins before the next zeroing
    }
    return prefix;
}

// median over the block's keys (ntot > 0 in total, no NaN), dtype arithmetic
template <int W>
__device__ double grp_median(GrpRed<W> &g, const unsigned long long *keys, int n, int ntot, bool f32, unsigned *hist)
{
    const int idx = ntot / 2;
    if (ntot % 2) {
        const double m = unkey64(grp_select<W>(g, keys, n, idx, hist));
        return f32 ? (double)(0.0f + (float)m) : 0.0 + m;
    }
    const unsigned long long klo = grp_select<W>(g, keys, n, idx - 1, hist);
    int le = 0;
    unsigned long long nxt = ~0ull;
    for (int j = g.lane; j < n; j += 64) {
        const unsigned long long k = keys[j];
        le += k <= klo;
        if (k > klo && k < nxt) nxt = k;
    }
    le = g.sum_i(le);
    nxt = g.min_u64(nxt);
    const unsigned long long khi = le > idx ? klo : nxt;
    const double lo = unkey64(klo), hi = unkey64(khi);
    if (f32) {
        const float t = (0.0f + (float)lo) + (float)hi;
        return (double)(t / 2.0f);
    }
    const double t = (0.0 + lo) + hi;
    return t / 2.0;
}

// one block of W waves per line; LDS: 256 bins, 2*W reduction slots, len keys
template <int W> __global__ __launch_bounds__(64 * W) void k_linestats_grp(LineStatsArgs a, int rows, int len)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lsm[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned *hist = (unsigned *)lsm;
    GrpRed<W> g{(unsigned long long *)(lsm + 1024), wave, lane};
    const int nline = rows ? a.nsub : a.nchan;
    const int line = blockIdx.x;
    const int diag = line / nline, idx = line % nline;
    const bool f32 = diag == 2 && a.ptp_f32, plain = diag == 3;
    const int seg = (((len + W - 1) / W) + 63) & ~63;
    const int q0w = wave * seg, q1w = min(len, q0w + seg);
    unsigned long long *keys = (unsigned long long *)(lsm + 1024 + 16 * W) + q0w;
    int cnt = 0, nan = 0;
    for (int q0 = q0w; q0 < q1w; q0 += 64) {
        const int q = q0 + lane;
        double d = 0.0;
        bool v = false;
        if (q < q1w) {
            const size_t kk = rows ? (size_t)idx * a.nchan + q : (size_t)q * a.nchan + idx;
            v = plain ? true : (a.valid[kk] != 0);
            d = diag == 0 ? a.std_d[kk] : diag == 1 ? a.mean_d[kk] : diag == 2 ? a.ptp_d[kk] : a.fft_d[kk];
        }
        const unsigned long long m = __ballot(v);
        if (v) keys[cnt + __popcll(m & ((1ull << lane) - 1ull))] = key64(d);
        nan |= v && isnan(d);
        cnt += __popcll(m);
    }
    nan = g.sum_uniform(__any(nan) ? 1 : 0);   // the barrier also publishes the keys
    const int ntot = g.sum_uniform(cnt);
    double med = NAN, mad = NAN;
    if (ntot > 0 && !nan) {
        med = grp_median<W>(g, keys, cnt, ntot, f32, hist);
        int rnan = 0;
        for (int j = lane; j < cnt; j += 64) {
            const double d = unkey64(keys[j]);
            const double r = f32 ? (double)fabsf((float)d - (float)med) : fabs(d - med);
            rnan |= isnan(r);
            keys[j] = key64(r);
        }
        rnan = g.sum_uniform(__any(rnan) ? 1 : 0);
        if (!rnan) mad = grp_median<W>(g, keys, cnt, ntot, f32, hist);
    }
    if (threadIdx.x == 0) {
        if (!rows) {
            a.col_med[diag * a.nchan + idx] = med;
            a.col_mad[diag * a.nchan + idx] = mad;
        } else {
            a.row_med[diag * a.nsub + idx] = med;
            a.row_mad[diag * a.nsub + idx] = mad;
        }
    }
}

// ============================================================ detrended scaling
// Opt-in (ic_set_detrend; iterative_cleaner_amd/detrend.py is the definition,
// followed here operation by operation): a polynomial trend of order k <= 3 is
// fitted to every line with clipping rounds, and the line's median and MAD are
// those of d' = dtype(f64(d) - p(x)).  k_combine_dt forms the same d' per entry
// with the same function (detrend_value).

struct TrendCoef {
    double a0, a1, a2, a3;
};

__device__ __forceinline__ double trend_x(int j, int n)
{
    return n == 1 ? 0.0 : (double)(2 * j - (n - 1)) / (double)(n - 1);
}
// p(x) by Horner from a_k
__device__ __forceinline__ double trend_poly(double x, const TrendCoef &c, int k)
{
    double t = k >= 3 ? c.a3 : k == 2 ? c.a2 : k == 1 ? c.a1 : c.a0;
    if (k >= 3) t = t * x + c.a2;
    if (k >= 2) t = t * x + c.a1;
    if (k >= 1) t = t * x + c.a0;
    return t;
}
// d' of a valid entry j of a line of n values: dtype(f64(d) - p(x_j)), the
// dtype's value held in a double (d holds an f32 value when f32)
__device__ __forceinline__ double detrend_value(double d, bool f32, int j, int n, const TrendCoef &c, int k)
{
    const double r = d - trend_poly(trend_x(j, n), c, k);
    return f32 ? (double)(float)r : r;
}

__device__ __forceinline__ double line_value(const LineStatsArgs &a, int diag, size_t kk)
{
    return diag == 0 ? a.std_d[kk] : diag == 1 ? a.mean_d[kk] : diag == 2 ? a.ptp_d[kk] : a.fft_d[kk];
}

// the chains' halving tree and the elimination, below both fits: S, B hold a
// lane's chain on entry.  false: a refused pivot
template <int K> __device__ __forceinline__ bool trend_solve(double (&S)[2 * K + 1], double (&B)[K + 1], TrendCoef &out);

// one fit of order K over the entries of `use` (bit j of use[j / 64]): the 64
// chains are the wave's lanes, whatever the block's wave count (every wave of
// the block computes the same sums).  false: the trend is zero.
template <int K>
__device__ bool trend_fit(const LineStatsArgs &a, int diag, int rows, int idx, int len,
                          const unsigned long long *use, int lane, TrendCoef &out)
{
    double S[2 * K + 1], B[K + 1];
#pragma unroll
    for (int p = 0; p <= 2 * K; ++p) S[p] = 0.0;
#pragma unroll
    for (int p = 0; p <= K; ++p) B[p] = 0.0;
    for (int q0 = 0; q0 < len; q0 += 64) {
        const int j = q0 + lane;
        const unsigned long long w = use[q0 >> 6];
        if (j < len && ((w >> lane) & 1ull)) {
            const size_t kk = rows ? (size_t)idx * a.nchan + j : (size_t)j * a.nchan + idx;
            const double x = trend_x(j, len), y = line_value(a, diag, kk);
            double xp = 1.0;
#pragma unroll
            for (int p = 0; p <= 2 * K; ++p) {
                S[p] = S[p] + xp;
                if (p <= K) B[p] = B[p] + xp * y;
                xp = xp * x;
            }
        }
    }
    return trend_solve<K>(S, B, out);
}

// the statement's piecewise fit of one piece [b, b + L) of a line: trend_fit on
// the piece's own abscissa, the 64 chains by the local index i = j - b.  false:
// the piece is retired (<= K members, or a refused pivot).
template <int K>
__device__ bool piece_fit(const LineStatsArgs &a, int diag, int rows, int idx, int b, int L,
                          const unsigned long long *use, int lane, TrendCoef &out)
{
    double S[2 * K + 1], B[K + 1];
#pragma unroll
    for (int p = 0; p <= 2 * K; ++p) S[p] = 0.0;
#pragma unroll
    for (int p = 0; p <= K; ++p) B[p] = 0.0;
    int members = 0;
    for (int i0 = 0; i0 < L; i0 += 64) {
        const int i = i0 + lane, j = b + i;
        const bool in = i < L && ((use[j >> 6] >> (j & 63)) & 1ull);
        members += __popcll(__ballot(in));
        if (in) {
            const size_t kk = rows ? (size_t)idx * a.nchan + j : (size_t)j * a.nchan + idx;
            const double x = trend_x(i, L), y = line_value(a, diag, kk);
            double xp = 1.0;
#pragma unroll
            for (int p = 0; p <= 2 * K; ++p) {
                S[p] = S[p] + xp;
                if (p <= K) B[p] = B[p] + xp * y;
                xp = xp * x;
            }
        }
    }
    if (members <= K) return false;
    return trend_solve<K>(S, B, out);
}

template <int K> __device__ __forceinline__ bool trend_solve(double (&S)[2 * K + 1], double (&B)[K + 1], TrendCoef &out)
{
    // halving tree over the chains: t[l] = t[l] + t[l + h], h = 32 .. 1
#pragma unroll
    for (int p = 0; p <= 2 * K; ++p) {
        double v = S[p];
        for (int h = 32; h > 0; h >>= 1) v = v + __shfl_down(v, h);
        S[p] = __shfl(v, 0);
    }
#pragma unroll
    for (int p = 0; p <= K; ++p) {
        double v = B[p];
        for (int h = 32; h > 0; h >>= 1) v = v + __shfl_down(v, h);
        B[p] = __shfl(v, 0);
    }
    double G[K + 1][K + 1];
#pragma unroll
    for (int p = 0; p <= K; ++p)
#pragma unroll
        for (int q = 0; q <= K; ++q) G[p][q] = S[p + q];
    bool ok = true;
#pragma unroll
    for (int i = 0; i <= K; ++i) {
        const double piv = G[i][i];
        if (!(piv > 0.0 && isfinite(piv))) ok = false;
#pragma unroll
        for (int r = i + 1; r <= K; ++r) {
            const double f = G[r][i] / piv;
#pragma unroll
            for (int c = i + 1; c <= K; ++c) G[r][c] = G[r][c] - f * G[i][c];
            B[r] = B[r] - f * B[i];
        }
    }
    if (!ok) return false;   // (the operations after a refused pivot are discarded)
    double x[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int i = K; i >= 0; --i) {
        double s = B[i];
#pragma unroll
        for (int c = i + 1; c <= K; ++c) s = s - G[i][c] * x[c];
        x[i] = s / G[i][i];
    }
    out = TrendCoef{x[0], x[1], x[2], x[3]};
    return true;
}

// one block of W waves per line (W = 1: one wave per line); LDS: 256 bins,
// 2*W reduction slots, W segments of seg keys, the membership words of the line.
// Every round reads the line again from memory (short and L2-resident); LDS
// holds the selection keys and the membership bits only.
template <int W>
__global__ __launch_bounds__(64 * W) void k_linetrend(LineStatsArgs a, TrendArgs t, int rows, int len)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lsm[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned *hist = (unsigned *)lsm;
    GrpRed<W> g{(unsigned long long *)(lsm + 1024), wave, lane};
    const int nline = rows ? a.nsub : a.nchan;
    const int line = blockIdx.x;
    const int diag = line / nline, idx = line % nline;
    const bool f32 = diag == 2 && a.ptp_f32, plain = diag == 3;
    const int k = rows ? t.subint_order : t.chan_order;
    const int seg = (((len + W - 1) / W) + 63) & ~63;
    const int q0w = min(len, wave * seg), q1w = min(len, q0w + seg);
    unsigned long long *keys = (unsigned long long *)(lsm + 1024 + 16 * W) + (size_t)wave * seg;
    unsigned long long *use = (unsigned long long *)(lsm + 1024 + 16 * W) + (size_t)W * seg;
    const unsigned long long below = (1ull << lane) - 1ull;
    // membership = valid; any valid value not finite: no trend
    int nv = 0, bad = 0;
    for (int q0 = q0w; q0 < q1w; q0 += 64) {
        const int q = q0 + lane;
        bool v = false;
        if (q < q1w) {
            const size_t kk = rows ? (size_t)idx * a.nchan + q : (size_t)q * a.nchan + idx;
            v = plain ? true : (a.valid[kk] != 0);
            bad |= v && !isfinite(line_value(a, diag, kk));
        }
        const unsigned long long m = __ballot(v);
        if (lane == 0) use[q0 >> 6] = m;
        nv += __popcll(m);
    }
    bad = g.sum_uniform(__any(bad) ? 1 : 0);   // the barrier also publishes the membership words
    nv = g.sum_uniform(nv);
    const TrendCoef zero{0.0, 0.0, 0.0, 0.0};
    TrendCoef c = zero;
    if (k > 0 && nv > 0 && !bad) {
        int nuse = nv;
        for (int r = 1; r <= t.rounds; ++r) {
            if (nuse <= k) {
                c = zero;
                break;
            }
            const bool ok = k == 1   ? trend_fit<1>(a, diag, rows, idx, len, use, lane, c)
                            : k == 2 ? trend_fit<2>(a, diag, rows, idx, len, use, lane, c)
                                     : trend_fit<3>(a, diag, rows, idx, len, use, lane, c);
            if (!ok) {
                c = zero;
                break;
            }
            if (r == t.rounds) break;
            // e = y - p(x) over the membership, this wave's slice
            int cnt = 0, nf = 0;
            for (int q0 = q0w; q0 < q1w; q0 += 64) {
                const int q = q0 + lane;
                const bool in = q < q1w && ((use[q0 >> 6] >> lane) & 1ull);
                double e = 0.0;
                if (in) {
                    const size_t kk = rows ? (size_t)idx * a.nchan + q : (size_t)q * a.nchan + idx;
                    e = line_value(a, diag, kk) - trend_poly(trend_x(q, len), c, k);
                }
                const unsigned long long m = __ballot(in);
                if (in) keys[cnt + __popcll(m & below)] = key64(e);
                nf |= in && !isfinite(e);
                cnt += __popcll(m);
            }
            nf = g.sum_uniform(__any(nf) ? 1 : 0);
            if (nf) break;
            const double med = grp_median<W>(g, keys, cnt, nuse, false, hist);
            for (int j = lane; j < cnt; j += 64) keys[j] = key64(fabs(unkey64(keys[j]) - med));
            const double mad = grp_median<W>(g, keys, cnt, nuse, false, hist);
            if (mad == 0.0) break;
            const double lim = t.clip * mad;
            int changed = 0, nn = 0;
            for (int q0 = q0w; q0 < q1w; q0 += 64) {
                const int q = q0 + lane;
                bool in = false;
                if (q < q1w) {
                    const size_t kk = rows ? (size_t)idx * a.nchan + q : (size_t)q * a.nchan + idx;
                    if (plain ? true : (a.valid[kk] != 0)) {
                        const double e = line_value(a, diag, kk) - trend_poly(trend_x(q, len), c, k);
                        in = fabs(e - med) <= lim;
                    }
                }
                const unsigned long long m = __ballot(in);
                changed |= m != use[q0 >> 6];
                if (lane == 0) use[q0 >> 6] = m;   // this wave's words: read by the others after the barrier below
                nn += __popcll(m);
            }
            changed = g.sum_uniform(changed);
            nuse = g.sum_uniform(nn);
            if (!changed) break;
        }
    }
    // median and MAD of d', as k_linestats_grp takes them of d
    int cnt = 0, nan = 0;
    for (int q0 = q0w; q0 < q1w; q0 += 64) {
        const int q = q0 + lane;
        double d = 0.0;
        bool v = false;
        if (q < q1w) {
            const size_t kk = rows ? (size_t)idx * a.nchan + q : (size_t)q * a.nchan + idx;
            v = plain ? true : (a.valid[kk] != 0);
            if (v) d = detrend_value(line_value(a, diag, kk), f32, q, len, c, k);
        }
        const unsigned long long m = __ballot(v);
        if (v) keys[cnt + __popcll(m & below)] = key64(d);
        nan |= v && isnan(d);
        cnt += __popcll(m);
    }
    nan = g.sum_uniform(__any(nan) ? 1 : 0);
    double med = NAN, mad = NAN;
    if (nv > 0 && !nan) {
        med = grp_median<W>(g, keys, cnt, nv, f32, hist);
        int rnan = 0;
        for (int j = lane; j < cnt; j += 64) {
            const double d = unkey64(keys[j]);
            const double r = f32 ? (double)fabsf((float)d - (float)med) : fabs(d - med);
            rnan |= isnan(r);
            keys[j] = key64(r);
        }
        rnan = g.sum_uniform(__any(rnan) ? 1 : 0);
        if (!rnan) mad = grp_median<W>(g, keys, cnt, nv, f32, hist);
    }
    if (threadIdx.x == 0) {
        double *coef = (rows ? t.row_coef : t.col_coef) + ((size_t)diag * nline + idx) * 4;
        coef[0] = c.a0;
        coef[1] = c.a1;
        coef[2] = c.a2;
        coef[3] = c.a3;
        if (!rows) {
            a.col_med[diag * a.nchan + idx] = med;
            a.col_mad[diag * a.nchan + idx] = mad;
        } else {
            a.row_med[diag * a.nsub + idx] = med;
            a.row_mad[diag * a.nsub + idx] = mad;
        }
    }
}

// ---- piecewise detrending (ic_set_detrend_pieces; detrend.py) ------------------
// A direction's lines are cut at the same starts; every piece is fitted on its
// own abscissa, the membership and the stop rules stay the line's.

// entry q of a line: its piece p, its local index i and the piece's length L
struct PieceAt {
    int p, i, L;
};
__device__ __forceinline__ PieceAt piece_at(int q, const int16_t *__restrict__ piece, const int32_t *__restrict__ starts)
{
    const int p = piece[q], b = starts[p];
    return PieceAt{p, q - b, starts[p + 1] - b};
}

// k_linetrend with the fit per piece.  LDS: k_linetrend's, then the line's piece
// coefficients pc[m] and retired flags ret[m].  Piece p is fitted by wave p mod
// W (the chains are that wave's lanes by the local index, so no sum depends on
// W) and published through pc across a barrier; residuals, clipping and d' look
// an entry's piece up in piece_of / starts.
template <int W>
__global__ __launch_bounds__(64 * W) void k_linetrend_pw(LineStatsArgs a, TrendArgs t, PieceArgs pa, int rows, int len)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lsm[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned *hist = (unsigned *)lsm;
    GrpRed<W> g{(unsigned long long *)(lsm + 1024), wave, lane};
    const int nline = rows ? a.nsub : a.nchan;
    const int line = blockIdx.x;
    const int diag = line / nline, idx = line % nline;
    const bool f32 = diag == 2 && a.ptp_f32, plain = diag == 3;
    const int k = rows ? t.subint_order : t.chan_order;
    const int m = rows ? pa.row_np : pa.col_np;
    const int32_t *__restrict__ starts = rows ? pa.row_starts : pa.col_starts;
    const int16_t *__restrict__ piece = rows ? pa.row_piece : pa.col_piece;
    const int seg = (((len + W - 1) / W) + 63) & ~63;
    const int q0w = min(len, wave * seg), q1w = min(len, q0w + seg);
    unsigned long long *keys = (unsigned long long *)(lsm + 1024 + 16 * W) + (size_t)wave * seg;
    unsigned long long *use = (unsigned long long *)(lsm + 1024 + 16 * W) + (size_t)W * seg;
    TrendCoef *pc = (TrendCoef *)(use + (len + 63) / 64);
    unsigned char *ret = (unsigned char *)(pc + m);
    const unsigned long long below = (1ull << lane) - 1ull;
    const TrendCoef zero{0.0, 0.0, 0.0, 0.0};
    for (int p = threadIdx.x; p < m; p += 64 * W) {
        pc[p] = zero;
        ret[p] = 0;
    }
    // membership = valid; any valid value not finite: no trend
    int nv = 0, bad = 0;
    for (int q0 = q0w; q0 < q1w; q0 += 64) {
        const int q = q0 + lane;
        bool v = false;
        if (q < q1w) {
            const size_t kk = rows ? (size_t)idx * a.nchan + q : (size_t)q * a.nchan + idx;
            v = plain ? true : (a.valid[kk] != 0);
            bad |= v && !isfinite(line_value(a, diag, kk));
        }
        const unsigned long long mk = __ballot(v);
        if (lane == 0) use[q0 >> 6] = mk;
        nv += __popcll(mk);
    }
    bad = g.sum_uniform(__any(bad) ? 1 : 0);   // the barrier also publishes the membership words, pc and ret
    nv = g.sum_uniform(nv);
    if (k > 0 && nv > 0 && !bad) {
        int nuse = nv;
        for (int r = 1; r <= t.rounds; ++r) {
            for (int p = wave; p < m; p += W) {
                if (ret[p]) continue;   // this wave's own flag, uniform
                const int b = starts[p], L = starts[p + 1] - b;
                TrendCoef c = zero;   // a retired piece's: piece_fit writes c only when it succeeds
                const bool ok = k == 1   ? piece_fit<1>(a, diag, rows, idx, b, L, use, lane, c)
                                : k == 2 ? piece_fit<2>(a, diag, rows, idx, b, L, use, lane, c)
                                         : piece_fit<3>(a, diag, rows, idx, b, L, use, lane, c);
                if (lane == 0) {
                    pc[p] = c;
                    if (!ok) ret[p] = 1;
                }
            }
            __syncthreads();   // every piece's coefficients of this round
            if (r == t.rounds || nuse == 0) break;
            // e = y - p_q(x) over the membership, this wave's slice
            int cnt = 0, nf = 0;
            for (int q0 = q0w; q0 < q1w; q0 += 64) {
                const int q = q0 + lane;
                const bool in = q < q1w && ((use[q0 >> 6] >> lane) & 1ull);
                double e = 0.0;
                if (in) {
                    const size_t kk = rows ? (size_t)idx * a.nchan + q : (size_t)q * a.nchan + idx;
                    const PieceAt at = piece_at(q, piece, starts);
                    e = line_value(a, diag, kk) - trend_poly(trend_x(at.i, at.L), pc[at.p], k);
                }
                const unsigned long long mk = __ballot(in);
                if (in) keys[cnt + __popcll(mk & below)] = key64(e);
                nf |= in && !isfinite(e);
                cnt += __popcll(mk);
            }
            nf = g.sum_uniform(__any(nf) ? 1 : 0);
            if (nf) break;
            const double med = grp_median<W>(g, keys, cnt, nuse, false, hist);
            for (int j = lane; j < cnt; j += 64) keys[j] = key64(fabs(unkey64(keys[j]) - med));
            const double mad = grp_median<W>(g, keys, cnt, nuse, false, hist);
            if (mad == 0.0) break;
            const double lim = t.clip * mad;
            int changed = 0, nn = 0;
            for (int q0 = q0w; q0 < q1w; q0 += 64) {
                const int q = q0 + lane;
                bool in = false;
                if (q < q1w) {
                    const size_t kk = rows ? (size_t)idx * a.nchan + q : (size_t)q * a.nchan + idx;
                    if (plain ? true : (a.valid[kk] != 0)) {
                        const PieceAt at = piece_at(q, piece, starts);
                        const double e = line_value(a, diag, kk) - trend_poly(trend_x(at.i, at.L), pc[at.p], k);
                        in = fabs(e - med) <= lim;
                    }
                }
                const unsigned long long mk = __ballot(in);
                changed |= mk != use[q0 >> 6];
                if (lane == 0) use[q0 >> 6] = mk;   // this wave's words: read by the others after the barrier below
                nn += __popcll(mk);
            }
            changed = g.sum_uniform(changed);
            nuse = g.sum_uniform(nn);
            if (!changed) break;
        }
    }
    // median and MAD of d', as k_linestats_grp takes them of d
    int cnt = 0, nan = 0;
    for (int q0 = q0w; q0 < q1w; q0 += 64) {
        const int q = q0 + lane;
        double d = 0.0;
        bool v = false;
        if (q < q1w) {
            const size_t kk = rows ? (size_t)idx * a.nchan + q : (size_t)q * a.nchan + idx;
            v = plain ? true : (a.valid[kk] != 0);
            if (v) {
                const PieceAt at = piece_at(q, piece, starts);
                d = detrend_value(line_value(a, diag, kk), f32, at.i, at.L, pc[at.p], k);
            }
        }
        const unsigned long long mk = __ballot(v);
        if (v) keys[cnt + __popcll(mk & below)] = key64(d);
        nan |= v && isnan(d);
        cnt += __popcll(mk);
    }
    nan = g.sum_uniform(__any(nan) ? 1 : 0);
    double med = NAN, mad = NAN;
    if (nv > 0 && !nan) {
        med = grp_median<W>(g, keys, cnt, nv, f32, hist);
        int rnan = 0;
        for (int j = lane; j < cnt; j += 64) {
            const double d = unkey64(keys[j]);
            const double r = f32 ? (double)fabsf((float)d - (float)med) : fabs(d - med);
            rnan |= isnan(r);
            keys[j] = key64(r);
        }
        rnan = g.sum_uniform(__any(rnan) ? 1 : 0);
        if (!rnan) mad = grp_median<W>(g, keys, cnt, nv, f32, hist);
    }
    // the line's coefficients [m][4]; pc is final since the barrier after the last fit
    double *coef = (rows ? t.row_coef : t.col_coef) + ((size_t)diag * nline + idx) * m * 4;
    for (int i = threadIdx.x; i < 4 * m; i += 64 * W) coef[i] = ((const double *)pc)[i];
    if (threadIdx.x == 0) {
        if (!rows) {
            a.col_med[diag * a.nchan + idx] = med;
            a.col_mad[diag * a.nchan + idx] = mad;
        } else {
            a.row_med[diag * a.nsub + idx] = med;
            a.row_mad[diag * a.nsub + idx] = mad;
        }
    }
}

// ============================================================ combine

__device__ __forceinline__ double scale_masked_d(double dv, bool valid, double med, double mad, double thr)
{
    if (!valid) return 0.0 + fabs(dv);
    const double r = dv - med;
    const double q = r / mad;
    const bool dom = !isfinite(q) || (fabs(r) * DBL_MIN >= fabs(mad));
    if (dom) return 0.0 + fabs(0.0 + r);
    const double aq = fabs(q);
    const double res = aq / thr;
    if (!isfinite(res) || aq * DBL_MIN >= fabs(thr)) return 0.0 + aq;
    return res;
}

__device__ __forceinline__ double scale_masked_f(float dv, bool valid, float med, float mad, double thr)
{
    if (!valid) return 0.0 + (double)fabsf(dv);
    const float r = dv - med;
    const float q = r / mad;
    const bool dom = !isfinite(q) || ((double)fabsf(r) * DBL_MIN >= (double)fabsf(mad));
    if (dom) return 0.0 + (double)fabsf(0.0f + r);
    const float aq = fabsf(q);
    const double res = (double)aq / thr;
    if (!isfinite(res) || (double)aq * DBL_MIN >= fabs(thr)) return 0.0 + (double)aq;
    return res;
}

__device__ __forceinline__ double scale_plain(double dv, double med, double mad, double thr)
{
    const double r = dv - med;
    const double q = r / mad;
    return fabs(q) / thr;
}

__device__ __forceinline__ double nanmax2(double a, double b)
{
    if (isnan(a) || isnan(b)) return NAN;
    return a > b ? a : b;
}

// |test - 1| at or below this counts as a near tie (the fftmax tolerance of
// the parity tests, DESIGN.md "Numerical semantics")
constexpr double kNearTie = 1e-9;

// counters: [0] changed vs hist[iter-1], [1] zero weights, [2] profiles whose
// fit status is not 1-4 (info may be null: 0), [3] profiles whose test value
// lies within kNearTie of the zap threshold 1.0 (where the last bits of fftmax,
// not bit-identical to pocketfft, could decide), [4+h] != hist[h]

// TR = TrendView: the detrended form (k_combine_dt): every diagnostic enters its channel's
// scaler as the channel direction's d' and its subint's scaler as the subint
// direction's d' (detrend_value with the line's coefficients; invalid entries
// keep d); the rest is k_combine's.  bdim / gdim: the kernel's blockDim.x /
// gridDim.x, read in the kernel
// TR = PieceView: the piecewise form (k_combine_pw): as TrendView, the d' of an
// entry formed with its piece's coefficients on the piece's abscissa
// TR = ShardTrendView / ShardPieceView: the two on a channel shard
// (k_combine_dt_sh, k_combine_pw_sh; ic_shard_enable_detrend): the shard's nchan
// channels are chan0 .. chan0 + nchan of a subint line of nchan_g, so the subint
// direction's d' of local entry (s, c) is formed at chan0 + c of nchan_g (in
// pieces: looked up there in the full-length table) with the row's gathered
// coefficients; the channel direction is the unsharded one
struct NoTrend {
    static constexpr bool on = false, pieces = false, shard = false;
};
struct TrendView {
    static constexpr bool on = true, pieces = false, shard = false;
    const TrendCoef *col_coef, *row_coef;   // [4][nchan], [4][nsub]
    int chan_order, subint_order;
};
struct PieceView {
    static constexpr bool on = true, pieces = true, shard = false;
    const TrendCoef *col_coef, *row_coef;   // [4][nchan][col_np], [4][nsub][row_np]
    int chan_order, subint_order;
    PieceArgs pa;
};
struct ShardTrendView {
    static constexpr bool on = true, pieces = false, shard = true;
    const TrendCoef *col_coef, *row_coef;   // [4][nchan] (the shard's), [4][nsub]
    int chan_order, subint_order;
    int chan0, nchan_g;
};
struct ShardPieceView {
    static constexpr bool on = true, pieces = true, shard = true;
    const TrendCoef *col_coef, *row_coef;   // [4][nchan][col_np] (the shard's), [4][nsub][row_np]
    int chan_order, subint_order;
    PieceArgs pa;                           // row_starts / row_piece: over nchan_g
    int chan0, nchan_g;
};
template <class TR>
__device__ __forceinline__ void combine_body(
    int nsub, int nchan, const uint8_t *__restrict__ valid, const int32_t *__restrict__ info,
    const float *__restrict__ w0,
    const double *__restrict__ std_d, const double *__restrict__ mean_d, const double *__restrict__ ptp_d, int ptp_f32,
    const double *__restrict__ fft_d, const double *__restrict__ col_med, const double *__restrict__ col_mad,
    const double *__restrict__ row_med, const double *__restrict__ row_mad, double cth, double sth,
    double *__restrict__ test, float *__restrict__ W, float *__restrict__ hist, int iter,
    int32_t *__restrict__ counters, const unsigned bdim, const unsigned gdim, const TR tr)
{
    // grid-stride; the convergence counters are reduced per block (one atomic
    // per counter per block: same-address atomics serialise at the memory side)
    __shared__ int red[4][4];
    __shared__ unsigned long long dred[4];
    const size_t P = (size_t)nsub * nchan;
    int changed = 0, zero = 0, bad = 0, near = 0;
    unsigned long long diff = 0ull;   // bit h: W != hist[h] somewhere (h < 64)
    const int hmax = iter < 64 ? iter : 64;
    for (size_t k = (size_t)blockIdx.x * bdim + threadIdx.x; k < P; k += (size_t)gdim * bdim) {
        const int s = (int)(k / nchan), c = (int)(k % nchan);
        const bool v = valid[k] != 0;
        double S[4];
        if constexpr (TR::on) {
            // dc / ds: the entry's d' in its channel line (entry s of nsub) and
            // in its subint line (entry c of nchan)
            const double dv[4] = {std_d[k], mean_d[k], ptp_d[k], fft_d[k]};
            double dc[4], ds[4];
            // the entry's place in its subint line, and the line's length
            int cg = c, ng = nchan;
            if constexpr (TR::shard) {
                cg = tr.chan0 + c;
                ng = tr.nchan_g;
            }
            if constexpr (TR::pieces) {
                // the same, on the abscissa and with the coefficients of the
                // entry's piece of either line
                const PieceAt ac = piece_at(s, tr.pa.col_piece, tr.pa.col_starts);
                const PieceAt as = piece_at(cg, tr.pa.row_piece, tr.pa.row_starts);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const bool f32 = q == 2 && ptp_f32;
                    const bool in = q == 3 || v;
                    const TrendCoef *cc = tr.col_coef + ((size_t)q * nchan + c) * tr.pa.col_np + ac.p;
                    const TrendCoef *rc = tr.row_coef + ((size_t)q * nsub + s) * tr.pa.row_np + as.p;
                    dc[q] = in ? detrend_value(dv[q], f32, ac.i, ac.L, *cc, tr.chan_order) : dv[q];
                    ds[q] = in ? detrend_value(dv[q], f32, as.i, as.L, *rc, tr.subint_order) : dv[q];
                }
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const bool f32 = q == 2 && ptp_f32;
                    const bool in = q == 3 || v;
                    dc[q] = in ? detrend_value(dv[q], f32, s, nsub, tr.col_coef[(size_t)q * nchan + c], tr.chan_order)
                               : dv[q];
                    ds[q] = in ? detrend_value(dv[q], f32, cg, ng, tr.row_coef[(size_t)q * nsub + s], tr.subint_order)
                               : dv[q];
                }
            }
            S[0] = nanmax2(scale_masked_d(dc[0], v, col_med[c], col_mad[c], cth),
                           scale_masked_d(ds[0], v, row_med[s], row_mad[s], sth));
            S[1] = nanmax2(scale_masked_d(dc[1], v, col_med[nchan + c], col_mad[nchan + c], cth),
                           scale_masked_d(ds[1], v, row_med[nsub + s], row_mad[nsub + s], sth));
            S[2] = ptp_f32 ? nanmax2(scale_masked_f((float)dc[2], v, (float)col_med[2 * nchan + c],
                                                    (float)col_mad[2 * nchan + c], cth),
                                     scale_masked_f((float)ds[2], v, (float)row_med[2 * nsub + s],
                                                    (float)row_mad[2 * nsub + s], sth))
                           : nanmax2(scale_masked_d(dc[2], v, col_med[2 * nchan + c], col_mad[2 * nchan + c], cth),
                                     scale_masked_d(ds[2], v, row_med[2 * nsub + s], row_mad[2 * nsub + s], sth));
            S[3] = nanmax2(scale_plain(dc[3], col_med[3 * nchan + c], col_mad[3 * nchan + c], cth),
                           scale_plain(ds[3], row_med[3 * nsub + s], row_mad[3 * nsub + s], sth));
        } else {
            S[0] = nanmax2(scale_masked_d(std_d[k], v, col_med[c], col_mad[c], cth),
                           scale_masked_d(std_d[k], v, row_med[s], row_mad[s], sth));
            S[1] = nanmax2(scale_masked_d(mean_d[k], v, col_med[nchan + c], col_mad[nchan + c], cth),
                           scale_masked_d(mean_d[k], v, row_med[nsub + s], row_mad[nsub + s], sth));
            // ptp: numpy.ma in f32 for f32 data (Appendix A.5), f64 for f64 data
            S[2] = ptp_f32 ? nanmax2(scale_masked_f((float)ptp_d[k], v, (float)col_med[2 * nchan + c],
                                                    (float)col_mad[2 * nchan + c], cth),
                                     scale_masked_f((float)ptp_d[k], v, (float)row_med[2 * nsub + s],
                                                    (float)row_mad[2 * nsub + s], sth))
                           : nanmax2(scale_masked_d(ptp_d[k], v, col_med[2 * nchan + c], col_mad[2 * nchan + c], cth),
                                     scale_masked_d(ptp_d[k], v, row_med[2 * nsub + s], row_mad[2 * nsub + s], sth));
            S[3] = nanmax2(scale_plain(fft_d[k], col_med[3 * nchan + c], col_mad[3 * nchan + c], cth),
                           scale_plain(fft_d[k], row_med[3 * nsub + s], row_mad[3 * nsub + s], sth));
        }
        double t;
        if (isnan(S[0]) || isnan(S[1]) || isnan(S[2]) || isnan(S[3])) {
            t = NAN;
        } else {
            // sort 4
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3 - a; ++b)
                    if (S[b] > S[b + 1]) {
                        const double tmp = S[b];
                        S[b] = S[b + 1];
                        S[b + 1] = tmp;
                    }
            t = ((0.0 + S[1]) + S[2]) / 2.0;
        }
        test[k] = t;
        near += fabs(t - 1.0) <= kNearTie;   // false for NaN
        const float wn = (t >= 1.0) ? 0.0f : w0[k];
        W[k] = wn;
        hist[(size_t)iter * P + k] = wn;
        changed += !(wn == hist[(size_t)(iter - 1) * P + k]);
        zero += (wn == 0.0f);
        if (info) {   // "Bad status for least squares fit" (iterative_cleaner.py:284-285)
            const int st = info[k];
            bad += (st < 1 || st > 4);
        }
        // history equality (iterative_cleaner.py:135-136)
        for (int h = 0; h < hmax; ++h)
            if (!(wn == hist[(size_t)h * P + k])) diff |= 1ull << h;
        for (int h = 64; h < iter; ++h)
            if (!(wn == hist[(size_t)h * P + k])) atomicOr(&counters[4 + h], 1);
    }
    for (int off = 32; off > 0; off >>= 1) {
        changed += __shfl_xor(changed, off);
        zero += __shfl_xor(zero, off);
        bad += __shfl_xor(bad, off);
        near += __shfl_xor(near, off);
        diff |= __shfl_xor(diff, off);
    }
    const int wave = threadIdx.x >> 6, nw = bdim >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[0][wave] = changed;
        red[1][wave] = zero;
        red[2][wave] = bad;
        red[3][wave] = near;
        dred[wave] = diff;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int ch = 0, ze = 0, bd = 0, nt = 0;
        unsigned long long df = 0ull;
        for (int w = 0; w < nw; ++w) {
            ch += red[0][w];
            ze += red[1][w];
            bd += red[2][w];
            nt += red[3][w];
            df |= dred[w];
        }
        // counters[0..1] (changed, zero) as one u64 add: both < 2^32, no carry
        if (ch || ze)
            atomicAdd((unsigned long long *)counters, ((unsigned long long)(unsigned)ze << 32) | (unsigned)ch);
        if (bd) atomicAdd(&counters[2], bd);
        if (nt) atomicAdd(&counters[3], nt);
        for (int h = 0; h < hmax; ++h)
            if ((df >> h) & 1ull) atomicOr(&counters[4 + h], 1);
    }
}

__global__ __launch_bounds__(256) void k_combine(
    int nsub, int nchan, const uint8_t *__restrict__ valid, const int32_t *__restrict__ info,
    const float *__restrict__ w0,
    const double *__restrict__ std_d, const double *__restrict__ mean_d, const double *__restrict__ ptp_d, int ptp_f32,
    const double *__restrict__ fft_d, const double *__restrict__ col_med, const double *__restrict__ col_mad,
    const double *__restrict__ row_med, const double *__restrict__ row_mad, double cth, double sth,
    double *__restrict__ test, float *__restrict__ W, float *__restrict__ hist, int iter,
    int32_t *__restrict__ counters)
{
    combine_body(nsub, nchan, valid, info, w0, std_d, mean_d, ptp_d, ptp_f32, fft_d, col_med, col_mad, row_med, row_mad,
                 cth, sth, test, W, hist, iter, counters, blockDim.x, gridDim.x, NoTrend{});
}

__global__ __launch_bounds__(256) void k_combine_dt(
    int nsub, int nchan, const uint8_t *__restrict__ valid, const int32_t *__restrict__ info,
    const float *__restrict__ w0,
    const double *__restrict__ std_d, const double *__restrict__ mean_d, const double *__restrict__ ptp_d, int ptp_f32,
    const double *__restrict__ fft_d, const double *__restrict__ col_med, const double *__restrict__ col_mad,
    const double *__restrict__ row_med, const double *__restrict__ row_mad, double cth, double sth,
    double *__restrict__ test, float *__restrict__ W, float *__restrict__ hist, int iter,
    int32_t *__restrict__ counters, TrendArgs t)
{
    combine_body(nsub, nchan, valid, info, w0, std_d, mean_d, ptp_d, ptp_f32, fft_d, col_med, col_mad, row_med, row_mad,
                 cth, sth, test, W, hist, iter, counters, blockDim.x, gridDim.x,
                 TrendView{(const TrendCoef *)t.col_coef, (const TrendCoef *)t.row_coef, t.chan_order, t.subint_order});
}

__global__ __launch_bounds__(256) void k_combine_pw(
    int nsub, int nchan, const uint8_t *__restrict__ valid, const int32_t *__restrict__ info,
    const float *__restrict__ w0,
    const double *__restrict__ std_d, const double *__restrict__ mean_d, const double *__restrict__ ptp_d, int ptp_f32,
    const double *__restrict__ fft_d, const double *__restrict__ col_med, const double *__restrict__ col_mad,
    const double *__restrict__ row_med, const double *__restrict__ row_mad, double cth, double sth,
    double *__restrict__ test, float *__restrict__ W, float *__restrict__ hist, int iter,
    int32_t *__restrict__ counters, TrendArgs t, PieceArgs pa)
{
    combine_body(nsub, nchan, valid, info, w0, std_d, mean_d, ptp_d, ptp_f32, fft_d, col_med, col_mad, row_med, row_mad,
                 cth, sth, test, W, hist, iter, counters, blockDim.x, gridDim.x,
                 PieceView{(const TrendCoef *)t.col_coef, (const TrendCoef *)t.row_coef, t.chan_order, t.subint_order,
                           pa});
}

// the two on a channel shard: the subint direction at chan0 + c of nchan_g
__global__ __launch_bounds__(256) void k_combine_dt_sh(
    int nsub, int nchan, const uint8_t *__restrict__ valid, const int32_t *__restrict__ info,
    const float *__restrict__ w0,
    const double *__restrict__ std_d, const double *__restrict__ mean_d, const double *__restrict__ ptp_d, int ptp_f32,
    const double *__restrict__ fft_d, const double *__restrict__ col_med, const double *__restrict__ col_mad,
    const double *__restrict__ row_med, const double *__restrict__ row_mad, double cth, double sth,
    double *__restrict__ test, float *__restrict__ W, float *__restrict__ hist, int iter,
    int32_t *__restrict__ counters, TrendArgs t, int chan0, int nchan_g)
{
    combine_body(nsub, nchan, valid, info, w0, std_d, mean_d, ptp_d, ptp_f32, fft_d, col_med, col_mad, row_med, row_mad,
                 cth, sth, test, W, hist, iter, counters, blockDim.x, gridDim.x,
                 ShardTrendView{(const TrendCoef *)t.col_coef, (const TrendCoef *)t.row_coef, t.chan_order,
                                t.subint_order, chan0, nchan_g});
}

__global__ __launch_bounds__(256) void k_combine_pw_sh(
    int nsub, int nchan, const uint8_t *__restrict__ valid, const int32_t *__restrict__ info,
    const float *__restrict__ w0,
    const double *__restrict__ std_d, const double *__restrict__ mean_d, const double *__restrict__ ptp_d, int ptp_f32,
    const double *__restrict__ fft_d, const double *__restrict__ col_med, const double *__restrict__ col_mad,
    const double *__restrict__ row_med, const double *__restrict__ row_mad, double cth, double sth,
    double *__restrict__ test, float *__restrict__ W, float *__restrict__ hist, int iter,
    int32_t *__restrict__ counters, TrendArgs t, PieceArgs pa, int chan0, int nchan_g)
{
    combine_body(nsub, nchan, valid, info, w0, std_d, mean_d, ptp_d, ptp_f32, fft_d, col_med, col_mad, row_med, row_mad,
                 cth, sth, test, W, hist, iter, counters, blockDim.x, gridDim.x,
                 ShardPieceView{(const TrendCoef *)t.col_coef, (const TrendCoef *)t.row_coef, t.chan_order,
                                t.subint_order, pa, chan0, nchan_g});
}

// ============================================================ launchers

// one direction's plain lines; wave-private LDS: 256-bin histogram + the line's keys
static hipError_t launch_linestats_dir(hipStream_t st, const LineStatsArgs &a, int rows, int len, int lines)
{
    // few long lines (the rows): W waves per line (a.grp_waves = W in {0, 4, 8},
    // 0 = one wave per line; a.grp_minlen = the shortest line it takes)
    if (lines < 8192 && len >= a.grp_minlen) {
        const int W = a.grp_waves;
        if (W == 4 || W == 8) {
            const int seg = (((len + W - 1) / W) + 63) & ~63;
            const size_t gshm = 1024 + 16 * (size_t)W + (size_t)W * seg * 8;
            if (gshm <= kLdsBlockMax) {
                if (W == 4)
                    IC_GGL(k_linestats_grp<4>, dim3(lines), dim3(256), gshm, st, a, rows, len);
                else
                    IC_GGL(k_linestats_grp<8>, dim3(lines), dim3(512), gshm, st, a, rows, len);
                return hipGetLastError();
            }
        }
    }
    const int per_wave = 1024 + ((len * 8 + 15) / 16) * 16;
    int wpb = 4;
    while (wpb > 1 && (size_t)wpb * per_wave > 64 * 1024) --wpb;
    const size_t shm = (size_t)wpb * per_wave;
    if (shm > kLdsBlockMax) return hipErrorInvalidValue;
    IC_GGL(k_linestats, dim3(cdiv(lines, wpb)), dim3(64 * wpb), shm, st, a, rows, len, wpb, per_wave);
    return hipGetLastError();
}

// one direction's detrended lines with W waves per line, if LDS holds them
// (*done).  With pieces LDS also holds a line's piece coefficients (32 B each)
// and retired flags
template <int W>
static hipError_t launch_linetrend_w(hipStream_t st, const LineStatsArgs &a, const TrendArgs &t, const PieceArgs *pa,
                                     int rows, int len, int lines, bool *done)
{
    const int seg = (((len + W - 1) / W) + 63) & ~63;
    size_t shm = 1024 + 16 * (size_t)W + (size_t)W * seg * 8 + (size_t)((len + 63) / 64) * 8;
    if (pa) {
        const size_t m = (size_t)(rows ? pa->row_np : pa->col_np);
        shm += m * 32 + ((m + 15) & ~(size_t)15);
    }
    *done = shm <= kLdsBlockMax;
    if (!*done) return hipSuccess;
    if (pa)
        IC_GGL(k_linetrend_pw<W>, dim3(lines), dim3(64 * W), shm, st, a, t, *pa, rows, len);
    else
        IC_GGL(k_linetrend<W>, dim3(lines), dim3(64 * W), shm, st, a, t, rows, len);
    return hipGetLastError();
}

// columns (length nsub), then rows (length nchan).  The detrended forms' rows of
// >= grp_minlen values take grp_waves waves per line, as the plain ones do; the
// bits do not depend on it.
hipError_t launch_lines(hipStream_t st, const LineStatsArgs &a, const TrendArgs *trend, const PieceArgs *pa, int which)
{
    if (pa && (!trend || pa->col_np < 1 || pa->col_np > kMaxPieces || pa->row_np < 1 || pa->row_np > kMaxPieces))
        return hipErrorInvalidValue;
    for (int rows = 0; rows < 2; ++rows) {
        if (!((which >> rows) & 1)) continue;
        const int len = rows ? a.nchan : a.nsub;
        const int lines = 4 * (rows ? a.nsub : a.nchan);
        if (lines == 0 || len == 0) continue;
        hipError_t e = hipSuccess;
        if (!trend) {
            e = launch_linestats_dir(st, a, rows, len, lines);
        } else {
            bool done = false;
            if (lines < 8192 && len >= a.grp_minlen) {
                if (a.grp_waves == 4) e = launch_linetrend_w<4>(st, a, *trend, pa, rows, len, lines, &done);
                if (a.grp_waves == 8) e = launch_linetrend_w<8>(st, a, *trend, pa, rows, len, lines, &done);
            }
            if (!done) {
                e = launch_linetrend_w<1>(st, a, *trend, pa, rows, len, lines, &done);
                if (!done) return hipErrorInvalidValue;
            }
        }
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_combine(hipStream_t st, const CombineArgs &c)
{
    const LineStatsArgs &a = c.ls;
    const bool shard = c.trend && c.nchan_g != 0;
    if (c.pieces && !c.trend) return hipErrorInvalidValue;
    if (shard && (c.chan0 < 0 || a.nchan < 0 || c.chan0 + a.nchan > c.nchan_g)) return hipErrorInvalidValue;
    const size_t P = (size_t)a.nsub * a.nchan;
    const unsigned grid = cap_grid(std::min<size_t>(cdiv(P, 256), 1024), c.grid_cap);
    // the arguments every form takes, then the form's own
    auto go = [&](auto kernel, auto... form) {
        IC_GGL(kernel, dim3(grid), dim3(256), 0, st, a.nsub, a.nchan, a.valid, c.info, c.w0, a.std_d, a.mean_d, a.ptp_d,
               a.ptp_f32, a.fft_d, a.col_med, a.col_mad, a.row_med, a.row_mad, c.chanthresh, c.subintthresh, c.test,
               c.W, c.hist, c.iter, c.counters, form...);
        return hipGetLastError();
    };
    if (!c.trend) return go(k_combine);
    if (shard) {
        if (c.pieces) return go(k_combine_pw_sh, *c.trend, *c.pieces, c.chan0, c.nchan_g);
        return go(k_combine_dt_sh, *c.trend, c.chan0, c.nchan_g);
    }
    if (c.pieces) return go(k_combine_pw, *c.trend, *c.pieces);
    return go(k_combine_dt, *c.trend);
}

}  // namespace icgpu
