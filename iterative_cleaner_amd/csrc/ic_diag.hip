// ic_diag.hip -- the diagnostics of the surgical-cleaning loop, with their
// launchers.  The FFT pieces, the P2 / CLay layouts and the rules shared with
// the rotation are in ic_fftdiag.h.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see Makefile).
// -ffp-contract=off is load-bearing: every f64/f32 operation below must be an
// individually rounded IEEE op in the order written, so that results equal
// numpy / scipy (MINPACK) bit-for-bit.  Explicit fma() is never used on an
// exact path.
//
// Kernels:
//   k_diag           residual (ic.py:279-288), f32 store (:272), dededisperse
//                    (:104), apply_weights (:296), diagnostics (:206-217); any
//                    nbin, a wave per profile (what no kernel below serves)
//   k_diag_p2        the same for the power-of-two nbin (IC_P2_SIZES)
//   k_diag_cl        the chain layout at nbin 1024 / 2048 / 4096
//   k_diag_mr        the same for the mixed-radix nbin (mr_supported)
//   k_diag_czt       the same for the other nbin in 129..4096 (diag_czt_supported):
//                    fftmax by a chirp-z transform
//   k_residual       the residual cube on request (ic_get_residual)
//   k_tnorm          sum(T*T), fit_mode 1's denominator
#include <algorithm>
#include <math.h>

#include <type_traits>

#include "ic_fftdiag.h"

namespace icgpu {

// ============================================================ diagnostics

// numpy pairwise sum of n values produced by get(i), in dtype Tp (one wave).
// scratch: >= 8*nleaf + nleaf + nops slots of Tp in LDS.
template <typename Tp, typename Get>
__device__ Tp wave_pairwise(const PwPlan &pl, Get get, Tp *scratch, int lane)
{
    const int nl = pl.nleaf;
    Tp *acc = scratch;             // [nl*8]
    Tp *slot = scratch + nl * 8;   // [nl + nops]
    for (int task = lane; task < nl * 8; task += 64) {
        const int Lf = task >> 3, j = task & 7;
        const int st = pl.leaf_start[Lf], len = pl.leaf_len[Lf];
        if (len < 8) {
            if (j == 0) {
                Tp res = (Tp)0;
                for (int q = 0; q < len; ++q) res = res + get(st + q);
                acc[task] = res;
            }
            continue;
        }
        const int main = len - len % 8;
        Tp r = get(st + j);
        for (int q = 8; q < main; q += 8) r = r + get(st + q + j);
        acc[task] = r;
    }
    wave_sync();
    for (int Lf = lane; Lf < nl; Lf += 64) {
        const int st = pl.leaf_start[Lf], len = pl.leaf_len[Lf];
        const Tp *r = acc + Lf * 8;
        Tp res;
        if (len < 8) {
            res = r[0];
        } else {
            const Tp a01 = r[0] + r[1], a23 = r[2] + r[3], a45 = r[4] + r[5], a67 = r[6] + r[7];
            const Tp lo = a01 + a23, hi = a45 + a67;
            res = lo + hi;
            for (int q = len - len % 8; q < len; ++q) res = res + get(st + q);
        }
        slot[Lf] = res;
    }
    wave_sync();
    Tp out = (Tp)0;
    if (lane == 0) {
        for (int o = 0; o < pl.nops; ++o) slot[nl + o] = slot[pl.op_a[o]] + slot[pl.op_b[o]];
        out = (Tp)0 + slot[pl.root];
        acc[0] = out;
    }
    wave_sync();
    out = acc[0];
    wave_sync();
    return out;
}

// Persistent blocks of `wpb` independent waves; each wave cleans profiles
// k = blockIdx.x*wpb + wave, += gridDim.x*wpb.  LDS: plan + twiddles (block-shared,
// loaded once) | per wave: complex work [n/2] (pow2) | X f32 [n] | pairwise scratch.
// Per profile: the f32 residual (iterative_cleaner.py:279-288, :272), dededispersion
// (:104), the ORIGINAL weight (:296) and the four diagnostics (:206-217) with
// numpy.ma data conventions.
// exp(-2 pi i q/n) for 0 <= q < n from the half table tw[0..n/2)
__device__ __forceinline__ double2 twid(const double2 *tw, int q, int half)
{
    if (q < half) return tw[q];
    const double2 t = tw[q - half];
    return make_double2(-t.x, -t.y);
}

// One radix-R Stockham stage over m points (src -> dst), Ns = product of earlier radices.
// get(q) supplies src point q (lets the first stage read the real input directly).
template <int R, typename Get>
__device__ __forceinline__ void stockham_stage(Get get, double2 *dst, int m, int Ns, const double2 *tw, int n,
                                               int lane)
{
    const int nb = m / R;
    const int tmul = n / (R * Ns);
    for (int b = lane; b < nb; b += 64) {
        const int k = b & (Ns - 1);
        double2 v[R];
#pragma unroll
        for (int r = 0; r < R; ++r) v[r] = get(b + r * nb);
        if (Ns > 1) {
#pragma unroll
            for (int r = 1; r < R; ++r) v[r] = cmul(v[r], twid(tw, r * k * tmul, n / 2));
        }
        dft_small<R>(v);
        const int idx = (b - k) * R + k;
#pragma unroll
        for (int r = 0; r < R; ++r) dst[idx + r * Ns] = v[r];
    }
}

struct DiagLayout {
    int ntw;          // twiddles in LDS
    size_t cw_off, x_off, p_off, scr_off, per_wave;
};

__host__ __device__ inline DiagLayout diag_layout(int n, int nleaf, int nops)
{
    DiagLayout L;
    const bool pow2 = (n & (n - 1)) == 0 && n >= 4;
    L.ntw = pow2 ? n / 2 : n;
    L.cw_off = 0;                                            // buffer A: n/2 complex
    const size_t cwb = (size_t)(pow2 ? n / 2 : 1) * 16;
    L.x_off = cwb;                                           // buffer B (n/2 complex) aliases X (n f64)
    const size_t xb = ((size_t)n * 8 + 15) & ~(size_t)15;
    const size_t pb = ((size_t)n * 4 + 15) & ~(size_t)15;
    L.p_off = L.x_off + (pow2 ? (cwb > xb ? cwb : xb) : xb);  // DIAG_CLOSED: the fit-cube row
    L.scr_off = L.p_off + pb;
    L.per_wave = L.scr_off + (size_t)(nleaf * 9 + nops + 8) * 8;
    L.per_wave = (L.per_wave + 15) & ~(size_t)15;
    return L;
}

__global__ __launch_bounds__(256) void k_diag(DiagArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ PwPlan pl;
    const int n = a.nbin;
    const int wpb = blockDim.x >> 6;
    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    {
        const int32_t *src = (const int32_t *)a.plan;
        int32_t *dst = (int32_t *)&pl;
        for (int q = threadIdx.x; q < (int)(sizeof(PwPlan) / 4); q += blockDim.x) dst[q] = src[q];
    }
    const DiagLayout lay = diag_layout(n, a.plan->nleaf, a.plan->nops);
    double2 *tw = (double2 *)smem;
    for (int q = threadIdx.x; q < lay.ntw; q += blockDim.x) tw[q] = a.tw[q];
    __syncthreads();
    unsigned char *wb = smem + (size_t)lay.ntw * 16 + (size_t)wave * lay.per_wave;
    double2 *cw = (double2 *)(wb + lay.cw_off);
    double *X = (double *)(wb + lay.x_off);   // f32 values unless data_f64
    float *Pr = (float *)(wb + lay.p_off);
    double *scr = (double *)(wb + lay.scr_off);
    const bool pow2 = (n & (n - 1)) == 0 && n >= 4;
    const size_t P = (size_t)a.nsub * a.nchan;
    const double *T64 = a.T64;
    const int mode = a.mode;

    for (size_t k = (size_t)blockIdx.x * wpb + wave; k < P; k += (size_t)gridDim.x * wpb) {
        const int c = (int)((unsigned)k % (unsigned)a.nchan);
        const float w = a.w0[k];
        const bool valid = (w != 0.0f);
        const int sh = mode == DIAG_STATS ? 0 : a.shift[c];
        wave_sync();   // previous profile's LDS reads are done
        double x = 0.0;
        int stt = 0;
        const float *p;
        if (mode == DIAG_CLOSED) {
            // the fit-cube row f32(ded - base0), dedispersed order, then the
            // closed-form amplitude from numpy pairwise sums
            const float *row = a.raw + k * (size_t)n;
            const float b = a.base[k];
            for (int j = lane; j < n; j += 64) {
                int i = j - sh;
                if (i < 0) i += n;
                Pr[i] = row[j] - b;
            }
            wave_sync();
            // the products in the stored (dispersed) order j: bin i = (j - sh) mod n
            const double dot = wave_pairwise<double>(pl, [&](int q) {
                int i = q - sh;
                if (i < 0) i += n;
                return T64[i] * (double)Pr[i];
            }, scr, lane);
            const double TT = *a.TT;
            x = TT != 0.0 ? dot / TT : 0.0;
            stt = isfinite(x) ? 1 : 5;
            if (lane == 0) {
                a.amp[k] = x;
                a.info[k] = stt;
            }
            p = Pr;
        } else {
            if (mode == DIAG_EXACT) {
                x = a.amp[k];
                stt = a.info[k];
            }
            p = a.D + k * (size_t)a.ldD;
        }
        const bool tr = a.dtiled && mode == DIAG_EXACT;   // the tiled fit cube (dt_ofs)
        auto prow = [&](int i) -> float { return tr ? a.D[dt_ofs(k, i, a.ldD)] : p[i]; };
        const bool ok = fit_ok(stt);
        // residual -> X (dispersed frame): X[j] = f32(f32(r[i]) * w), j = (i + sh) mod n
        // (f64(f32(r[i])) * f64(w) for f64 data)
        for (int i = lane; i < n; i += 64) {
            float R = 0.0f;
            if (mode == DIAG_STATS) {
                R = p[i];
            } else if (ok) {
                R = residual_sample(x, T64[i], prow(i), i, a);
            }
            int j = i + sh;
            if (j >= n) j -= n;
            X[j] = a.data_f64 ? (double)R * (double)w : (double)(R * w);
        }
        wave_sync();
        double mean = 0.0, sd = 0.0, ptp = ptp_fill(a.data_f64);
        if (valid) {
            if (a.data_f64)
                mean = wave_pairwise<double>(pl, [&](int q) { return X[q]; }, scr, lane) / (double)n;
            else
                mean = (double)wave_pairwise<float>(pl, [&](int q) { return (float)X[q]; }, (float *)scr, lane) /
                       (double)n;
            const double mu = mean;
            const double ss = wave_pairwise<double>(
                pl,
                [&](int q) {
                    const double d = (double)X[q] - mu;
                    return d * d;
                },
                scr, lane);
            sd = sqrt(ss / (double)n);
            double mx = -INFINITY, mn = INFINITY;
            int nan = 0;
            for (int q = lane; q < n; q += 64) {
                const double v = X[q];
                if (isnan(v)) nan = 1;
                mx = fmax(mx, v);
                mn = fmin(mn, v);
            }
            mx = wave_tree<64>(mx, OpMaxF());
            mn = wave_tree<64>(mn, OpMinF());
            nan = wave_tree<64>(nan, OpOr());
            // max - min in the data dtype (exact widening of f32 values)
            ptp = nan ? (double)NAN : (a.data_f64 ? mx - mn : (double)((float)mx - (float)mn));
        }
        // fftmax: max_k |rfft(v)_k|, v = f64(X) - mean (valid) or f64(X) (invalid)
        const double mu = valid ? mean : 0.0;
        double best = 0.0;
        int nanf = 0;
        if (pow2) {
            const int m = n / 2;
            double2 *bufA = cw;
            double2 *bufB = (double2 *)X;    // X is dead once the first stage has read it
            int lg = 0;
            while ((1 << lg) < m) ++lg;
            // stage radices: as many 8s as possible, then one 4 or 2
            int Ns = 1, done = 0;
            double2 *src = nullptr, *dst = bufA;
            auto first = [&](int q) {
                return valid ? make_double2((double)X[2 * q] - mu, (double)X[2 * q + 1] - mu)
                             : make_double2((double)X[2 * q], (double)X[2 * q + 1]);
            };
            auto from = [&](int q) { return src[q]; };
            while (done < lg) {
                const int rem = lg - done;
                const int rl = rem >= 3 ? 3 : rem;
                if (Ns == 1) {
                    if (rl == 3) stockham_stage<8>(first, dst, m, Ns, tw, n, lane);
                    else if (rl == 2) stockham_stage<4>(first, dst, m, Ns, tw, n, lane);
                    else stockham_stage<2>(first, dst, m, Ns, tw, n, lane);
                } else {
                    if (rl == 3) stockham_stage<8>(from, dst, m, Ns, tw, n, lane);
                    else if (rl == 2) stockham_stage<4>(from, dst, m, Ns, tw, n, lane);
                    else stockham_stage<2>(from, dst, m, Ns, tw, n, lane);
                }
                wave_sync();
                Ns <<= rl;
                done += rl;
                src = dst;
                dst = (dst == bufA) ? bufB : bufA;
            }
            const double2 *Z = (lg == 0) ? nullptr : src;
            // X_k = (Z_k + conj(Z_{m-k}))/2 - i/2 W^k (Z_k - conj(Z_{m-k})), W = exp(-2 pi i/n)
            for (int kk = lane; kk <= m; kk += 64) {
                const double2 zk = Z[kk == m ? 0 : kk];
                const double2 zm = Z[kk == 0 ? 0 : m - kk];
                const double er = 0.5 * (zk.x + zm.x), ei = 0.5 * (zk.y - zm.y);
                const double orr = 0.5 * (zk.y + zm.y), oi = -0.5 * (zk.x - zm.x);
                double wr = -1.0, wi = 0.0;
                if (kk < m) {
                    const double2 wv = tw[kk];
                    wr = wv.x;
                    wi = wv.y;
                }
                const double re = er + (orr * wr - oi * wi);
                const double im = ei + (orr * wi + oi * wr);
                const double mag = hypot(re, im);
                if (isnan(mag)) nanf = 1;
                best = fmax(best, mag);
            }
        } else {
            for (int kk = lane; kk <= n / 2; kk += 64) {
                double sr = 0.0, si = 0.0;
                int q = 0;
                for (int j = 0; j < n; ++j) {
                    const double v = valid ? (double)X[j] - mu : (double)X[j];
                    const double2 wv = tw[q];
                    sr += v * wv.x;
                    si += v * wv.y;
                    q += kk;
                    if (q >= n) q -= n;
                }
                const double mag = hypot(sr, si);
                if (isnan(mag)) nanf = 1;
                best = fmax(best, mag);
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            best = fmax(best, __shfl_xor(best, off));
            nanf |= __shfl_xor(nanf, off);
        }
        if (lane == 0) {   // diag_store, restated: the call moved the epilogue's code
            a.std_o[k] = valid && isfinite(mean) ? sd : 0.0;   // numpy.ma: a non-finite mean is masked -> std 0
            a.mean_o[k] = valid ? mean : 0.0;
            a.ptp_o[k] = ptp;
            a.fft_o[k] = nanf ? NAN : best;
        }
    }
}

// ---------------------------------------------------------------------------
// k_diag_p2<N>: the same diagnostics for power-of-two nbin = N (IC_P2_SIZES:
// 64..8192).  A profile group of TPP = 64*WPP threads cleans one profile: one
// wave for N <= 1024, N/1024 waves for N = 2048/4096/8192, so every thread holds
// the same 16 samples and one pairwise chain at every N >= 1024 (at N = 4096 one
// wave per profile needed a 32-KiB work array per wave: 1.25 waves/SIMD).  At
// N = 8192 the group is 8 waves (512 threads) around a 64-KiB work array (68 KiB
// for f64 data): two groups per CU, 4 waves per SIMD, and four radix-8 stages.
// numpy's pairwise sum for N = 2^k is a balanced tree over leaves of
// min(N,128) samples, each leaf 8 strided chains of min(N,128)/8 samples:
// chain c = (leaf c/8, accumulator c%8) lives in thread c%TPP, slot c/TPP, and
// the tree is reproduced exactly by xor-shuffles within a wave (IEEE add is
// commutative), a balanced add of the group's waves and a balanced in-register
// add of the slots.  X sits in LDS at idx + 8*(idx>>7) so the chain reads are
// bank-conflict free.  The rFFT is an in-place mixed-radix Stockham FFT of
// N/2 complex points (all of a stage's inputs are in registers before it
// writes).
// Modes (DiagArgs.mode):
//   DIAG_EXACT   residual from the exact fit's amplitude / status (ic.py:279-288)
//   DIAG_CLOSED  fit_mode 1: closed-form amplitude a = sum(T*p) / sum(T*T)
//                (numpy pairwise f64 sums over the dedispersed profile, the
//                fit cube row p = f32(ded - base0) formed from the raw cube),
//                then the same residual; writes amp / info
//   DIAG_STATS   comprehensive_stats alone (ic.py:181-226): X = f32(row * w)
// occupancy floors (waves per SIMD, <= 128 VGPRs): 4 for the multi-wave groups
// (the LDS allows 4 blocks of 4096 per CU and 2 of 8192, 16 waves either way)
// and for N = 1024 (the LDS allows 4
// waves/SIMD with 8-wave blocks), where the template is then read from L1
// instead of being held in 32 VGPRs.  Measured on C2 (k_diag ms per clean):
// 3 waves + template in registers 8.63, 4 waves + registers 8.10 (spills),
// 4 waves + L1 template 7.95 (profiles/r02_c2_diag_ab.txt).
template <int N>
constexpr int p2_min_waves() { return N >= 2048 ? 4 : (N == 1024 ? 4 : 1); }

// D64 (data_f64): psrchive's get_data returns f64, so apply_weights and the
// masked statistics run in f64 (iterative_cleaner.py:111-112, :206-209): X =
// f64(R) * f64(w), the mean's pairwise sum and ptp in f64.
template <int N, int MODE, bool D64>
__global__ __launch_bounds__(N >= 2048 ? P2<N>::TPP : 512, p2_min_waves<N>()) void k_diag_p2(DiagArgs a)
{
    using C = P2<N, D64>;
    using XT = typename std::conditional<D64, double, float>::type;
    constexpr int WPP = C::WPP, TPP = C::TPP, NPT = C::NPT;
    // one-wave groups keep the template and the next row in registers; the
    // multi-wave groups (N >= 2048) read both when needed and rely on occupancy
    constexpr bool TREG = WPP == 1 && N != 1024, PREFETCH = WPP == 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // [M] post-processing twiddles, then the stage tables (LDS copy unless TWG)
    const double2 *tw = C::TWG ? a.tw_p2 : (const double2 *)smem;
    const double *T = a.T64;          // L1/L2-resident, read coalesced
    constexpr int mode = MODE;
    const int lane = threadIdx.x & 63;
    // WPP == 1: independent waves (groups) per block; WPP > 1: the block is one group
    const int group = WPP == 1 ? (int)(threadIdx.x >> 6) : 0;
    const int gpb = WPP == 1 ? (int)(blockDim.x >> 6) : 1;
    const int wave = WPP == 1 ? 0 : (int)(threadIdx.x >> 6);   // wave within the group
    int t = WPP == 1 ? lane : (int)threadIdx.x;               // thread within the group
    if (!C::TWG) {
        for (int q = threadIdx.x; q < C::TW; q += blockDim.x) ((double2 *)smem)[q] = a.tw_p2[q];
        __syncthreads();
    }
    unsigned char *gb = smem + (size_t)C::TW_LDS * 16 + (size_t)group * C::GROUP_BYTES;
    XT *X = (XT *)gb;
    double2 *Cb = (double2 *)gb;   // aliases X after the first FFT stage has read it
    double *red = (double *)(gb + C::WORK_BYTES);   // 64 slots of 8 B (WPP > 1)
    const unsigned P = (unsigned)a.nsub * (unsigned)a.nchan;
    const unsigned stride = gridDim.x * gpb;
    const int nchan = a.nchan;
    // the template stays in registers, and each group loads the next profile's
    // row while it works on the current one: every global load of the loop is
    // issued ahead of its use (software pipelining)
    double tv[TREG ? NPT : 1];
    if (TREG) {
#pragma unroll
        for (int u = 0; u < NPT; ++u) tv[u] = T[t + TPP * u];
    }
    constexpr bool closed = mode == DIAG_CLOSED || mode == DIAG_FIT;
    const double TT = closed ? *a.TT : 0.0;
    // DIAG_EXACT reads the raw row, not the fit cube: the cube's value is
    // D_i = f32(raw_j - base0), j = (i + sh) mod N (k_chan_partials mode 3), and
    // the raw rows are contiguous whatever the cube's layout (dt_ofs)
    constexpr bool fromraw = mode == DIAG_CLOSED || mode == DIAG_EXACT;
    const float *rows = fromraw ? a.raw : a.D;
    const size_t ld = fromraw ? (size_t)N : (size_t)a.ldD;
    float pv[NPT];
    auto loadrow = [&](unsigned kk) {
        const float *pn = rows + (size_t)kk * ld;
#pragma unroll
        for (int u = 0; u < NPT; ++u) pv[u] = pn[t + TPP * u];
    };
    // profiles: all P, or the slots of a list, minus those with skip[k] != 0
    // (the two passes of the exact fit's forked diagnostics)
    const RoundList rl(a.list, a.nctr, (long)P);
    const unsigned nslot = (unsigned)rl.n();
    const uint8_t *skip = a.skip;
    auto next_slot = [&](unsigned sl) {   // the first slot >= sl this group measures (uniform)
        if (skip)
            while (sl < nslot && skip[rl.at(sl)]) sl += stride;
        return sl;
    };
    unsigned slot = next_slot(__builtin_amdgcn_readfirstlane(blockIdx.x * gpb + group));
    unsigned k = slot < nslot ? (unsigned)rl.at(slot) : 0u;
    // per-profile scalars, loaded one profile ahead as well
    double nx = 0.0;
    int nst = 0, nsh = 0;
    float nw = 0.0f, nb = 0.0f;
    if (slot < nslot) {
        if (PREFETCH) {
            loadrow(k);
        }
        if (mode == DIAG_EXACT) {
            nx = a.amp[k];
            nst = a.info[k];
        }
        if (fromraw) nb = a.base[k];
        nw = a.w0[k];
        nsh = (mode == DIAG_STATS || mode == DIAG_FIT) ? 0 : a.shift[k % (unsigned)nchan];
    }
    for (unsigned snext = 0; slot < nslot; slot = snext, k = slot < nslot ? (unsigned)rl.at(slot) : 0u) {
        snext = next_slot(slot + stride);
        // opaque to the optimiser: the LDS addresses of the FFT stages derive
        // from t, and hoisting all of them out of the loop costs ~100 VGPRs
        // (spills at N >= 2048); recomputing them is a few VALU ops each
        asm volatile("" : "+v"(t));
        double x = nx;
        int st = nst;
        const float w = nw;
        const bool valid = (w != 0.0f);
        const int sh = nsh;
        const float bk = nb;
        if (!PREFETCH) {
            loadrow(k);
        }
        gsync<WPP>();
        if (closed) {
            // fit cube row p_i = f32(ded_i - base0), i = (j - sh) mod N: to LDS in
            // the dedispersed order, then a = sum(T*p)/sum(T*T) over the chains
            // of the stored order (the products T_i p_i of j = i + sh)
            const XWrap<N, TPP> xw((t - sh) & (N - 1));
#pragma unroll
            for (int u = 0; u < NPT; ++u) X[xw(u)] = (XT)(pv[u] - bk);
            gsync<WPP>();
            double cs[C::CPL];
            const bool act = C::ACT >= TPP || t < C::ACT;   // every thread holds a chain at N >= 512
#pragma unroll
            for (int sl = 0; sl < C::CPL; ++sl) {
                const int ch = t + TPP * sl;
                const int base = (ch >> 3) * C::LEAF + (ch & 7);
                double r = 0.0;
                if (act) {
                    // the chain's stored (dispersed) samples j = base + 8 q pair
                    // with the dedispersed bins i = (j - sh) mod N
                    auto term = [&](int j) {
                        const int i = (j - sh) & (N - 1);
                        return T[i] * (double)X[xaddr(i)];
                    };
                    r = term(base);
#pragma unroll
                    for (int q = 1; q < C::CL; ++q) {
                        const double pr = term(base + 8 * q);
                        r = r + pr;
                    }
                }
                cs[sl] = r;
            }
            const double dot = 0.0 + chain_total<N, double>(cs, red, wave, lane);
            x = TT != 0.0 ? dot / TT : 0.0;
            st = isfinite(x) ? 1 : 5;
#pragma unroll
            for (int u = 0; u < NPT; ++u) pv[u] = (float)X[TPP % 128 == 0 ? xaddr(t) + u * (TPP + TPP / 16) : xaddr(t + TPP * u)];
            if (t == 0) {
                a.amp[k] = x;
                a.info[k] = st;
            }
            gsync<WPP>();
        }
        if constexpr (mode == DIAG_FIT) {   // the amplitude is all this mode produces
            if (PREFETCH && snext < nslot) loadrow((unsigned)rl.at(snext));
            continue;
        }
        const bool ok = fit_ok(st);
        // residual -> X (dispersed frame, padded addresses)
        // X = apply_weights(R, w0): f32(R * w), or f64(R) * f64(w) for f64 data
        auto weigh = [&](float R) -> XT {
            if constexpr (D64) return (double)R * (double)w;
            else return R * w;
        };
        if (mode == DIAG_STATS) {
#pragma unroll
            for (int u = 0; u < NPT; ++u) X[TPP % 128 == 0 ? xaddr(t) + u * (TPP + TPP / 16) : xaddr(t + TPP * u)] = weigh(pv[u]);
        } else if (mode == DIAG_EXACT) {
            // sample j = t + TPP u of the raw row (dispersed frame) is the
            // dedispersed sample i = (j - sh) mod N: residual f32(x T_i - D_i)
            // with D_i = f32(raw_j - base0), written to X[j]
            const int i0 = (t - sh) & (N - 1);
            double tg[NPT];   // the template gathered at i: all loads issued before the first use
            {
                // byte offsets (8 i0 + 8 TPP u) mod 8N through a buffer descriptor: two VALU per load
                const __amdgpu_buffer_rsrc_t tr =
                    __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(T), 0, 8 * N, 0x00020000);
                const unsigned b0 = 8u * (unsigned)i0;
#pragma unroll
                for (int u = 0; u < NPT; ++u)
                    tg[u] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(
                                                           tr, (b0 + 8u * TPP * u) & (8u * N - 1u), 0, 0));
            }
            if (a.pr_on) {
#pragma unroll
                for (int u = 0; u < NPT; ++u) {
                    const int i = (i0 + TPP * u) & (N - 1);
                    const float pj = pv[u] - bk;
                    const float e = residual_sample(x, tg[u], pj, i, PulseRegion{true, a.pr_start, a.pr_end, a.pr_factor});
                    const float R = ok ? e : 0.0f;
                    X[TPP % 128 == 0 ? xaddr(t) + u * (TPP + TPP / 16) : xaddr(t + TPP * u)] = weigh(R);
                }
            } else {
#pragma unroll
                for (int u = 0; u < NPT; ++u) {
                    const float pj = pv[u] - bk;
                    const float e = residual_sample(x, tg[u], pj);
                    const float R = ok ? e : 0.0f;
                    X[TPP % 128 == 0 ? xaddr(t) + u * (TPP + TPP / 16) : xaddr(t + TPP * u)] = weigh(R);
                }
            }
        } else if (a.pr_on) {
            const XWrap<N, TPP> xw((t + sh) & (N - 1));
#pragma unroll
            for (int u = 0; u < NPT; ++u) {
                const int i = t + TPP * u;
                // residual_sample, restated: either call changed some closed forms of this kernel
                const double uu = x * (TREG ? tv[u] : T[i]);
                double e = uu - (double)pv[u];
                if (i >= a.pr_start && i < a.pr_end) e = e * a.pr_factor;
                const float R = ok ? (float)e : 0.0f;
                X[xw(u)] = weigh(R);
            }
        } else {
            const XWrap<N, TPP> xw((t + sh) & (N - 1));
#pragma unroll
            for (int u = 0; u < NPT; ++u) {
                const int i = t + TPP * u;
                const float e = residual_sample(x, TREG ? tv[u] : T[i], pv[u]);
                const float R = ok ? e : 0.0f;
                X[xw(u)] = weigh(R);
            }
        }
        if (snext < nslot) {
            const unsigned kn = (unsigned)rl.at(snext);
            if (PREFETCH) loadrow(kn);
            if (mode == DIAG_EXACT) {
                nx = a.amp[kn];
                nst = a.info[kn];
            }
            if (fromraw) nb = a.base[kn];
            nw = a.w0[kn];
            nsh = mode == DIAG_STATS ? 0 : a.shift[kn % (unsigned)nchan];
        }
        gsync<WPP>();
        double mean = 0.0, sd = 0.0, fftv = 0.0, ptp = ptp_fill(D64);
        if (valid) {
            // chain values -> registers
            XT v[C::CPL][C::CL];
            const bool act = C::ACT >= TPP || t < C::ACT;   // every thread holds a chain at N >= 512
#pragma unroll
            for (int sl = 0; sl < C::CPL; ++sl) {
                const int ch = t + TPP * sl;
                const int base = (ch >> 3) * C::LEAF + (ch & 7);
#pragma unroll
                for (int q = 0; q < C::CL; ++q) v[sl][q] = act ? X[xaddr(base) + 8 * q] : (XT)0;
            }
            // mean: pairwise sum in the data dtype (f32, or f64 for f64 data)
            XT fs[C::CPL];
#pragma unroll
            for (int sl = 0; sl < C::CPL; ++sl) {
                XT r = v[sl][0];
#pragma unroll
                for (int q = 1; q < C::CL; ++q) r = r + v[sl][q];
                fs[sl] = r;
            }
            const XT s32 = (XT)0 + chain_total<N, XT>(fs, (XT *)(red + 16), wave, lane);
            mean = (double)s32 / (double)N;
            // var: f64 pairwise sum of (f64(X) - mean)^2
            double ds[C::CPL];
#pragma unroll
            for (int sl = 0; sl < C::CPL; ++sl) {
                double d0 = (double)v[sl][0] - mean;
                double r = d0 * d0;
#pragma unroll
                for (int q = 1; q < C::CL; ++q) {
                    const double d = (double)v[sl][q] - mean;
                    const double sq = d * d;
                    r = r + sq;
                }
                ds[sl] = r;
            }
            const double ss = 0.0 + chain_total<N, double>(ds, red + 24, wave, lane);
            sd = sqrt(ss / (double)N);
            // ptp (NaN-propagating), in the data dtype
            XT mx = -INFINITY, mn = INFINITY;
            if (act) {
#pragma unroll
                for (int sl = 0; sl < C::CPL; ++sl)
#pragma unroll
                    for (int q = 0; q < C::CL; ++q) {
                        mx = OpMaxF()(mx, v[sl][q]);
                        mn = OpMinF()(mn, v[sl][q]);
                    }
            }
            mx = group_tree<WPP, 64>(mx, OpMaxF(), (XT *)(red + 32), wave, lane);
            mn = group_tree<WPP, 64>(mn, OpMinF(), (XT *)(red + 40), wave, lane);
            // a NaN sample makes the pairwise sum s32 NaN; a NaN s32 without one
            // (inf - inf) is rare, and only then are the samples checked one by one
            int nan = 0;
            if (isnan(s32)) {   // group-uniform
                if (act) {
#pragma unroll
                    for (int sl = 0; sl < C::CPL; ++sl)
#pragma unroll
                        for (int q = 0; q < C::CL; ++q) nan |= isnan(v[sl][q]);
                }
                nan = group_tree<WPP, 64>(nan, OpOr(), (int *)(red + 48), wave, lane);
            }
            ptp = nan ? (double)NAN : (double)(XT)(mx - mn);
            // rFFT of f64(X) - mean: N/2-point complex Stockham, in place
            p2_fft<C::M, TPP, C::LG, 0, 1, C::M, XT>(Cb, X, mean, tw, t);
            // X_k = E_k + w^k O_k, computed as 2 X_k (the 1/2 factors are exact
            // powers of two, applied once to the maximum).  Bins pair up: with
            // E_k, O_k from Z_k and Z_(M-k), E_(M-k) = conj E_k, O_(M-k) = conj O_k
            // and w^(M-k) = -conj w^k, so X_(M-k) = conj(E_k - w^k O_k): one
            // product t = w^k O_k serves X_k = E + t and X_(M-k).  Pairs k = 0 ..
            // M/2 cover every bin: k = 0 gives DC (E + O) and Nyquist (E - O), k = M/2
            // pairs with itself.  NaN: the a2 are >= 0 or NaN, so their sum is NaN
            // iff one of them is.
            constexpr int H = C::M / 2;
            constexpr int JF = H / TPP;   // pair tasks every thread holds
            double best2 = 0.0, nsum = 0.0;
#pragma unroll
            for (int j = 0; j < JF; ++j) {
                // kk = t + TPP j, M - kk = (TPP - t) + (M - TPP (j + 1)): 64-multiples apart
                const int kk = t + TPP * j;
                const double2 zk = Cb[cidx(t) + TPP * j];
                const double2 zm = Cb[kk == 0 ? 0 : cidx(TPP - t) + (C::M - TPP * (j + 1))];
                spec_pair_nan(zk, zm, tw[kk], best2, nsum);
            }
            {
                const int kk = t + TPP * JF;   // the rest: kk <= M/2 (one thread at N >= 256)
                if (kk <= H) spec_pair_nan(Cb[cidx(kk)], Cb[cidx(kk == 0 ? 0 : C::M - kk)], tw[kk], best2, nsum);
            }
            int nanf = isnan(nsum);
            best2 = group_tree<WPP, 64>(best2, OpMaxF(), red + 52, wave, lane);
            nanf = group_tree<WPP, 64>(nanf, OpOr(), (int *)(red + 60), wave, lane);
            fftv = nanf ? NAN : 0.5 * sqrt(best2);
        } else {
            // invalid: rfft of f64(X) = +-0 -> 0, unless R was non-finite (X NaN)
            int nanx = 0;
            for (int i = t; i < N; i += TPP) nanx |= isnan(X[xaddr(i)]);
            nanx = group_tree<WPP, 64>(nanx, OpOr(), (int *)(red + 48), wave, lane);
            fftv = nanx ? NAN : 0.0;
        }
        if (t == 0) {   // diag_store, restated: the call changed three of this kernel's forms
            a.std_o[k] = valid && isfinite(mean) ? sd : 0.0;   // numpy.ma: a non-finite mean is masked -> std 0
            a.mean_o[k] = valid ? mean : 0.0;
            a.ptp_o[k] = ptp;
            a.fft_o[k] = fftv;
        }
    }
}

// ---------------------------------------------------------------------------
// k_diag_cl<N, MODE>: DIAG_EXACT / DIAG_CLOSED diagnostics for N >= 1024 (f32
// data, no pulse region), chain layout.  Same arithmetic and the same bits as
// k_diag_p2 (ic.py:206-217, :272-288, :296); what changes is where the data
// lives:
// - Thread t of a profile group (L = N/16 threads: one wave at N = 1024) owns
//   pairwise chain t = (leaf t/8, accumulator t%8), the dispersed-frame samples
//   j = 128(t/8) + t%8 + 8q, q < 16, and loads them straight from the raw row
//   (one 64-bit address per profile, immediate offsets 32q).
// - The template is gathered at i = (j - sh) mod N from T2 = [T, T] (2N f64),
//   so the wrap costs nothing: one address, immediate offsets 64q.
// - mean / var / ptp run on the residual in registers (no LDS round trip), and
//   the var pass stores d = f64(X) - mean, which IS the FFT's input, as f64
//   into the complex work array in the first stage's gather order, so the FFT
//   starts without conversions or subtractions.  The work array's input image
//   is swizzled slot(p) = p ^ (((p >> 6) & 3) << 2): the chain stores (32
//   lanes x 8 B per half-wave) and the stage-1 gathers (16-B points) are both
//   bank-conflict free, and all addresses are per-thread bases + immediates.
// - Profile-uniform conditions (fit status, w0 == 0 / 1) are scalar branches.
// DIAG_CLOSED first forms the closed-form amplitude over the same chains (the
// stored order: the products T_i p_i of the lane's samples j, i = (j - sh) mod
// N, with the template gathered for the residual).
template <int N, int MODE>
__global__ __launch_bounds__(CLay<N>::L * CLay<N>::GPB, 4) void k_diag_cl(DiagArgs a)
{
    using C = CLay<N>;
    constexpr int L = C::L, WPP = C::WPP, M = C::M;
    constexpr bool closed = MODE == DIAG_CLOSED;
    constexpr bool stats = MODE == DIAG_STATS;   // X = f32(D_row * w): the rows are the residual
    constexpr bool twder = WPP > 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const double2 *tw = C::TWG ? a.tw_p2 : (const double2 *)smem;
    const int lane = threadIdx.x & 63;
    const int group = WPP == 1 ? (int)(threadIdx.x >> 6) : 0;
    const int gpb = WPP == 1 ? (int)(blockDim.x >> 6) : 1;
    const int wave = WPP == 1 ? 0 : (int)(threadIdx.x >> 6);
    int t = WPP == 1 ? lane : (int)threadIdx.x;
    if (!C::TWG) {
        for (int q = threadIdx.x; q < C::TW_LDS; q += blockDim.x) ((double2 *)smem)[q] = a.tw_p2[q];
        __syncthreads();
    }
    unsigned char *gb = smem + (size_t)C::TW_LDS * 16 + (size_t)group * C::GROUP_BYTES;
    double2 *Cb = (double2 *)gb;
    double *red = (double *)(gb + C::CBYTES);
    const unsigned P = (unsigned)a.nsub * (unsigned)a.nchan;
    const unsigned stride = gridDim.x * gpb;
    const unsigned nchan = (unsigned)a.nchan;
    // profiles: all P, or the slots of a list, minus those with skip[k] != 0
    // (the two passes of the fit's forked diagnostics)
    const RoundList rl(a.list, a.nctr, (long)P);
    const unsigned nslot = (unsigned)rl.n();
    const uint8_t *skip = a.skip;
    // The group's upcoming slots, 64 at a time: lane j of each wave holds the
    // profile of slot wb0 + j stride (-1: past the end, or skipped), so the next
    // profile is a ballot bit away and the list and skip reads are one batch per
    // 64 profiles, where a dependent pair of reads per profile stalled the
    // prefetch of the next row (list and skip passes of the fork).
    unsigned wb0 = 0;
    int wkk = -1;
    unsigned long long wmask = 0;
    auto fill = [&](unsigned b) {
        wb0 = b;
        const unsigned sl = b + (unsigned)lane * stride;
        int kk = -1;
        if (sl < nslot && sl >= b) {
            kk = (int)rl.at(sl);
            if (skip && skip[kk]) kk = -1;
        }
        wkk = kk;
        wmask = __ballot(kk >= 0);
    };
    auto take = [&]() -> int {   // the next profile of the group (uniform), -1 when done
        while (wmask == 0) {
            const unsigned nb = wb0 + 64u * stride;
            if (nb >= nslot || nb < wb0) return -1;
            fill(nb);
        }
        const int j = __builtin_ctzll(wmask);
        wmask &= wmask - 1;
        return __builtin_amdgcn_readlane(wkk, j);
    };
    // a VGPR zero: the per-profile scalars of the next profile are read by
    // vector loads (counted on vmcnt), not scalar ones, whose lgkmcnt would be
    // waited on by the FFT's LDS waits
    int zv;
    asm volatile("v_mov_b32 %0, 0" : "=v"(zv));
    const int ca = t >> 3, cc = t & 7;
    const int jb = 128 * ca + cc;   // first sample of the thread's chain
    // byte offsets in the work array: d of chain sample q at wb[q & 3] + 64 (q & ~3)
    // (point p = jb/2 + 4q, part cc & 1); stage-1 point t + L r at rb[r & 3] + 16 L r
    int wb[4], rb[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        wb[m] = 16 * (64 * ca + ((4 * m + (cc >> 1)) ^ (4 * (ca & 3)))) + 8 * (cc & 1);
        rb[m] = 16 * (t ^ ((((t >> 6) + (L / 64) * m) & 3) << 2));
    }
    float pv[16];
    auto loadrow = [&](unsigned kk) {
        const float *pn = (stats ? a.D : a.raw) + (size_t)kk * N + jb;
#pragma unroll
        for (int q = 0; q < 16; ++q) pv[q] = pn[8 * q];
    };
    fill(__builtin_amdgcn_readfirstlane(blockIdx.x * gpb + group));
    int kq = take();
    unsigned k = kq >= 0 ? (unsigned)kq : 0u;
    double nx = 0.0;
    int nst = 0, nsh = 0;
    float nw = 0.0f, nb = 0.0f;
    auto prefetch = [&](unsigned kk) {
        loadrow(kk);
        const unsigned kv = kk + (unsigned)zv;
        if (!closed && !stats) {
            nx = a.amp[kv];
            nst = a.info[kv];
        }
        if (!stats) {
            nb = a.base[kv];
            nsh = a.shift[kk % nchan + (unsigned)zv];
        }
        nw = a.w0[kv];
    };
    if (kq >= 0) prefetch(k);
    for (; kq >= 0;) {
        // multi-wave groups: keep the FFT's LDS addresses inside the loop (hoisted,
        // they spill at N >= 2048; k_diag_p2); one wave: hoisted, 118 VGPRs
        if (WPP > 1) asm volatile("" : "+v"(t));
        double x = ufirst(nx);
        int st = ufirst(nst);
        const float w = ufirst(nw);
        const float bk = nb;
        const int sh = ufirst(nsh);
        // template at the dedispersed index of every chain sample
        double tg[16];
        if constexpr (!stats) {
            const double *tb = a.T2 + ((unsigned)(jb - sh) & (unsigned)(N - 1));
#pragma unroll
            for (int q = 0; q < 16; ++q) tg[q] = tb[8 * q];
        }
        if constexpr (closed) {
            // a = sum(T*p)/sum(T*T) over the chains of the stored (dispersed)
            // order: the lane's samples j = jb + 8q with p = f32(raw_j - base),
            // the dedispersed bin i = (j - sh) mod N, T_i = tg[q] (the
            // residual's gather): no second read of the row (round 6; before,
            // the dot ran over the dedispersed chains and gathered raw at
            // (i + sh) mod N again)
            double r = tg[0] * (double)(pv[0] - bk);
#pragma unroll
            for (int q = 1; q < 16; ++q) {
                const double pr = tg[q] * (double)(pv[q] - bk);
                r = r + pr;
            }
            double cs[1] = {r};
            const double dot = 0.0 + chain_total<N, double>(cs, red, wave, lane);
            const double TT = *a.TT;
            x = ufirst(TT != 0.0 ? dot / TT : 0.0);
            st = isfinite(x) ? 1 : 5;
            if (t == 0) {
                a.amp[k] = x;
                a.info[k] = st;
            }
        }
        // residual (ic.py:279-288) of the dispersed-frame sample j, f32 store
        // (:272), apply_weights (:296): X_j = f32(f32(x T_i - D_i) * w), D_i = f32(raw_j - base0)
        const bool ok = stats || (st >= 1 && st <= 4);   // fit_ok, restated: the call moved the closed mode's code
        const bool valid = w != 0.0f;
        float X[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            if constexpr (stats) {
                X[q] = pv[q];
            } else {
                const float pj = pv[q] - bk;
                const double e = x * tg[q] - (double)pj;
                X[q] = (float)e;
            }
        }
        if (w != 1.0f) {   // fractional weights (w * 1 = w exactly: skipped)
#pragma unroll
            for (int q = 0; q < 16; ++q) X[q] = X[q] * w;
        }
        if (!ok) {   // a bad leastsq status zeroes the residual (ic.py:284-286)
            asm volatile("");   // a rare branch, not 16 selects on every profile
#pragma unroll
            for (int q = 0; q < 16; ++q) X[q] = 0.0f * w;
        }
        const unsigned kc = k;   // this profile (the prefetch below moves k on)
        kq = take();
        if (kq >= 0) {
            k = (unsigned)kq;
            prefetch(k);
        }
        double mean = 0.0, sd = 0.0, fftv = 0.0, ptp = ptp_fill(false);
        if (valid) {
            // mean: f32 chain, then the pairwise tree (ic.py:207)
            // (this chain arithmetic is restated in rot_stats, ic_rotate.hip: edit both.  A
            // shared helper changed the operand order of the adds in the machine code)
            float s = X[0];
#pragma unroll
            for (int q = 1; q < 16; ++q) s = s + X[q];
            float fs[1] = {s};
            const float s32 = 0.0f + chain_total<N, float>(fs, (float *)(red + 16), wave, lane);
            mean = (double)s32 / (double)N;
            // the previous profile's spectrum reads are done before d overwrites the array
            gsync<WPP>();
            // var (ic.py:206): f64 pairwise sum of (f64(X) - mean)^2; d -> FFT input
            double r = 0.0;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const double d = (double)X[q] - mean;
                const double sq = d * d;
                r = q == 0 ? sq : r + sq;
                *(double *)(gb + wb[q & 3] + 64 * (q & ~3)) = d;
            }
            double rs[1] = {r};
            const double ss = 0.0 + chain_total<N, double>(rs, red + 24, wave, lane);
            sd = sqrt(ss / (double)N);
            // ptp (ic.py:208), NaN-propagating
            float mx = -INFINITY, mn = INFINITY;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                mx = OpMaxF()(mx, X[q]);
                mn = OpMinF()(mn, X[q]);
            }
            mx = group_tree<WPP, 64>(mx, OpMaxF(), (float *)(red + 32), wave, lane);
            mn = group_tree<WPP, 64>(mn, OpMinF(), (float *)(red + 36), wave, lane);
            int nan = 0;
            if (isnan(s32)) {
#pragma unroll
                for (int q = 0; q < 16; ++q) nan |= isnan(X[q]);
                nan = group_tree<WPP, 64>(nan, OpOr(), (int *)(red + 40), wave, lane);
            }
            ptp = nan ? (double)NAN : (double)(float)(mx - mn);
            // rFFT of d (ic.py:210-212): stage 1 (radix 8, no twiddles) from the
            // swizzled input image, then k_diag_p2's stages
            gsync<WPP>();
            double2 v[8];
#pragma unroll
            for (int r8 = 0; r8 < 8; ++r8) v[r8] = *(const double2 *)(gb + rb[r8 & 3] + 16 * L * r8);
            gsync<WPP>();
            dft_small<8>(v);
            {
                const int A = 8 * t + (t & 7);   // cidx(8t + r) = A ^ r
#pragma unroll
                for (int r8 = 0; r8 < 8; ++r8) Cb[A ^ r8] = v[r8];
            }
            gsync<WPP>();
            p2_fft<M, L, C::LG, 3, 8, M, float, twder>(Cb, (const float *)nullptr, 0.0, tw, t);
            // spectrum in conjugate bin pairs (k_diag_p2).  No NaN bookkeeping:
            // a finite f32 sum s32 means every X is finite, and then every d,
            // Z and |X_k|^2 is finite (|X_k|^2 < 1e85); a non-finite s32 (a NaN or
            // Inf sample, or an f32 overflow: d = -Inf) makes some bin NaN in
            // any FFT order, so numpy's max|rfft| is NaN (ic.py:210-212)
            constexpr int H = M / 2;
            constexpr int JF = H / L;
            double best2 = 0.0;
            static_assert(JF == 4 && 16 * L == N, "tw[t + L j] = tw[t] exp(-2 pi i j / 16)");
            const double2 wt = tw[t];
#pragma unroll
            for (int j = 0; j < JF; ++j) {
                const int kk = t + L * j;
                const double2 zk = Cb[cidx(t) + L * j];
                const double2 zm = Cb[kk == 0 ? 0 : cidx(L - t) + (M - L * (j + 1))];
                if (twder) {
                    // exp(-2 pi i j / 16), j = 0..3
                    constexpr double c16[4] = {1.0, 0.92387953251128675613, 0.70710678118654752440,
                                               0.38268343236508977173};
                    constexpr double s16[4] = {0.0, 0.38268343236508977173, 0.70710678118654752440,
                                               0.92387953251128675613};
                    const double2 wj = make_double2(c16[j], -s16[j]);
                    spec_pair(zk, zm, j == 0 ? wt : cmul_f(wt, wj), best2);
                } else {
                    spec_pair(zk, zm, tw[kk], best2);
                }
            }
            spec_self_pair(Cb[cidx(H)], tw[H], best2);   // k = M/2 (one task, on every lane)
            best2 = group_tree<WPP, 64>(best2, OpMaxF(), red + 44, wave, lane);
            fftv = isfinite(s32) ? 0.5 * sqrt(best2) : (double)NAN;
        } else {
            // invalid: rfft of f64(X) = +-0 -> 0, unless R was non-finite (X NaN)
            int nanx = 0;
#pragma unroll
            for (int q = 0; q < 16; ++q) nanx |= isnan(X[q]);
            nanx = group_tree<WPP, 64>(nanx, OpOr(), (int *)(red + 52), wave, lane);
            fftv = nanx ? NAN : 0.0;
        }
        if (t == 0) diag_store(a, kc, valid, mean, sd, ptp, fftv);
    }
}

// ---------------------------------------------------------------------------
// k_diag_mr: k_diag's diagnostics for the mixed-radix lengths (mr_supported:
// n = 2M, M = 2^a 3^b 5^c, n a multiple of 8, 64 .. 4096), n a runtime value.
// A profile group of W = ceil(n / 1024) waves cleans one profile: MW = false,
// one wave per profile and independent waves in a block that share the f64
// twiddle table in LDS; MW = true, the block is one group of 2 .. 4 waves and
// the table is read through L1/L2 (k_diag_p2's two forms).  PPT: complex points
// a thread holds (M <= 64 W PPT), so a thread has 2 PPT samples of the row.
// Per group the LDS holds one work array: the X image (f32, or f64 for f64
// data) that the statistics read, then, in place, the M complex points of the
// rFFT at pad(q) = q + q/8 (a radix-R first stage scatters at a stride of R
// points: unpadded, the lanes of a 16-byte store share 2 or 4 bank groups);
// every input of a stage is in registers before the group writes.  DIAG_CLOSED
// adds the f32 fit-cube row.
// mean / std / ptp / amp: k_diag's arithmetic, bit for bit: the numpy pairwise
// order of the PwPlan (wave_pairwise's chains and leaf sums, spread over the
// group), whose post-order adds run in registers: every MR length has at most
// 32 leaves, so slot s of the plan lives in lane s of the group's first wave
// and an add is two lane reads.  fftmax: Stockham stages in mr_plan's order
// (FMA allowed, as in k_diag_p2), then the conjugate-pair step (spec_pair_nan;
// k = 0 is the DC / Nyquist pair, k = M/2 pairs with itself).  Nothing depends
// on the launch: a profile's four values are the same bits from a full pass, a
// list, a skip pass or any grid.
struct MrLayout {
    size_t tw_bytes, plan_off, groups_off;       // block: twiddles (MW = false), leaf table, groups
    size_t p_off, acc_off, red_off, per_group;   // group: work array at 0, closed-mode row, pairwise, partials
};

__host__ __device__ inline MrLayout mr_layout(int n, bool mw, bool d64, bool closed)
{
    MrLayout L;
    const int M = n / 2, nlub = n / 64 + 1;   // leaves hold >= 64 samples
    L.tw_bytes = mw ? 0 : (size_t)n * 16;
    L.plan_off = L.tw_bytes;
    L.groups_off = L.plan_off + (((size_t)nlub * 8 + 15) & ~(size_t)15);
    const size_t cb = (size_t)(M + M / 8 + 1) * 16, xb = (size_t)n * (d64 ? 8 : 4);
    const size_t work = ((cb > xb ? cb : xb) + 15) & ~(size_t)15;
    L.p_off = work;
    L.acc_off = L.p_off + (closed ? (((size_t)n * 4 + 15) & ~(size_t)15) : 0);
    L.red_off = L.acc_off + (size_t)nlub * 64;   // 8 chain sums of 8 B per leaf
    L.per_group = L.red_off + 32 * 8;
    return L;
}

__device__ __forceinline__ int mr_pad(int q) { return q + (q >> 3); }

// the PwPlan as the kernel keeps it: leaf starts / lengths in LDS, the adds
// packed op_a | op_b << 16 in lane o of every wave
struct MrPlan {
    const int32_t *ls, *ll;
    int nl, nops, root, opv;
};

// wave_pairwise over a group of tpp threads (t: thread of the group): the same
// chains, leaf sums and post-order adds, so the same bits.  acc: 8 nl slots of
// Tp; res: one slot (MW).  Leaves of an MR length hold >= 8 samples.
template <bool MW, typename Tp, typename Get>
__device__ __forceinline__ Tp mr_pairwise(const MrPlan &pl, Get get, Tp *acc, Tp *res, int t, int tpp)
{
    const int nl = pl.nl;
    for (int task = t; task < nl * 8; task += tpp) {
        const int Lf = task >> 3, j = task & 7;
        const int st = pl.ls[Lf], len = pl.ll[Lf];
        const int main = len - len % 8;
        Tp r = get(st + j);
        for (int q = 8; q < main; q += 8) r = r + get(st + q + j);
        acc[task] = r;
    }
    gsync<MW ? 2 : 1>();
    Tp v = (Tp)0;
    if (t < nl) {
        const int st = pl.ls[t], len = pl.ll[t];
        const Tp *r = acc + t * 8;
        const Tp a01 = r[0] + r[1], a23 = r[2] + r[3], a45 = r[4] + r[5], a67 = r[6] + r[7];
        const Tp lo = a01 + a23, hi = a45 + a67;
        v = lo + hi;
        for (int q = len - len % 8; q < len; ++q) v = v + get(st + q);
    }
    Tp out = (Tp)0;
    if (!MW || t < 64) {   // slot s in lane s: slot[nl + o] = slot[op_a[o]] + slot[op_b[o]]
        for (int o = 0; o < pl.nops; ++o) {
            const int ab = __builtin_amdgcn_readlane(pl.opv, o);
            const Tp s = lane_read(v, ab & 0xffff) + lane_read(v, ab >> 16);
            if (t == nl + o) v = s;
        }
        out = (Tp)0 + lane_read(v, pl.root);
    }
    if constexpr (MW) {
        if (t == 0) res[0] = out;
        __syncthreads();
        out = res[0];
    }
    return out;
}

// group-uniform reduction of a per-thread value (max / min / or: any order)
template <bool MW, typename T, typename Op>
__device__ __forceinline__ T mr_tree(T v, Op op, T *red, int t, int tpp)
{
    const T w = wave_tree<64>(v, op);
    if constexpr (MW) {
        if ((t & 63) == 0) red[t >> 6] = w;
        __syncthreads();
        T r = red[0];
        for (int i = 1; i < (tpp >> 6); ++i) r = op(r, red[i]);
        __syncthreads();
        return r;
    } else {
        return w;
    }
}

// One Stockham stage of radix R and span ns (the product of the earlier
// radices) of the group's FFT_M, in place: butterfly j < G = M/R reads point
// j + q G, multiplies by tw[q k step] (k = j mod ns by a multiply with
// ceil(2^32 / ns), step = n/(R ns); not in the first stage) and writes DFT_R's
// y_p to point (j - k) R + k + p ns.  FIRST: the points are the pairs of the
// real row X minus mu.
template <int R, bool FIRST, int PPT, bool MW, typename XT>
__device__ __forceinline__ void mr_diag_stage(double2 *C, const XT *X, double mu, const double2 *tw, int M, int step,
                                              int ns, int t, int tpp)
{
    constexpr int BPT = (PPT + R - 1) / R;   // butterflies a thread holds
    const int G = M / R;
    const unsigned magic = ns > 1 ? 0xffffffffu / (unsigned)ns + 1u : 0u;
    double2 v[BPT][R];
#pragma unroll
    for (int u = 0; u < BPT; ++u) {
        const int j = t + tpp * u;
        if (j < G) {
#pragma unroll
            for (int q = 0; q < R; ++q) {
                const int pt = j + q * G;
                if constexpr (FIRST) {
                    if constexpr (sizeof(XT) == 8) {
                        const double2 xv = *(const double2 *)(X + 2 * pt);
                        v[u][q] = make_double2(xv.x - mu, xv.y - mu);
                    } else {
                        const float2 xv = *(const float2 *)(X + 2 * pt);
                        v[u][q] = make_double2((double)xv.x - mu, (double)xv.y - mu);
                    }
                } else {
                    v[u][q] = C[mr_pad(pt)];
                }
            }
        }
    }
    gsync<MW ? 2 : 1>();
#pragma unroll
    for (int u = 0; u < BPT; ++u) {
        const int j = t + tpp * u;
        if (j < G) {
            const int k = ns > 1 ? j - (int)__umulhi((unsigned)j, magic) * ns : 0;
            if (!FIRST) {
                double2 w[R];
#pragma unroll
                for (int q = 1; q < R; ++q) w[q] = tw[q * k * step];
#pragma unroll
                for (int q = 1; q < R; ++q) v[u][q] = cmul_f(v[u][q], w[q]);
            }
            dft_small<R>(v[u]);
            const int o = (j - k) * R + k;
#pragma unroll
            for (int p = 0; p < R; ++p) C[mr_pad(o + p * ns)] = v[u][p];
        }
    }
    gsync<MW ? 2 : 1>();
}

template <int PPT, bool MW, bool D64>
__global__ __launch_bounds__(MW ? 256 : 512, PPT > 2 ? 3 : 4) void k_diag_mr(DiagArgs a, unsigned long long radices, int nst)
{
    using XT = typename std::conditional<D64, double, float>::type;
    constexpr int SPT = 2 * PPT;   // samples of the row a thread holds
    extern __shared__ __attribute__((aligned(16))) unsigned char mr_sm[];
    const int n = a.nbin, M = n >> 1, H = M >> 1;
    const int mode = a.mode;
    const int lane = threadIdx.x & 63;
    const int tpp = MW ? (int)blockDim.x : 64;
    int t = MW ? (int)threadIdx.x : lane;
    const int group = MW ? 0 : (int)(threadIdx.x >> 6);
    const int gpb = MW ? 1 : (int)(blockDim.x >> 6);
    const MrLayout lay = mr_layout(n, MW, D64, mode == DIAG_CLOSED);
    const double2 *tw = MW ? a.tw : (const double2 *)mr_sm;
    MrPlan pl;
    {
        int32_t *ls = (int32_t *)(mr_sm + lay.plan_off);
        const int nl = a.plan->nleaf;
        int32_t *ll = ls + nl;
        if (!MW)
            for (int q = threadIdx.x; q < n; q += blockDim.x) ((double2 *)mr_sm)[q] = a.tw[q];
        for (int q = threadIdx.x; q < nl; q += blockDim.x) {
            ls[q] = a.plan->leaf_start[q];
            ll[q] = a.plan->leaf_len[q];
        }
        pl.ls = ls;
        pl.ll = ll;
        pl.nl = nl;
        pl.nops = a.plan->nops;
        pl.root = a.plan->root;
        pl.opv = lane < pl.nops ? (a.plan->op_a[lane] | (a.plan->op_b[lane] << 16)) : 0;
        __syncthreads();
    }
    unsigned char *gb = mr_sm + lay.groups_off + (size_t)group * lay.per_group;
    XT *X = (XT *)gb;
    double2 *C = (double2 *)gb;   // takes X's place once the first stage has read it
    float *Pr = (float *)(gb + lay.p_off);
    double *acc = (double *)(gb + lay.acc_off);
    double *red = (double *)(gb + lay.red_off);
    const unsigned P = (unsigned)a.nsub * (unsigned)a.nchan;
    const unsigned stride = gridDim.x * gpb;
    const double *T64 = a.T64;
    // profiles: all P, or the slots of a list, minus those with skip[k] != 0
    const RoundList rl(a.list, a.nctr, (long)P);
    const unsigned nslot = (unsigned)rl.n();
    const uint8_t *skip = a.skip;
    for (unsigned slot = blockIdx.x * gpb + group; slot < nslot; slot += stride) {
        const unsigned k = (unsigned)rl.at(slot);
        if (skip && skip[k]) continue;   // group-uniform
        // opaque to the optimiser: hoisting the stages' LDS addresses, which
        // derive from t, out of the loop costs ~100 VGPRs (k_diag_p2)
        asm volatile("" : "+v"(t));
        const float w = a.w0[k];
        const bool valid = (w != 0.0f);
        const int sh = mode == DIAG_STATS ? 0 : a.shift[k % (unsigned)a.nchan];
        const bool tr = a.dtiled && mode == DIAG_EXACT;   // the tiled fit cube (dt_ofs)
        // every global load of the row in flight at once: CLOSED the raw row
        // (dispersed order j), otherwise the fit cube / given row (order i)
        float pv[SPT];
#pragma unroll
        for (int u = 0; u < SPT; ++u) {
            const int i = t + tpp * u;
            pv[u] = 0.0f;
            if (i < n) {
                if (mode == DIAG_CLOSED) pv[u] = a.raw[(size_t)k * n + i];
                else pv[u] = a.D[d_ofs(k, i, a.ldD, tr)];
            }
        }
        double x = 0.0;
        int stt = 0;
        gsync<MW ? 2 : 1>();   // the previous profile's LDS reads are done
        if (mode == DIAG_CLOSED) {
            // the fit-cube row f32(ded - base0), dedispersed order, then the
            // closed-form amplitude from numpy pairwise sums over the stored
            // (dispersed) order j: bin i = (j - sh) mod n
            const float b = a.base[k];
#pragma unroll
            for (int u = 0; u < SPT; ++u) {
                const int j = t + tpp * u;
                if (j < n) {
                    int i = j - sh;
                    if (i < 0) i += n;
                    Pr[i] = pv[u] - b;
                }
            }
            gsync<MW ? 2 : 1>();
            const double dot = mr_pairwise<MW, double>(pl, [&](int q) {
                int i = q - sh;
                if (i < 0) i += n;
                return T64[i] * (double)Pr[i];
            }, acc, red, t, tpp);
            const double TT = *a.TT;
            x = TT != 0.0 ? dot / TT : 0.0;
            stt = isfinite(x) ? 1 : 5;
            if (t == 0) {
                a.amp[k] = x;
                a.info[k] = stt;
            }
#pragma unroll
            for (int u = 0; u < SPT; ++u) {
                const int i = t + tpp * u;
                if (i < n) pv[u] = Pr[i];
            }
        } else if (mode == DIAG_EXACT) {
            x = a.amp[k];
            stt = a.info[k];
        }
        const bool ok = fit_ok(stt);
        // residual -> X (dispersed frame): X[j] = f32(f32(r[i]) * w), j = (i + sh) mod n
        // (f64(f32(r[i])) * f64(w) for f64 data); the thread keeps its values for the ptp
        XT xv[SPT];
#pragma unroll
        for (int u = 0; u < SPT; ++u) {
            const int i = t + tpp * u;
            xv[u] = (XT)0;
            if (i < n) {
                float R = 0.0f;
                if (mode == DIAG_STATS) R = pv[u];
                else if (ok) R = residual_sample(x, T64[i], pv[u], i, a);
                int j = i + sh;
                if (j >= n) j -= n;
                if constexpr (D64) xv[u] = (double)R * (double)w;
                else xv[u] = R * w;
                X[j] = xv[u];
            }
        }
        gsync<MW ? 2 : 1>();
        double mean = 0.0, sd = 0.0, fftv = 0.0, ptp = ptp_fill(D64);
        if (valid) {
            // mean: pairwise sum in the data dtype; var: f64 pairwise sum of (f64(X) - mean)^2
            const XT s = mr_pairwise<MW, XT>(pl, [&](int q) { return X[q]; }, (XT *)acc, (XT *)red, t, tpp);
            mean = (double)s / (double)n;
            const double mu = mean;
            const double ss = mr_pairwise<MW, double>(pl, [&](int q) {
                const double d = (double)X[q] - mu;
                return d * d;
            }, acc, red + 1, t, tpp);
            sd = sqrt(ss / (double)n);
            // ptp (NaN-propagating), max - min in the data dtype
            XT mx = -INFINITY, mn = INFINITY;
            int nan = 0;
#pragma unroll
            for (int u = 0; u < SPT; ++u) {
                if (t + tpp * u < n) {
                    nan |= isnan(xv[u]);
                    mx = OpMaxF()(mx, xv[u]);
                    mn = OpMinF()(mn, xv[u]);
                }
            }
            mx = mr_tree<MW>(mx, OpMaxF(), (XT *)(red + 4), t, tpp);
            mn = mr_tree<MW>(mn, OpMinF(), (XT *)(red + 8), t, tpp);
            nan = mr_tree<MW>(nan, OpOr(), (int *)(red + 12), t, tpp);
            ptp = nan ? (double)NAN : (double)(XT)(mx - mn);
            // rFFT of f64(X) - mean: FFT_M in place over the work array
            int ns = 1, step = n;
            for (int st = 0; st < nst; ++st) {
                const int R = (int)((radices >> (4 * st)) & 15);
                step /= R;
                if (st == 0) {   // M is a multiple of 4: the first radix is 8 or 4
                    if (R == 8) mr_diag_stage<8, true, PPT, MW, XT>(C, X, mu, tw, M, step, ns, t, tpp);
                    else mr_diag_stage<4, true, PPT, MW, XT>(C, X, mu, tw, M, step, ns, t, tpp);
                } else {
                    switch (R) {
                    case 8: mr_diag_stage<8, false, PPT, MW, XT>(C, X, mu, tw, M, step, ns, t, tpp); break;
                    case 5: mr_diag_stage<5, false, PPT, MW, XT>(C, X, mu, tw, M, step, ns, t, tpp); break;
                    case 4: mr_diag_stage<4, false, PPT, MW, XT>(C, X, mu, tw, M, step, ns, t, tpp); break;
                    case 3: mr_diag_stage<3, false, PPT, MW, XT>(C, X, mu, tw, M, step, ns, t, tpp); break;
                    default: mr_diag_stage<2, false, PPT, MW, XT>(C, X, mu, tw, M, step, ns, t, tpp); break;
                    }
                }
                ns *= R;
            }
            // the real spectrum in conjugate bin pairs (k_diag_p2): 2 X_k and
            // 2 X_(M-k) from Z_k, Z_(M-k) and w^k = tw[k], k = 0 .. M/2
            double best2 = 0.0, nsum = 0.0;
            for (int kk = t; kk <= H; kk += tpp)
                spec_pair_nan(C[mr_pad(kk)], C[mr_pad(kk == 0 ? 0 : M - kk)], tw[kk], best2, nsum);
            int nanf = isnan(nsum);
            best2 = mr_tree<MW>(best2, OpMaxF(), red + 16, t, tpp);
            nanf = mr_tree<MW>(nanf, OpOr(), (int *)(red + 20), t, tpp);
            fftv = nanf ? NAN : 0.5 * sqrt(best2);
        } else {
            // invalid: rfft of f64(X) = +-0 -> 0, unless R was non-finite (X NaN)
            int nanx = 0;
#pragma unroll
            for (int u = 0; u < SPT; ++u)
                if (t + tpp * u < n) nanx |= isnan(xv[u]);
            nanx = mr_tree<MW>(nanx, OpOr(), (int *)(red + 12), t, tpp);
            fftv = nanx ? NAN : 0.0;
        }
        if (t == 0) diag_store(a, k, valid, mean, sd, ptp, fftv);
    }
}

// ---------------------------------------------------------------------------
// k_diag_czt: k_diag's diagnostics for the other lengths (diag_czt_supported:
// 129 .. 4096, neither a power of two nor mixed-radix; odd and prime lengths
// to 2048 included; the kernel itself takes any n in 16 .. 4096 whose L <=
// 4096), n a runtime value.  std / mean / ptp / amp are k_diag's
// arithmetic, bit for bit, in k_diag_mr's form (the row image in LDS, the
// PwPlan's chains and leaf sums spread over the group, the post-order adds in
// the lanes of the first wave).  fftmax replaces the direct O(n^2) DFT by a
// chirp-z (Bluestein) transform in f64 (diag_czt.py states it in numpy):
//   even n: Z = DFT_m of z[q] = v[2q] + i v[2q+1], m = n/2 (odd m included),
//           then the conjugate-pair step over k = 0 .. m/2 (spec_pair_nan: for
//           an odd m no bin pairs with itself, and the pairs (k, m - k) of
//           k <= (m-1)/2 still cover 0 .. m);
//   odd n:  DFT_n of the real row, bins 0 .. (n-1)/2;
//   DFT_m:  a = z w zero-padded to L = czt_length(m), A = FFT_L(a), times the
//           per-length filter B / L, the inverse FFT_L as the conjugate of a
//           forward one, times w: Z_k = w_k conj(c_k), w_j = exp(-i pi j^2/m).
//           |w| = 1, so the odd lengths take |c_k| directly.
// The per-length tables (DiagArgs.czt, f64 pairs): [L] exp(-2 pi i q/L), [L]
// B / L, [m] w.  The FFT_L are mr_plan(2 L)'s radix 8 / 4 / 2 Stockham stages, in
// place over one work array per group at mr_pad (k_diag_mr's stage); the first
// stage of each FFT forms its input on the fly (a from the row image, which
// the work array then overwrites; conj(A B) from the array itself).  A group is
// one wave while L <= 512, with the twiddles of L in LDS (MW = false), and
// L/512 = 2 .. 8 waves above, with the twiddles read through L1/L2 (MW = true):
// the work array bounds the profiles a CU holds, so more waves around one
// array is what fills the SIMDs, and 8 points per thread is what fits the
// registers without a spill.  B and w are read from global memory by every
// profile and stay cache-resident.  PPT: points of the work array a thread
// holds (L <= 64 W PPT), which is also the samples of the row it holds (n <=
// L).  Nothing depends on the launch.
__host__ __device__ inline MrLayout czt_layout(int n, int L, bool mw, bool d64, bool closed)
{
    MrLayout lay;
    const int nlub = n / 64 + 1;   // leaves hold >= 64 samples
    lay.tw_bytes = mw ? 0 : (size_t)L * 16;
    lay.plan_off = lay.tw_bytes;
    lay.groups_off = lay.plan_off + (((size_t)nlub * 8 + 15) & ~(size_t)15);
    const size_t cb = (size_t)(L + L / 8 + 1) * 16, xb = (size_t)n * (d64 ? 8 : 4);
    const size_t work = ((cb > xb ? cb : xb) + 15) & ~(size_t)15;
    lay.p_off = work;
    lay.acc_off = lay.p_off + (closed ? (((size_t)n * 4 + 15) & ~(size_t)15) : 0);
    lay.red_off = lay.acc_off + (size_t)nlub * 64;   // 8 chain sums of 8 B per leaf
    lay.per_group = lay.red_off + 40 * 8;   // k_diag_czt's partials: up to 8 waves
    return lay;
}

// mr_pairwise without its limit of 32 leaves (4094 bins have 33): slot s of the
// plan lives in lane s & 63 of the group's first wave, register s >> 6, so up
// to 64 leaves and 128 slots.  The same chains, leaf sums and post-order adds,
// so the same bits.
template <bool MW, typename Tp, typename Get>
__device__ __forceinline__ Tp czt_pairwise(const MrPlan &pl, Get get, Tp *acc, Tp *res, int t, int tpp)
{
    const int nl = pl.nl;
    for (int task = t; task < nl * 8; task += tpp) {
        const int Lf = task >> 3, j = task & 7;
        const int st = pl.ls[Lf], len = pl.ll[Lf];
        const int main = len - len % 8;
        Tp r = get(st + j);
        for (int q = 8; q < main; q += 8) r = r + get(st + q + j);
        acc[task] = r;
    }
    gsync<MW ? 2 : 1>();
    Tp v0 = (Tp)0, v1 = (Tp)0;
    if (t < nl) {
        const int st = pl.ls[t], len = pl.ll[t];
        const Tp *r = acc + t * 8;
        const Tp a01 = r[0] + r[1], a23 = r[2] + r[3], a45 = r[4] + r[5], a67 = r[6] + r[7];
        const Tp lo = a01 + a23, hi = a45 + a67;
        v0 = lo + hi;
        for (int q = len - len % 8; q < len; ++q) v0 = v0 + get(st + q);
    }
    Tp out = (Tp)0;
    if (!MW || t < 64) {   // slot[nl + o] = slot[op_a[o]] + slot[op_b[o]]
        const auto slot = [&](int s) { return s < 64 ? lane_read(v0, s) : lane_read(v1, s - 64); };
        for (int o = 0; o < pl.nops; ++o) {
            const int ab = __builtin_amdgcn_readlane(pl.opv, o);
            const Tp s = slot(ab & 0xffff) + slot(ab >> 16);
            const int d = nl + o;
            if (t == d) v0 = s;
            if (t == d - 64) v1 = s;
        }
        out = (Tp)0 + slot(pl.root);
    }
    if constexpr (MW) {
        if (t == 0) res[0] = out;
        __syncthreads();
        out = res[0];
    }
    return out;
}

// One radix-R Stockham stage of the group's FFT_L (L and ns powers of two), in
// place: butterfly j < G = L/R takes the points get(j + q G) into registers,
// multiplies by tw[q k step] (k = j mod ns, step = L/(R ns); not in a first
// stage, ns = 1) and, once the whole group has read, writes DFT_R's y_p to
// point (j - k) R + k + p ns.
template <int R, int PPT, bool MW, typename Get>
__device__ __forceinline__ void czt_stage(double2 *C, Get get, const double2 *tw, int L, int step, int ns, int t,
                                          int tpp)
{
    constexpr int BPT = (PPT + R - 1) / R;   // butterflies a thread holds
    const int G = L / R;
    double2 v[BPT][R];
#pragma unroll
    for (int u = 0; u < BPT; ++u) {
        const int j = t + tpp * u;
        if (j < G) {
#pragma unroll
            for (int q = 0; q < R; ++q) v[u][q] = get(j + q * G);
        }
    }
    gsync<MW ? 2 : 1>();
#pragma unroll
    for (int u = 0; u < BPT; ++u) {
        const int j = t + tpp * u;
        if (j < G) {
            const int k = j & (ns - 1);
            if (ns > 1) {
                double2 w[R];
#pragma unroll
                for (int q = 1; q < R; ++q) w[q] = tw[q * k * step];
#pragma unroll
                for (int q = 1; q < R; ++q) v[u][q] = cmul_f(v[u][q], w[q]);
            }
            dft_small<R>(v[u]);
            const int o = (j - k) * R + k;
#pragma unroll
            for (int p = 0; p < R; ++p) C[mr_pad(o + p * ns)] = v[u][p];
        }
    }
    gsync<MW ? 2 : 1>();
}

template <int PPT, bool MW, bool D64>
__global__ __launch_bounds__(512, 3) void k_diag_czt(DiagArgs a, unsigned long long radices,
                                                                             int nst, int L)
{
    using XT = typename std::conditional<D64, double, float>::type;
    extern __shared__ __attribute__((aligned(16))) unsigned char cz_sm[];
    const int n = a.nbin;
    const bool even = !(n & 1);
    const int m = even ? n >> 1 : n;          // the Bluestein DFT's length
    const int H = even ? m >> 1 : n >> 1;     // the last pair task (even n) / bin (odd n)
    const int mode = a.mode;
    const int lane = threadIdx.x & 63;
    const int tpp = MW ? (int)blockDim.x : 64;
    int t = MW ? (int)threadIdx.x : lane;
    const int group = MW ? 0 : (int)(threadIdx.x >> 6);
    const int gpb = MW ? 1 : (int)(blockDim.x >> 6);
    const MrLayout lay = czt_layout(n, L, MW, D64, mode == DIAG_CLOSED);
    const double2 *tw = MW ? a.czt : (const double2 *)cz_sm;   // exp(-2 pi i q/L)
    const double2 *Bf = a.czt + L;                             // the filter, scaled by 1/L
    const double2 *ch = a.czt + 2 * (size_t)L;                 // the chirp w[m]
    MrPlan pl;
    {
        int32_t *ls = (int32_t *)(cz_sm + lay.plan_off);
        const int nl = a.plan->nleaf;
        int32_t *ll = ls + nl;
        if (!MW)
            for (int q = threadIdx.x; q < L; q += blockDim.x) ((double2 *)cz_sm)[q] = a.czt[q];
        for (int q = threadIdx.x; q < nl; q += blockDim.x) {
            ls[q] = a.plan->leaf_start[q];
            ll[q] = a.plan->leaf_len[q];
        }
        pl.ls = ls;
        pl.ll = ll;
        pl.nl = nl;
        pl.nops = a.plan->nops;
        pl.root = a.plan->root;
        pl.opv = lane < pl.nops ? (a.plan->op_a[lane] | (a.plan->op_b[lane] << 16)) : 0;
        __syncthreads();
    }
    unsigned char *gb = cz_sm + lay.groups_off + (size_t)group * lay.per_group;
    XT *X = (XT *)gb;
    double2 *C = (double2 *)gb;   // takes X's place once the first stage has read it
    float *Pr = (float *)(gb + lay.p_off);
    double *acc = (double *)(gb + lay.acc_off);
    double *red = (double *)(gb + lay.red_off);
    const unsigned P = (unsigned)a.nsub * (unsigned)a.nchan;
    const unsigned stride = gridDim.x * gpb;
    const double *T64 = a.T64;
    // profiles: all P, or the slots of a list, minus those with skip[k] != 0
    const RoundList rl(a.list, a.nctr, (long)P);
    const unsigned nslot = (unsigned)rl.n();
    const uint8_t *skip = a.skip;
    for (unsigned slot = blockIdx.x * gpb + group; slot < nslot; slot += stride) {
        const unsigned k = (unsigned)rl.at(slot);
        if (skip && skip[k]) continue;   // group-uniform
        // opaque to the optimiser: the stages' LDS addresses derive from t (k_diag_p2)
        asm volatile("" : "+v"(t));
        const float w = a.w0[k];
        const bool valid = (w != 0.0f);
        const int sh = mode == DIAG_STATS ? 0 : a.shift[k % (unsigned)a.nchan];
        const bool tr = a.dtiled && mode == DIAG_EXACT;   // the tiled fit cube (dt_ofs)
        // every global load of the row in flight at once: CLOSED the raw row
        // (dispersed order j), otherwise the fit cube / given row (order i)
        float pv[PPT];
#pragma unroll
        for (int u = 0; u < PPT; ++u) {
            const int i = t + tpp * u;
            pv[u] = 0.0f;
            if (i < n) {
                if (mode == DIAG_CLOSED) pv[u] = a.raw[(size_t)k * n + i];
                else pv[u] = a.D[d_ofs(k, i, a.ldD, tr)];
            }
        }
        double x = 0.0;
        int stt = 0;
        gsync<MW ? 2 : 1>();   // the previous profile's LDS reads are done
        if (mode == DIAG_CLOSED) {
            // the fit-cube row f32(ded - base0), dedispersed order, then the
            // closed-form amplitude from numpy pairwise sums over the stored
            // (dispersed) order j: bin i = (j - sh) mod n
            const float b = a.base[k];
#pragma unroll
            for (int u = 0; u < PPT; ++u) {
                const int j = t + tpp * u;
                if (j < n) {
                    int i = j - sh;
                    if (i < 0) i += n;
                    Pr[i] = pv[u] - b;
                }
            }
            gsync<MW ? 2 : 1>();
            const double dot = czt_pairwise<MW, double>(pl, [&](int q) {
                int i = q - sh;
                if (i < 0) i += n;
                return T64[i] * (double)Pr[i];
            }, acc, red, t, tpp);
            const double TT = *a.TT;
            x = TT != 0.0 ? dot / TT : 0.0;
            stt = isfinite(x) ? 1 : 5;
            if (t == 0) {
                a.amp[k] = x;
                a.info[k] = stt;
            }
#pragma unroll
            for (int u = 0; u < PPT; ++u) {
                const int i = t + tpp * u;
                if (i < n) pv[u] = Pr[i];
            }
        } else if (mode == DIAG_EXACT) {
            x = a.amp[k];
            stt = a.info[k];
        }
        const bool ok = fit_ok(stt);
        // residual -> X (dispersed frame): X[j] = f32(f32(r[i]) * w), j = (i + sh) mod n
        // (f64(f32(r[i])) * f64(w) for f64 data); the thread keeps its values for the ptp
        XT xv[PPT];
#pragma unroll
        for (int u = 0; u < PPT; ++u) {
            const int i = t + tpp * u;
            xv[u] = (XT)0;
            if (i < n) {
                float R = 0.0f;
                if (mode == DIAG_STATS) R = pv[u];
                else if (ok) R = residual_sample(x, T64[i], pv[u], i, a);
                int j = i + sh;
                if (j >= n) j -= n;
                if constexpr (D64) xv[u] = (double)R * (double)w;
                else xv[u] = R * w;
                X[j] = xv[u];
            }
        }
        gsync<MW ? 2 : 1>();
        double mean = 0.0, sd = 0.0, fftv = 0.0, ptp = ptp_fill(D64);
        // a non-finite sample: fftmax is NaN (numpy's rfft spreads it over every bin)
        int nanx = 0;
#pragma unroll
        for (int u = 0; u < PPT; ++u)
            if (t + tpp * u < n) nanx |= !isfinite(xv[u]);
        if (valid) {
            // mean: pairwise sum in the data dtype; var: f64 pairwise sum of (f64(X) - mean)^2
            const XT s = czt_pairwise<MW, XT>(pl, [&](int q) { return X[q]; }, (XT *)acc, (XT *)red, t, tpp);
            mean = (double)s / (double)n;
            const double mu = mean;
            const double ss = czt_pairwise<MW, double>(pl, [&](int q) {
                const double d = (double)X[q] - mu;
                return d * d;
            }, acc, red + 1, t, tpp);
            sd = sqrt(ss / (double)n);
            // ptp (NaN-propagating), max - min in the data dtype
            XT mx = -INFINITY, mn = INFINITY;
            int nan = 0;
#pragma unroll
            for (int u = 0; u < PPT; ++u) {
                if (t + tpp * u < n) {
                    nan |= isnan(xv[u]);
                    mx = OpMaxF()(mx, xv[u]);
                    mn = OpMinF()(mn, xv[u]);
                }
            }
            mx = mr_tree<MW>(mx, OpMaxF(), (XT *)(red + 2), t, tpp);
            mn = mr_tree<MW>(mn, OpMinF(), (XT *)(red + 10), t, tpp);
            nan = mr_tree<MW>(nan, OpOr(), (int *)(red + 18), t, tpp);
            ptp = nan ? (double)NAN : (double)(XT)(mx - mn);
            // a = (f64(X) - mean as complex pairs, or as a real row) w, zero-padded to L
            const auto in = [&](int p) -> double2 {
                if (p >= m) return make_double2(0.0, 0.0);
                const double2 wv = ch[p];
                if (even) return cmul_f(make_double2((double)X[2 * p] - mu, (double)X[2 * p + 1] - mu), wv);
                const double re = (double)X[p] - mu;
                return make_double2(re * wv.x, re * wv.y);
            };
            // conj(A B / L): the inverse FFT_L is the conjugate of a forward one of this
            const auto mid = [&](int p) -> double2 {
                const double2 y = cmul_f(C[mr_pad(p)], Bf[p]);
                return make_double2(y.x, -y.y);
            };
            const auto pt = [&](int p) -> double2 { return C[mr_pad(p)]; };
            for (int f = 0; f < 2; ++f) {
                int ns = 1, step = L;
                for (int st = 0; st < nst; ++st) {
                    const int R = (int)((radices >> (4 * st)) & 15);
                    step /= R;
                    if (st == 0) {   // L >= 16: the first radix is 8
                        if (f == 0) czt_stage<8, PPT, MW>(C, in, tw, L, step, ns, t, tpp);
                        else czt_stage<8, PPT, MW>(C, mid, tw, L, step, ns, t, tpp);
                    } else {
                        switch (R) {
                        case 8: czt_stage<8, PPT, MW>(C, pt, tw, L, step, ns, t, tpp); break;
                        case 4: czt_stage<4, PPT, MW>(C, pt, tw, L, step, ns, t, tpp); break;
                        default: czt_stage<2, PPT, MW>(C, pt, tw, L, step, ns, t, tpp); break;
                        }
                    }
                    ns *= R;
                }
            }
            // C holds c_k = conj(y_k), and Z_k = w_k y_k.  Even n: the real spectrum in
            // conjugate bin pairs (k_diag_p2), 2 X_k and 2 X_(m-k) from Z_k, Z_(m-k) and
            // exp(-2 pi i k/n), k = 0 .. m/2; odd n: |X_k| = |c_k|, k = 0 .. (n-1)/2
            double best2 = 0.0, nsum = 0.0;
            if (even) {
                const auto Z = [&](int q) -> double2 {
                    const double2 c = C[mr_pad(q)];
                    return cmul_f(make_double2(c.x, -c.y), ch[q]);
                };
                for (int kk = t; kk <= H; kk += tpp)
                    spec_pair_nan(Z(kk), Z(kk == 0 ? 0 : m - kk), a.tw[kk], best2, nsum);
            } else {
                for (int kk = t; kk <= H; kk += tpp) {
                    const double2 c = C[mr_pad(kk)];
                    const double a2 = __builtin_fma(c.x, c.x, c.y * c.y);
                    nsum = nsum + a2;
                    best2 = fmax(best2, a2);
                }
            }
            int nanf = isnan(nsum) | nanx;
            best2 = mr_tree<MW>(best2, OpMaxF(), red + 22, t, tpp);
            nanf = mr_tree<MW>(nanf, OpOr(), (int *)(red + 30), t, tpp);
            fftv = nanf ? NAN : (even ? 0.5 * sqrt(best2) : sqrt(best2));
        } else {
            // invalid: rfft of f64(X) = +-0 -> 0, unless R was non-finite (X NaN)
            nanx = mr_tree<MW>(nanx, OpOr(), (int *)(red + 18), t, tpp);
            fftv = nanx ? NAN : 0.0;
        }
        if (t == 0) diag_store(a, k, valid, mean, sd, ptp, fftv);
    }
}

// residual cube on request (ic_get_residual): R (dispersed frame, unweighted).
// D == nullptr (fit_mode 1 keeps no fit cube): the fit-cube row is formed from
// raw and the w0 baseline as in k_chan_partials mode 3, f32(ded - base).
__global__ __launch_bounds__(256) void k_residual(const float *__restrict__ D, const float *__restrict__ raw,
                                                  const float *__restrict__ base, const double *__restrict__ T64,
                                                  const double *__restrict__ amp, const int32_t *__restrict__ info,
                                                  const int32_t *__restrict__ shift, size_t P, int nchan, int nbin,
                                                  int ldD, int dtiled, int pr_on, double pr_factor, int pr_start,
                                                  int pr_end, float *__restrict__ R)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (size_t k = (size_t)blockIdx.x * 4 + wave; k < P; k += (size_t)gridDim.x * 4) {
        const int sh = shift[k % nchan];
        const bool ok = fit_ok(info[k]);
        const double a = amp[k];
        const float b = D ? 0.0f : base[k];
        for (int i = lane; i < nbin; i += 64) {
            int j = i + sh;
            if (j >= nbin) j -= nbin;
            float v = 0.0f;
            if (ok) {
                const float p = D ? D[d_ofs(k, i, ldD, dtiled)] : raw[k * nbin + j] - b;
                v = residual_sample(a, T64[i], p, i, PulseRegion{pr_on != 0, pr_start, pr_end, pr_factor});
            }
            R[k * nbin + j] = v;
        }
    }
}

// TT = numpy pairwise sum of T64[i]^2 (fit_mode 1's denominator), one wave
__global__ __launch_bounds__(64) void k_tnorm(const double *__restrict__ T64, const PwPlan *__restrict__ plan,
                                              double *__restrict__ TT)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char tsm[];
    const int lane = threadIdx.x & 63;
    const double v = wave_pairwise<double>(*plan, [&](int q) { return T64[q] * T64[q]; }, (double *)tsm, lane);
    if (lane == 0) *TT = v;
}

// ============================================================ launchers

template <int NN, bool D64>
static hipError_t launch_p2(hipStream_t st, const DiagArgs &a, size_t P)
{
    using C = P2<NN, D64>;
    const size_t fixed = (size_t)C::TW_LDS * 16;
    int gpb = C::WPP > 1 ? 1 : 8;
    while (gpb > 1 && fixed + gpb * (size_t)C::GROUP_BYTES > kLdsBudget) --gpb;
    const size_t shm = fixed + gpb * (size_t)C::GROUP_BYTES;
    const unsigned grid = cap_grid(std::min<size_t>((P + gpb - 1) / gpb, 4096), a.grid_cap);
    if (a.mode == DIAG_EXACT)
        IC_GGL((k_diag_p2<NN, DIAG_EXACT, D64>), dim3(grid), dim3(C::TPP * gpb), shm, st, a);
    else if (a.mode == DIAG_CLOSED)
        IC_GGL((k_diag_p2<NN, DIAG_CLOSED, D64>), dim3(grid), dim3(C::TPP * gpb), shm, st, a);
    else if (a.mode == DIAG_FIT)   // f32 rows either way (launch_diag passes D64 = false)
        IC_GGL((k_diag_p2<NN, DIAG_FIT, false>), dim3(grid), dim3(C::TPP * gpb), shm, st, a);
    else   // comprehensive_stats of given rows (f64 data: the fractional-dedispersion loop)
        IC_GGL((k_diag_p2<NN, DIAG_STATS, D64>), dim3(grid), dim3(C::TPP * gpb), shm, st, a);
    return hipGetLastError();
}

template <int NN>
static hipError_t launch_cl(hipStream_t st, const DiagArgs &a, size_t P)
{
    using C = CLay<NN>;
    const int gpb = C::GPB;
    const size_t shm = (size_t)C::TW_LDS * 16 + gpb * (size_t)C::GROUP_BYTES;
    const unsigned grid = cap_grid(std::min<size_t>((P + gpb - 1) / gpb, 4096), a.grid_cap);
    if (a.mode == DIAG_EXACT)
        IC_GGL((k_diag_cl<NN, DIAG_EXACT>), dim3(grid), dim3(C::L * gpb), shm, st, a);
    else if (a.mode == DIAG_STATS)
        IC_GGL((k_diag_cl<NN, DIAG_STATS>), dim3(grid), dim3(C::L * gpb), shm, st, a);
    else
        IC_GGL((k_diag_cl<NN, DIAG_CLOSED>), dim3(grid), dim3(C::L * gpb), shm, st, a);
    return hipGetLastError();
}

// k_diag_mr serves the mixed-radix lengths in every mode but DIAG_FIT
static bool uses_mr(const DiagArgs &a)
{
    return mr_supported(a.nbin) && (a.mode == DIAG_EXACT || a.mode == DIAG_CLOSED || a.mode == DIAG_STATS);
}

// leaves of numpy's pairwise sum of n values (make_plan's recursion)
static int pairwise_leaves(int n) { return n <= 128 ? 1 : pairwise_leaves(n / 2 - (n / 2) % 8) + pairwise_leaves(n - (n / 2 - (n / 2) % 8)); }

// groups per block of the one-wave form: the count (<= 8) that puts the most
// waves on a CU, whole blocks within its 160 KiB of LDS and within `cap` waves
// (what the kernel's registers allow); the larger block on a tie (fewer copies
// of the twiddle table)
static int mr_groups_per_block(const MrLayout &L, int cap)
{
    int best = 1, best_waves = 0;
    for (int g = 1; g <= 8; ++g) {
        const size_t shm = L.groups_off + g * L.per_group;
        if (shm > kLdsBudget) break;
        const int waves = (int)std::min<size_t>(kLdsBlockMax / shm, (size_t)(cap / g)) * g;
        if (waves >= best_waves) {
            best = g;
            best_waves = waves;
        }
    }
    return best;
}

static hipError_t launch_mr(hipStream_t st, const DiagArgs &a, size_t P)
{
    unsigned long long radices = 0;
    const int n = a.nbin, nst = mr_plan(n, &radices);
    // the pairwise adds run in the lanes of one wave (mr_pairwise)
    if (!nst || 2 * pairwise_leaves(n) > 64) return hipErrorInvalidValue;
    const int W = (n + 1023) / 1024;
    const bool mw = W > 1, d64 = a.data_f64 != 0;
    const MrLayout L = mr_layout(n, mw, d64, a.mode == DIAG_CLOSED);
    const int gpb = mw ? 1 : mr_groups_per_block(L, n <= 256 ? 16 : 12);   // __launch_bounds__: 4 / 3 waves per SIMD
    const size_t shm = L.groups_off + gpb * L.per_group;
    if (shm > kLdsBlockMax) return hipErrorInvalidValue;
    const dim3 grid(cap_grid(std::min<size_t>((P + gpb - 1) / gpb, 4096), a.grid_cap)), block(64 * (mw ? W : gpb));
#define IC_DIAG_MR(PPT, MW)                                                                        \
    do {                                                                                           \
        if (d64) IC_GGL((k_diag_mr<PPT, MW, true>), grid, block, shm, st, a, radices, nst);        \
        else IC_GGL((k_diag_mr<PPT, MW, false>), grid, block, shm, st, a, radices, nst);           \
        return hipGetLastError();                                                                  \
    } while (0)
    if (mw) IC_DIAG_MR(8, true);
    if (n <= 256) IC_DIAG_MR(2, false);
    IC_DIAG_MR(8, false);
#undef IC_DIAG_MR
}

// k_diag_czt serves the chirp-z lengths in every mode but DIAG_FIT
static bool uses_czt(const DiagArgs &a)
{
    return diag_czt_supported(a.nbin) && (a.mode == DIAG_EXACT || a.mode == DIAG_CLOSED || a.mode == DIAG_STATS);
}

static hipError_t launch_czt(hipStream_t st, const DiagArgs &a, size_t P)
{
    const int n = a.nbin, L = diag_czt_length(n);
    unsigned long long radices = 0;
    const int nst = mr_plan(2 * L, &radices);   // FFT_L: radix 8 while three levels remain, then 4 or 2
    // the tables are the caller's (the session's, or a one-shot scratch); the
    // pairwise adds run in two registers of the lanes of one wave (czt_pairwise)
    if (!a.czt || !nst || 2 * pairwise_leaves(n) > 128) return hipErrorInvalidValue;
    const int W = (L + 511) / 512;   // waves around one work array: 8 points per thread
    const bool mw = W > 1, d64 = a.data_f64 != 0, small = L <= 256;
    const MrLayout lay = czt_layout(n, L, mw, d64, a.mode == DIAG_CLOSED);
    const int gpb = mw ? 1 : mr_groups_per_block(lay, 12);   // __launch_bounds__: 3 waves per SIMD
    const size_t shm = lay.groups_off + gpb * lay.per_group;
    if (shm > kLdsBlockMax) return hipErrorInvalidValue;
    const dim3 grid(cap_grid(std::min<size_t>((P + gpb - 1) / gpb, 4096), a.grid_cap)), block(64 * (mw ? W : gpb));
#define IC_DIAG_CZT(PPT, MW)                                                                       \
    do {                                                                                           \
        if (d64) IC_GGL((k_diag_czt<PPT, MW, true>), grid, block, shm, st, a, radices, nst, L);    \
        else IC_GGL((k_diag_czt<PPT, MW, false>), grid, block, shm, st, a, radices, nst, L);       \
        return hipGetLastError();                                                                  \
    } while (0)
    if (mw) IC_DIAG_CZT(8, true);
    if (small) IC_DIAG_CZT(4, false);
    IC_DIAG_CZT(8, false);
#undef IC_DIAG_CZT
}

static bool uses_cl(const DiagArgs &a)
{
    if (!a.chain || a.data_f64 || !(a.nbin == 1024 || a.nbin == 2048 || a.nbin == 4096)) return false;
    // STATS: row-major residual rows (the FFT mode's rotated residual; the
    // pulse region was applied when they were formed)
    if (a.mode == DIAG_STATS) return a.D && a.ldD == a.nbin && !a.dtiled;
    return (a.mode == DIAG_EXACT || a.mode == DIAG_CLOSED) && a.T2 && a.raw && a.base && !a.pr_on;
}

// profile lists / skips: k_diag_cl, and k_diag_p2 / k_diag_mr / k_diag_czt in
// the exact mode and on given rows (the FFT mode's rotated residuals)
bool diag_list_supported(const DiagArgs &a)
{
    const int n = a.nbin;
    return uses_cl(a) ||
           ((a.mode == DIAG_EXACT || a.mode == DIAG_STATS) && (p2_supported(n) || mr_supported(n) || diag_czt_supported(n)));
}

// the generic k_diag's LDS layout as the host sizes it: nleaf/nops upper bound
// from nbin (leaves >= 64 samples except tiny n)
static DiagLayout generic_layout(int nbin)
{
    const int nleaf_ub = nbin <= 128 ? 1 : (nbin / 64 + 1);
    return diag_layout(nbin, nleaf_ub, nleaf_ub);
}

hipError_t launch_diag(hipStream_t st, const DiagArgs &a)
{
    const int nbin = a.nbin;
    const size_t P = (size_t)a.nsub * a.nchan;
    if (P == 0) return hipSuccess;
    if (a.mode == DIAG_CLOSED ? (!a.raw || !a.base || !a.TT || !a.amp || !a.info)
                              : (!a.D || a.ldD < nbin || (a.mode != DIAG_STATS && (!a.amp || !a.info)) ||
                                 (a.mode == DIAG_FIT && !a.TT)))
        return hipErrorInvalidValue;
    // the chain-layout kernel: exact / closed modes from the raw cube, f32 data, no pulse region
    if (uses_cl(a)) {
        if (nbin == 1024) return launch_cl<1024>(st, a, P);
        if (nbin == 2048) return launch_cl<2048>(st, a, P);
        if (nbin == 4096) return launch_cl<4096>(st, a, P);
    }
    if ((a.list || a.skip) && !diag_list_supported(a)) return hipErrorInvalidValue;
    if (uses_mr(a)) return launch_mr(st, a, P);
#define IC_P2(NN)                                                                                  \
    if (nbin == NN) {                                                                              \
        if (a.data_f64 && a.mode != DIAG_FIT) return launch_p2<NN, true>(st, a, P);                \
        return launch_p2<NN, false>(st, a, P);                                                     \
    }
    IC_P2_SIZES(IC_P2)
#undef IC_P2
    if (a.mode == DIAG_FIT) return hipErrorInvalidValue;   // power-of-two nbin only
    if (uses_czt(a)) return launch_czt(st, a, P);
    const DiagLayout lay = generic_layout(nbin);
    const size_t fixed = (size_t)lay.ntw * 16;
    int wpb = 4;
    while (wpb > 1 && fixed + wpb * lay.per_wave > kLdsBudget) --wpb;
    const size_t shm = fixed + wpb * lay.per_wave;
    if (shm > kLdsBlockMax) return hipErrorInvalidValue;
    const unsigned grid = cap_grid(std::min<size_t>((P + wpb - 1) / wpb, 8192), a.grid_cap);
    IC_GGL(k_diag, dim3(grid), dim3(64 * wpb), shm, st, a);
    return hipGetLastError();
}

size_t diag_lds_bytes(int nbin)
{
    if (p2_supported(nbin)) return 0;
    if (mr_supported(nbin)) {   // k_diag_mr's largest form: one group, f64 data, the closed mode's row
        const MrLayout L = mr_layout(nbin, nbin > 1024, true, true);
        return L.groups_off + L.per_group;
    }
    if (diag_czt_supported(nbin)) {   // k_diag_czt's largest form, likewise
        const int L = diag_czt_length(nbin);
        const MrLayout lay = czt_layout(nbin, L, L > 512, true, true);
        return lay.groups_off + lay.per_group;
    }
    const DiagLayout lay = generic_layout(nbin);
    return (size_t)lay.ntw * 16 + lay.per_wave;
}

hipError_t launch_tnorm(hipStream_t st, const double *T64, const PwPlan *plan, int nleaf_ub, double *TT)
{
    const size_t shm = (size_t)(nleaf_ub * 9 + nleaf_ub + 8) * 8;
    IC_GGL(k_tnorm, dim3(1), dim3(64), shm, st, T64, plan, TT);
    return hipGetLastError();
}

hipError_t launch_residual(hipStream_t st, const float *D, const float *raw, const float *base, const double *T64,
                           const double *amp, const int32_t *info, const int32_t *shift, int nsub, int nchan,
                           int nbin, int ldD, int dtiled, int pr_on, double pr_factor, int pr_start, int pr_end,
                           float *R, int grid_cap)
{
    const size_t P = (size_t)nsub * nchan;
    if (!D && (!raw || !base)) return hipErrorInvalidValue;
    const unsigned grid = cap_grid(std::min<size_t>(cdiv(P, 4), 16384), grid_cap);
    IC_GGL(k_residual, dim3(grid), dim3(256), 0, st, D, raw, base, T64, amp, info, shift, P, nchan, nbin,
                       ldD, dtiled, pr_on, pr_factor, pr_start, pr_end, R);
    return hipGetLastError();
}

}  // namespace icgpu
