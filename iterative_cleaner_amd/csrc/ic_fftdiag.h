// ic_fftdiag.h -- device-only code that the diagnostics (ic_diag.hip:
// k_diag, k_diag_p2, k_diag_cl, k_diag_mr, k_diag_czt) and the rotation (ic_rotate.hip: k_rotate,
// whose fused statistics rot_stats are k_diag_cl's, and k_rotate_mr) share:
// the f64 FFT pieces, the P2 / CLay profile-group layouts with their LDS
// address maps, the group reductions, the compile-time Stockham chain, and
// the one definition of each rule of the reference that both restate (the
// diagnostics' stores, the conjugate-pair spectrum step, the exact fit's
// residual sample; ic_codec.hip's k_residual_q takes the last from here too).
// Everything is forced inline or constexpr.
#pragma once
#include "ic_wave.h"

namespace icgpu {

// ---- mixed-radix (8/4/2, 3/5 for k_diag_mr) Stockham FFT helpers (forward, exp(-2 pi i jk/N)) ----
__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ double2 cmul(double2 a, double2 w)
{
    return make_double2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x);
}
// fused form for the power-of-two path (the FFT diagnostic is compared within
// a tolerance, never bit-for-bit: pocketfft's own rounding is not reproduced)
__device__ __forceinline__ double2 cmul_f(double2 a, double2 w)
{
    return make_double2(__builtin_fma(a.x, w.x, -(a.y * w.y)), __builtin_fma(a.x, w.y, a.y * w.x));
}
__device__ __forceinline__ double2 mul_mi(double2 a) { return make_double2(a.y, -a.x); }   // * (-i)

template <int R>
__device__ __forceinline__ void dft_small(double2 (&v)[R]);

template <>
__device__ __forceinline__ void dft_small<2>(double2 (&v)[2])
{
    const double2 a = v[0], b = v[1];
    v[0] = cadd(a, b);
    v[1] = csub(a, b);
}

template <>
__device__ __forceinline__ void dft_small<4>(double2 (&v)[4])
{
    const double2 s02 = cadd(v[0], v[2]), d02 = csub(v[0], v[2]);
    const double2 s13 = cadd(v[1], v[3]), d13 = mul_mi(csub(v[1], v[3]));
    v[0] = cadd(s02, s13);
    v[2] = csub(s02, s13);
    v[1] = cadd(d02, d13);
    v[3] = csub(d02, d13);
}

template <>
__device__ __forceinline__ void dft_small<8>(double2 (&v)[8])
{
    double2 e[4] = {v[0], v[2], v[4], v[6]};
    double2 o[4] = {v[1], v[3], v[5], v[7]};
    dft_small<4>(e);
    dft_small<4>(o);
    const double h = 0.70710678118654752440;   // sqrt(1/2)
    // o_k * exp(-2 pi i k/8), k = 0..3
    const double2 o1 = make_double2(h * (o[1].x + o[1].y), h * (o[1].y - o[1].x));
    const double2 o2 = mul_mi(o[2]);
    const double2 o3 = make_double2(h * (o[3].y - o[3].x), -h * (o[3].x + o[3].y));
    v[0] = cadd(e[0], o[0]);
    v[4] = csub(e[0], o[0]);
    v[1] = cadd(e[1], o1);
    v[5] = csub(e[1], o1);
    v[2] = cadd(e[2], o2);
    v[6] = csub(e[2], o2);
    v[3] = cadd(e[3], o3);
    v[7] = csub(e[3], o3);
}

// DFT_3 / DFT_5 in the written order of phase_rotation.py (_dft3, _dft5), f64
// constants (k_diag_mr; the rotation's packed f32 forms are rot_dft3 / rot_dft5)
template <>
__device__ __forceinline__ void dft_small<3>(double2 (&v)[3])
{
    constexpr double s3 = 0x1.bb67ae8584caap-1;   // sqrt(3)/2
    const double2 t = cadd(v[1], v[2]), d = csub(v[1], v[2]);
    const double2 m = make_double2(v[0].x - t.x * 0.5, v[0].y - t.y * 0.5);
    const double2 e = make_double2(d.x * s3, d.y * s3);
    v[0] = cadd(v[0], t);
    v[1] = make_double2(m.x + e.y, m.y - e.x);   // m - i e
    v[2] = make_double2(m.x - e.y, m.y + e.x);   // m + i e
}

template <>
__device__ __forceinline__ void dft_small<5>(double2 (&v)[5])
{
    constexpr double c1 = 0x1.3c6ef372fe950p-2;    // cos(2 pi/5)
    constexpr double c2 = -0x1.9e3779b97f4a8p-1;   // cos(4 pi/5)
    constexpr double s1 = 0x1.e6f0e134454ffp-1;    // sin(2 pi/5)
    constexpr double s2 = 0x1.2cf2304755a5ep-1;    // sin(4 pi/5)
    const double2 t1 = cadd(v[1], v[4]), t2 = cadd(v[2], v[3]), d1 = csub(v[1], v[4]), d2 = csub(v[2], v[3]);
    const double2 m1 = make_double2((v[0].x + t1.x * c1) + t2.x * c2, (v[0].y + t1.y * c1) + t2.y * c2);
    const double2 m2 = make_double2((v[0].x + t1.x * c2) + t2.x * c1, (v[0].y + t1.y * c2) + t2.y * c1);
    const double2 e1 = make_double2(d1.x * s1 + d2.x * s2, d1.y * s1 + d2.y * s2);
    const double2 e2 = make_double2(d1.x * s2 - d2.x * s1, d1.y * s2 - d2.y * s1);
    v[0] = cadd(v[0], cadd(t1, t2));
    v[1] = make_double2(m1.x + e1.y, m1.y - e1.x);
    v[2] = make_double2(m2.x + e2.y, m2.y - e2.x);
    v[3] = make_double2(m2.x - e2.y, m2.y + e2.x);
    v[4] = make_double2(m1.x - e1.y, m1.y + e1.x);
}

// layout of a k_diag_p2<N> profile group
template <int N, bool D64 = false>
struct P2 {
    static constexpr int WPP = N >= 2048 ? N / 1024 : 1;   // waves per profile
    static constexpr int TPP = 64 * WPP;                    // threads per profile
    static constexpr int M = N / 2;
    static constexpr int LEAF = N < 128 ? N : 128;
    static constexpr int NL = N / LEAF;
    static constexpr int CL = LEAF / 8;
    static constexpr int CH = 8 * NL;
    static constexpr int CPL = CH > TPP ? CH / TPP : 1;     // chains per thread
    static constexpr int ACT = CH < TPP ? CH : TPP;         // threads holding a chain
    static constexpr int WACT = ACT < 64 ? ACT : 64;        // ... per wave
    static constexpr int NPT = N / TPP;                     // samples per thread
    static constexpr int XPAD = N + 8 * NL;
    static constexpr int XBYTES = ((XPAD * (D64 ? 8 : 4) + 15) / 16) * 16;   // X: f32, or f64 (data_f64)
    static constexpr int CBYTES = M * 16;   // complex points at cidx(q)
    static constexpr int WORK_BYTES = XBYTES > CBYTES ? XBYTES : CBYTES;
    static constexpr int RED_BYTES = WPP > 1 ? 512 : 0;     // cross-wave partials
    static constexpr int GROUP_BYTES = WORK_BYTES + RED_BYTES;
    static constexpr int LG = __builtin_ctz(M);
    static constexpr int TW = 2 * M;   // twiddle entries: M post-processing + <= M stage tables
    // multi-wave groups: the table (up to 64 KiB) would cost blocks; it is read
    // through L1/L2 and the LDS holds only the groups' work arrays
    static constexpr bool TWG = WPP > 1;
    static constexpr int TW_LDS = TWG ? 0 : TW;
};

__device__ __forceinline__ int xaddr(int idx) { return idx + 8 * (idx >> 7); }

// xaddr((j0 + TPP u) mod N) for 0 <= j0 < N, in 3 VALU ops per u: the
// unwrapped address has compile-time offsets from one base (two for TPP = 64:
// xaddr(j0 + 64 u) = xaddr(j0) + 64 u + 8 ((u + bit6(j0)) >> 1)), and
// xaddr(j + N) = xaddr(j) + xaddr(N), so the wrap is an unsigned min
template <int N, int TPP>
struct XWrap {
    int a0, a1;
    __device__ __forceinline__ explicit XWrap(int j0) : a0(xaddr(j0)), a1(TPP == 64 ? xaddr(j0) + ((j0 >> 3) & 8) : 0) {}
    __device__ __forceinline__ int operator()(int u) const
    {
        constexpr int XN = N + 8 * (N >> 7);
        const int off = TPP % 128 == 0 ? u * (TPP + TPP / 16) : 64 * u + 8 * (u >> 1);
        const int au = ((TPP == 64 && (u & 1)) ? a1 : a0) + off;
        return (int)min((unsigned)au, (unsigned)(au - XN));
    }
};
// complex work array slot of point q: XOR swizzle of the low 3 bits with bits
// 3-5.  Conflict-free for every access of the kernel: the radix-8 scatters
// (ds_write_b128, 8-lane groups over 32 banks: low bits (b&7)^r or r^(b&7)) and
// the contiguous / reversed gathers (ds_read_b128, 16-lane groups over 64 banks).
__device__ __forceinline__ int cidx(int q) { return q ^ ((q >> 3) & 7); }
// Address forms with compile-time offsets (the thread index is opaque to the
// compiler, so it cannot split these itself):
//   cidx(x + 64 m) = cidx(x) + 64 m                 (the XOR reads bits 3-5 only)
//   xaddr(x + 8 q) = xaddr(x) + 8 q                 if x % 128 + 8 q < 128
//   xaddr(x + 128 m) = xaddr(x) + 136 m

// barrier of a profile group: one wave needs only ordering of its LDS ops
template <int WPP>
__device__ __forceinline__ void gsync()
{
    if constexpr (WPP > 1) __syncthreads();
    else wave_sync();
}

template <typename T, int CPL>
__device__ __forceinline__ T tree_slots(const T (&v)[CPL])
{
    if constexpr (CPL == 1) return v[0];
    else if constexpr (CPL == 2) return v[0] + v[1];
    else if constexpr (CPL == 4) return (v[0] + v[1]) + (v[2] + v[3]);
    else return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));   // CPL == 8
}

// Group-uniform reduction of a per-thread value: the wave tree over its WACT
// active lanes, then (WPP > 1) a balanced tree over the group's waves through
// `red` (WPP <= 8 slots of 8 B, one slot array per call site; both barriers keep
// the slots reusable on the next profile).  With the wave tree this is numpy's
// pairwise order: wave w holds leaves 8w .. 8w + 7, so waves pair up as the
// leaves' blocks of 8 do.
template <int WPP, int WACT, typename T, typename Op>
__device__ __forceinline__ T group_tree(T v, Op op, T *red, int wave, int lane)
{
    T w = wave_tree<WACT>(v, op);
    if constexpr (WPP == 1) {
        return w;
    } else {
        if (lane == 0) red[wave] = w;
        __syncthreads();
        T r;
        static_assert(WPP == 2 || WPP == 4 || WPP == 8, "the balanced tree is spelled out for 2, 4 and 8 waves");
        if constexpr (WPP == 2) r = op(red[0], red[1]);
        else if constexpr (WPP == 4) r = op(op(red[0], red[1]), op(red[2], red[3]));
        else r = op(op(op(red[0], red[1]), op(red[2], red[3])), op(op(red[4], red[5]), op(red[6], red[7])));
        __syncthreads();
        return r;
    }
}

// chain sums (one per slot) -> the pairwise total over the group, balanced
// over threads, then over slots
template <int N, typename T>
__device__ __forceinline__ T chain_total(const T (&cs)[P2<N>::CPL], T *red, int wave, int lane)
{
    using C = P2<N>;
    T fs[C::CPL];
#pragma unroll
    for (int sl = 0; sl < C::CPL; ++sl) fs[sl] = group_tree<C::WPP, C::WACT>(cs[sl], OpAdd(), red + 8 * sl, wave, lane);
    return tree_slots<T, C::CPL>(fs);
}

// One radix-R Stockham stage (compile-time R, NS = product of earlier radices),
// in place: every input of the stage is in registers before it writes.
// stw: this stage's twiddles w^(r k), w = exp(-2 pi i/(R NS)), as [k][r-1]
// (host-built in long double; no recurrences).  FIRST: the input is the real
// signal X (f32, padded addresses) minus mu, read as complex pairs.
// DER: only each butterfly's base twiddle w = stw[k][0] is read; w^2 .. w^(R-1)
// come from repeated complex products (a few ulp off the table's correctly
// rounded values: the FFT diagnostic is compared within 1e-9, and this trades
// R - 2 LDS reads for 4 (R - 2) VALU ops per butterfly)
template <int R, int NS, bool FIRST, int M, int TPP, typename XT, bool DER = false>
__device__ __forceinline__ void p2_stage(double2 *C, const XT *X, double mu, const double2 *stw, int t)
{
    constexpr int NB = M / R;
    constexpr int BPL = (NB + TPP - 1) / TPP;
    double2 v[BPL][R];
#pragma unroll
    for (int u = 0; u < BPL; ++u) {
        const int b = t + TPP * u;
        if (NB % TPP == 0 || b < NB) {
            // 2 q = 2 b + 2 r NB: a multiple of 128 apart when NB % 64 == 0
            const XT *xb = X + xaddr(2 * b);
            const double2 *cb = C + cidx(b);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int q = b + r * NB;
                if (FIRST) {
                    const XT *xq = NB % 64 == 0 ? xb + r * (2 * NB + NB / 8) : X + xaddr(2 * q);
                    if constexpr (sizeof(XT) == 8) {
                        const double2 xv = *(const double2 *)xq;
                        v[u][r] = make_double2(xv.x - mu, xv.y - mu);
                    } else {
                        const float2 xv = *(const float2 *)xq;
                        v[u][r] = make_double2((double)xv.x - mu, (double)xv.y - mu);
                    }
                } else {
                    v[u][r] = NB % 64 == 0 ? cb[r * NB] : C[cidx(q)];
                }
            }
        }
    }
    gsync<TPP / 64>();
#pragma unroll
    for (int u = 0; u < BPL; ++u) {
        const int b = t + TPP * u;
        if (NB % TPP == 0 || b < NB) {
            const int k = b & (NS - 1);
            if (NS > 1) {
                const double2 *tk = stw + k * (R - 1);
                if constexpr (DER) {
                    const double2 w1 = tk[0];
                    double2 wr = w1;
#pragma unroll
                    for (int r = 1; r < R; ++r) {
                        if (r > 1) wr = cmul_f(wr, w1);
                        v[u][r] = cmul_f(v[u][r], wr);
                    }
                } else {
#pragma unroll
                    for (int r = 1; r < R; ++r) v[u][r] = cmul_f(v[u][r], tk[r - 1]);
                }
            }
            dft_small<R>(v[u]);
            const int idx = (b - k) * R + k;
            if constexpr (NS % 64 == 0) {
                double2 *cw = C + cidx(idx);
#pragma unroll
                for (int r = 0; r < R; ++r) cw[r * NS] = v[u][r];
            } else if constexpr (NS == 8 && R == 8) {
                // idx = 64 m + k (k < 8): cidx(idx + 8 r) = 64 m + 8 r + (k ^ r)
#pragma unroll
                for (int r = 0; r < R; ++r) C[(idx ^ r) + 8 * r] = v[u][r];
            } else if constexpr (NS == 1 && R == 8) {
                // idx = 8 b: cidx(idx + r) = idx + (r ^ (b & 7)) = (idx + (b & 7)) ^ r
                const int A = idx + (b & 7);
#pragma unroll
                for (int r = 0; r < R; ++r) C[A ^ r] = v[u][r];
            } else {
#pragma unroll
                for (int r = 0; r < R; ++r) C[cidx(idx + r * NS)] = v[u][r];
            }
        }
    }
    gsync<TPP / 64>();
}

// the whole N/2-point FFT as a compile-time chain of stages (radix 8 while >= 3
// levels remain, then 4 or 2); OFF = offset of the next stage table in tw
template <int M, int TPP, int LG, int DONE, int NS, int OFF, typename XT, bool DER = false>
__device__ __forceinline__ void p2_fft(double2 *C, const XT *X, double mu, const double2 *tw, int t)
{
    if constexpr (DONE < LG) {
        constexpr int REM = LG - DONE;
        constexpr int R = REM >= 3 ? 8 : (REM == 2 ? 4 : 2);
        constexpr int LR = R == 8 ? 3 : (R == 4 ? 2 : 1);
        p2_stage<R, NS, DONE == 0, M, TPP, XT, DER>(C, X, mu, tw + OFF, t);
        p2_fft<M, TPP, LG, DONE + LR, NS * R, (NS > 1 ? OFF + NS * (R - 1) : OFF), XT, DER>(C, X, mu, tw, t);
    }
}

// entries of the k_diag_p2 / k_diag_cl twiddle table: M post-processing + the stage tables
constexpr int p2_tw_entries(int N)
{
    const int M = N / 2;
    int lg = 0;
    while ((1 << lg) < M) ++lg;
    int n = M;
    for (int done = 0, ns = 1; done < lg;) {
        const int rem = lg - done, R = rem >= 3 ? 8 : (rem == 2 ? 4 : 2);
        if (ns > 1) n += ns * (R - 1);
        ns *= R;
        done += R == 8 ? 3 : (R == 4 ? 2 : 1);
    }
    return n;
}

// The one-wave (N = 1024) form: twiddles from an LDS copy (through L1/L2:
// 2.59 ms per pass against 2.00), 4 waves per SIMD, 8 profile groups per
// block.  Closed mode takes the dedispersed-order samples of the row by a
// second global read, not from an LDS copy of the registers' dispersed-order
// ones: the read misses L2 often enough to add 15 % to the pass's HBM traffic,
// but the copy costs LDS bandwidth, which binds at N = 1024 (C2 fast mode
// 2.48 -> 2.62 ms per pass with the copy).  Stage and spectrum twiddles are
// derived from one base twiddle per butterfly / lane (p2_stage DER; tw[t + L j]
// = tw[t] exp(-2 pi i j / 16)) instead of read one each for the multi-wave
// groups (N >= 2048), whose table is read through L1/L2 (C5 k_diag 2.81 ->
// 2.68 ms per launch); at N = 1024, whose table is in LDS, that measured no
// faster (2.005 -> 2.03).
template <int N>
struct CLay {
    static constexpr int L = N / 16;     // threads per profile = chains of 16 samples
    static constexpr int WPP = L / 64;   // waves per profile
    static constexpr int M = N / 2;
    static constexpr int LG = __builtin_ctz(M);
    static constexpr int GPB = WPP > 1 ? 1 : 8;   // profile groups per block
    static constexpr bool TWG = WPP > 1;   // multi-wave groups read the table through L1/L2
    static constexpr int TW_LDS = TWG ? 0 : p2_tw_entries(N);
    static constexpr int CBYTES = M * 16;
    static constexpr int RED_BYTES = WPP > 1 ? 512 : 0;
    static constexpr int GROUP_BYTES = CBYTES + RED_BYTES;
    static_assert(N >= 1024 && L % 64 == 0, "chain layout: one chain of 16 samples per thread");
};

__device__ __forceinline__ float ufirst(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ __forceinline__ int ufirst(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ double ufirst(double v)
{
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)),
                            __builtin_amdgcn_readfirstlane(__double2loint(v)));
}

// ---- rules of the reference, each written once ------------------------------

// scipy leastsq status 1..4: a solution was found; otherwise the residual is 0
// (ic.py:284-286)
__device__ __forceinline__ bool fit_ok(int info) { return info >= 1 && info <= 4; }

// sample i of the exact fit's residual (ic.py:279-288, f32 store :272):
// f32(amp T_i - p_i), scaled by pr_factor on the pulse region [pr_start, pr_end)
// of `a` (DiagArgs, RotateArgs or PulseRegion), whose fields are read only where needed
template <typename Args>
__device__ __forceinline__ float residual_sample(double amp, double Ti, float pi, int i, const Args &a)
{
    const double u = amp * Ti;
    double e = u - (double)pi;
    if (a.pr_on && i >= a.pr_start && i < a.pr_end) e = e * a.pr_factor;
    return (float)e;
}
struct PulseRegion {
    bool pr_on;
    int pr_start, pr_end;
    double pr_factor;
};
// ... without a pulse region
__device__ __forceinline__ float residual_sample(double amp, double Ti, float pi)
{
    const double u = amp * Ti;
    return (float)(u - (double)pi);
}

// ptp of a masked profile (w0 == 0): numpy.ma's fill value of the data dtype
__device__ __forceinline__ double ptp_fill(bool f64) { return f64 ? 1e20 : (double)1e20f; }

// the four diagnostics of profile k (ic.py:206-217, numpy.ma conventions): a
// masked profile has mean 0, and a non-finite mean is masked in the std -> 0
template <typename Args, typename Idx>
__device__ __forceinline__ void diag_store(const Args &a, Idx k, bool valid, double mean, double sd, double ptp,
                                           double fftv)
{
    a.std_o[k] = valid && isfinite(mean) ? sd : 0.0;
    a.mean_o[k] = valid ? mean : 0.0;
    a.ptp_o[k] = ptp;
    a.fft_o[k] = fftv;
}

// Conjugate-pair step of the real spectrum from the half-length FFT Z (2 X_k;
// the derivation is at k_diag_p2's call): |2 X_k|^2 and |2 X_(M-k)|^2 from
// Z_k, Z_(M-k) and w^k, one product t = w^k O_k serving both bins.
__device__ __forceinline__ void spec_pair_mags(const double2 zk, const double2 zm, const double2 wv, double &a2,
                                               double &b2)
{
    const double er = zk.x + zm.x, ei = zk.y - zm.y;
    const double orr = zk.y + zm.y, oi = zm.x - zk.x;
    const double tr = __builtin_fma(orr, wv.x, -(oi * wv.y));
    const double ti = __builtin_fma(orr, wv.y, oi * wv.x);
    const double re = er + tr, im = ei + ti;
    const double rm = er - tr, imm = ti - ei;
    a2 = __builtin_fma(re, re, im * im);
    b2 = __builtin_fma(rm, rm, imm * imm);
}
__device__ __forceinline__ void spec_pair(const double2 zk, const double2 zm, const double2 wv, double &best2)
{
    double a2, b2;
    spec_pair_mags(zk, zm, wv, a2, b2);
    best2 = fmax(best2, fmax(a2, b2));
}
// ... that also sums the magnitudes: they are >= 0 or NaN, so the sum is NaN iff one is
__device__ __forceinline__ void spec_pair_nan(const double2 zk, const double2 zm, const double2 wv, double &best2,
                                              double &nsum)
{
    double a2, b2;
    spec_pair_mags(zk, zm, wv, a2, b2);
    nsum = nsum + a2;
    nsum = nsum + b2;
    best2 = fmax(best2, fmax(a2, b2));
}
// the self-paired bin k = M/2: spec_pair(z, z, w) with the exact zeros ei = oi
// = 0 of a finite z folded in
__device__ __forceinline__ void spec_self_pair(const double2 z, const double2 wv, double &best2)
{
    const double er = z.x + z.x, orr = z.y + z.y;
    const double tr = orr * wv.x, ti = orr * wv.y;
    const double re = er + tr, rm = er - tr, q2 = ti * ti;
    best2 = fmax(best2, fmax(__builtin_fma(re, re, q2), __builtin_fma(rm, rm, q2)));
}

}  // namespace icgpu
