// ic_rotate.hip -- fractional dedispersion: the FFT phase rotation at
// power-of-two (k_rotate, with the fused statistics rot_stats) and mixed-radix
// (k_rotate_mr) profile lengths, the opt-in chirp-z rotation of any other
// length (k_rotate_czt), the identity rotation, the channel phasor
// table they read (k_phasor_table), and their launchers.
#include <algorithm>
#include <float.h>
#include <math.h>

#include "ic_fftdiag.h"

namespace icgpu {

// ---------------------------------------------------------------------------
// Fractional dedispersion: psrchive's FFT phase rotation in the stand-in's
// written order (phase_rotation.py; oracle orc_rotate), in IEEE f32 as
// psrchive's.  A profile per wave (N <= 1024: four to a block, sharing the
// twiddle tables staged in LDS) or per block (N >= 2048); grid-stride over
// channel-major items so that the profiles in flight share a channel's phasor
// row in L2; the N/2 complex points live in LDS between the passes.
//   1. z[j] = (f32(x[2j] - b), f32(x[2j+1] - b))
//   2. Z = FFT_{N/2}(z): Stockham stages of radix 8 (then 4 or 2), one LDS
//      round trip per stage
//   3. pairs (k, N/2 - k): real spectrum, x phasor, inverse half-spectrum
//      (conj) in one linear map (rot_pair)
//   4. r = FFT_{N/2}(that); out = r.re / M, -r.im / M
// A complex point is an f32 pair (rc2) and every complex operation one packed
// VOP3P instruction (v_pk_add_f32 / v_pk_mul_f32 with op_sel / neg modifiers
// for the swaps and the one-sided signs), each half an IEEE f32 operation of
// the definition: the same bits as the oracle's scalar f32 code
// (-ffp-contract=off), at half the f64 instruction count.
typedef float rc2 __attribute__((ext_vector_type(2)));

#ifndef IC_ROT_TW_LDS_MAX
#define IC_ROT_TW_LDS_MAX 4096   // the longest nbin whose rotation stages its twiddle table in LDS
#endif

template <int N>
struct RotCfg {
    static constexpr int M = N / 2, H = M / 2;
    static constexpr int LG = __builtin_ctz(M);   // log2 M
    static constexpr int TB = M / 8 < 64 ? 64 : (M / 8 > 256 ? 256 : M / 8);
    // one-wave profiles run four to a block, which stages the twiddle table in
    // LDS once for all four; the one-block profiles of N = 2048 / 4096 stage it too,
    // once per block of the grid-stride loop (16 profiles per block at C5:
    // 62.7-63.1 -> 58.0-58.2 ms per C5 clean in the FFT mode, against f64
    // entries through L1/L2 rounded at each use)
    static constexpr int WPB = TB == 64 ? 4 : 1;
    // N = 8192: the f32 table (64 KiB) beside the 36 KiB of points would leave
    // one block (one wave per SIMD) per CU; its entries are read as f64 through
    // L1/L2 and rounded at the use (TwGlobal): the LDS then allows 4 blocks per
    // CU and the 251-256 VGPRs two (2 waves per SIMD).  Measured on a 64 x 512
    // x 8192 archive, alternating: 33.0-33.2 ms per clean with per-profile
    // delays and 33.9-34.1 per channel, against 38.5-38.6 and 40.3-40.5 staged
    // (-DIC_ROT_TW_LDS_MAX=8192 builds the staged form, tools/build_variant.sh)
    static constexpr bool TW_LDS = N <= IC_ROT_TW_LDS_MAX;
};

// LDS slot of complex point i: one pad slot after every 8 points.  With 8-byte
// points ds_write_b64 banks 16 contiguous lanes on (slot mod 16) and ds_read_b64
// 32 lanes on (slot mod 32) (MI355X_MICROARCH.md): the stage stores (lane t ->
// points 8 t + q, and 64 (t / 8) + t % 8 + 8 q) are conflict-free, the
// contiguous reads (t + 64 q) 2-way on 3 of 32 banks.  A XOR swizzle cannot
// make the stores conflict-free without per-q address arithmetic on the reads
// (bits 6+ of the slot change with q).  All offsets are per-lane bases plus
// immediates: rsl(i + 8 c) = rsl(i) + 9 c.
__device__ __forceinline__ constexpr int rsl(int i) { return i + (i >> 3); }
template <int M> constexpr int rot_slots() { return M + M / 8; }

// packed complex arithmetic (each half one IEEE f32 operation)
__device__ __forceinline__ rc2 pk_nlo(rc2 a, rc2 b)   // (a.x - b.x, a.y + b.y)
{
    rc2 r;
    asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ rc2 pk_nhi(rc2 a, rc2 b)   // (a.x + b.x, a.y - b.y)
{
    rc2 r;
    asm("v_pk_add_f32 %0, %1, %2 neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ rc2 pk_mi(rc2 a, rc2 b)   // a + (-i) b = (a.x + b.y, a.y - b.x)
{
    rc2 r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ rc2 pk_pi(rc2 a, rc2 b)   // a + i b = (a.x - b.y, a.y + b.x)
{
    rc2 r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ rc2 pk_c7(rc2 c)   // (c.y - c.x, c.x + c.y)
{
    rc2 r;
    asm("v_pk_add_f32 %0, %1, %1 op_sel:[1,0] op_sel_hi:[0,1] neg_lo:[0,1]" : "=v"(r) : "v"(c));
    return r;
}
__device__ __forceinline__ rc2 pk_cross(rc2 a, rc2 b)   // (a.y + b.y, a.x - b.x)
{
    rc2 r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[0,0] neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ rc2 pk_addc(rc2 a, rc2 b)   // (a.x + b.x, (-a.y) + (-b.y))
{
    rc2 r;
    asm("v_pk_add_f32 %0, %1, %2 neg_hi:[1,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ rc2 rc2_of(double2 d) { return (rc2){(float)d.x, (float)d.y}; }

// 8-byte loads of the phasor table / 16-byte loads of the f64 twiddle table
// through a buffer descriptor: a 32-bit per-lane offset plus an immediate,
// instead of a 64-bit address register per table entry kept live across the
// profile loop
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rot_rsrc(const void *p, unsigned bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ double2 rot_ld(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff)
{
    return __builtin_bit_cast(double2, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}
__device__ __forceinline__ rc2 rot_ld2(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff)
{
    return __builtin_bit_cast(rc2, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0));
}

// Twiddle sources: k_diag_p2's table (p2_twiddles: M plain entries tw[i] =
// exp(-2 pi i i / N), then for every Stockham stage after the first, of radix
// R and span ns, the entries w^(q k), w = exp(-2 pi i / (R ns)), as [k][q - 1]
// at M + ns - 8: the spans are 8, 64, 512, so the earlier tables fill ns - 8
// slots), the same long-double values rounded to f64; the rotation uses them
// rounded to f32.  Staged in LDS as f32 (TwLds32; with the statistics, whose
// FFT needs the f64 table in LDS too, the f32 stage tables only: TwLdsSt), or
// read as f64 through L1/L2 and rounded at the use (TwGlobal, one-block
// profiles N = 8192, whose f32 table would take 64 KiB).
template <int N>
struct TwGlobal {
    static constexpr bool ASM_ROWS = false;
    __amdgpu_buffer_rsrc_t r;
    template <int NS, int R>
    __device__ __forceinline__ rc2 stage(unsigned k, int q) const
    {
        return rc2_of(rot_ld(r, 16u * (unsigned)(k * (R - 1)), 16u * (unsigned)(N / 2 + NS - 8 + q - 1)));
    }
    __device__ __forceinline__ rc2 post(unsigned i) const { return rc2_of(rot_ld(r, 16u * i, 0)); }
};
template <int N>
struct TwLds32 {
    static constexpr bool ASM_ROWS = true;   // rot_pass reads the stage rows with ds_read_b64
    const rc2 *t;
    template <int NS, int R>
    __device__ __forceinline__ rc2 stage(unsigned k, int q) const
    {
        return t[N / 2 + NS - 8 + q - 1 + k * (R - 1)];
    }
    // LDS byte address of entry [k][0] of the stage table of span NS
    template <int NS, int R>
    __device__ __forceinline__ uint32_t row(unsigned k) const
    {
        return lds_u32(t + (N / 2 + NS - 8 + k * (R - 1)));
    }
    __device__ __forceinline__ rc2 post(unsigned i) const { return t[i]; }
};
// with the statistics: the f32 stage tables alone (s: the entries from M on)
// beside the f64 table the statistics FFT reads, whose plain part serves the
// post step (rounded at the use); 53 KB of LDS per four-wave block, three
// blocks per CU
template <int N>
struct TwLdsSt {
    static constexpr bool ASM_ROWS = true;
    const rc2 *s;
    const double2 *t;
    template <int NS, int R>
    __device__ __forceinline__ rc2 stage(unsigned k, int q) const
    {
        return s[NS - 8 + q - 1 + k * (R - 1)];
    }
    template <int NS, int R>
    __device__ __forceinline__ uint32_t row(unsigned k) const
    {
        return lds_u32(s + (NS - 8 + k * (R - 1)));
    }
    __device__ __forceinline__ rc2 post(unsigned i) const { return rc2_of(t[i]); }
};

// the rotation's complex product (a.r w.r - a.i w.i, a.r w.i + a.i w.r):
// (a.r w.r, a.r w.i) and (a.i w.i, a.i w.r), then one add with the low half
// subtracted
__device__ __forceinline__ rc2 rot_cmul(rc2 a, rc2 w)
{
    return pk_nlo(a.xx * w, a.yy * w.yx);
}
// DFT of 4 / 8 points in place, natural output order, in the written order of
// phase_rotation.py (_dft4, _dft8) and the oracle (dft4, dft8): c3 = -i d is
// folded into y1 = c1 + c3 = pk_mi(c1, d) and y3 = c1 - c3 = pk_pi(c1, d)
// (x + (-y) is x - y bit for bit), and c6 = -i c6 into the odd DFT_4's first
// level the same way
__device__ __forceinline__ void rot_dft4(rc2 *b)
{
    const rc2 c0 = b[0] + b[2], c1 = b[0] - b[2], c2 = b[1] + b[3], d = b[1] - b[3];
    b[0] = c0 + c2;
    b[1] = pk_mi(c1, d);
    b[2] = c0 - c2;
    b[3] = pk_pi(c1, d);
}
__device__ __forceinline__ void rot_dft8(rc2 *b)
{
    constexpr float s = (float)0x1.6a09e667f3bcdp-1;   // f32(f64(sqrt(2)/2))
    rc2 c[8];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        c[q] = b[q] + b[q + 4];
        c[q + 4] = b[q] - b[q + 4];
    }
    c[5] = pk_mi(c[5], c[5]) * (rc2){s, s};    // ((c.r + c.i) s, (c.i - c.r) s)
    c[7] = pk_c7(c[7]) * (rc2){s, -s};         // ((c.i - c.r) s, -((c.r + c.i) s))
    rot_dft4(c);
    // odd DFT_4 of (c4, c5, -i c6, c7)
    const rc2 e0 = pk_mi(c[4], c[6]), e1 = pk_pi(c[4], c[6]), e2 = c[5] + c[7], d = c[5] - c[7];
    b[0] = c[0];
    b[2] = c[1];
    b[4] = c[2];
    b[6] = c[3];
    b[1] = e0 + e2;
    b[3] = pk_mi(e1, d);
    b[5] = e0 - e2;
    b[7] = pk_pi(e1, d);
}

// One Stockham stage of radix Q = 2^R and span ns = 2^LGS (phase_rotation.py
// _stockham): group ja < G = M/Q holds the points v[ja + q G]; from the second
// stage on they are multiplied by the stage's twiddles w^(q k), k = ja mod ns,
// then transformed by DFT_Q, and y_p lands at v[(ja - k) Q + k + p ns].  One LDS
// round trip per stage (8 points per lane at N = 1024, three stages per FFT).
// IN_REG: the pass's input is z (one group per thread, G == TB) instead of
// LDS; OUT_REG: its output stays in z.  The last pass's group ja holds points
// ja + q G, the distribution the first pass reads, so a profile can enter and
// leave the FFT in registers (k_rotate's direct layout).
template <int N, int R, int LGS, bool IN_REG = false, bool OUT_REG = false, typename TW>
__device__ __forceinline__ void rot_pass(rc2 *v, const TW &tw, int t, rc2 *z = nullptr)
{
    using C = RotCfg<N>;
    constexpr int M = C::M, TB = C::TB, G = M >> R, Q = 1 << R;
    constexpr int GPT = (G + TB - 1) / TB;
    constexpr int ns = 1 << LGS;
    static_assert(!(IN_REG || OUT_REG) || G == TB, "register passes hold one group per thread");
    static_assert(ns == 1 || ns >= 8, "stage spans are 1, 8, 64, 512");
    rc2 u[GPT][Q];
    // the stage's twiddles first (their latency overlaps the LDS reads and the barrier)
    rc2 w[GPT][Q - 1];
    // one-group-per-lane passes read their points (and the f32 twiddle rows)
    // as separate ds_read_b64 in asm: the compiler pairs adjacent 8-byte LDS
    // loads into ds_read2_b64, which serves 16-lane groups on 32 banks at 4x
    // the LDS cycles per byte (MI355X_MICROARCH.md); one lgkmcnt wait ties
    // the values
    constexpr bool ASM = GPT == 1 && G == TB && G % 8 == 0 && !IN_REG;
    if constexpr (ASM) {
        const int ja = t, k = ja & (ns - 1);
        if constexpr (ns > 1 && TW::ASM_ROWS) {
            const uint32_t wa = tw.template row<ns, Q>((unsigned)k);
#pragma unroll
            for (int q = 1; q < Q; ++q)
                asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(w[0][q - 1]) : "v"(wa), "i"(8 * (q - 1)));
        } else if constexpr (ns > 1) {
#pragma unroll
            for (int q = 1; q < Q; ++q) w[0][q - 1] = tw.template stage<ns, Q>((unsigned)k, q);
        }
        const uint32_t va = lds_u32(v + rsl(ja));   // rsl(ja + q G) = rsl(ja) + q (G + G/8)
#pragma unroll
        for (int q = 0; q < Q; ++q)
            asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(u[0][q]) : "v"(va), "i"(8 * q * (G + G / 8)));
        if constexpr (Q == 8) {
            asm volatile("s_waitcnt lgkmcnt(0)"
                         : "+v"(u[0][0]), "+v"(u[0][1]), "+v"(u[0][2]), "+v"(u[0][3]), "+v"(u[0][4]), "+v"(u[0][5]),
                           "+v"(u[0][6]), "+v"(u[0][7]));
        } else {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int q = 0; q < Q; ++q) asm volatile("" : "+v"(u[0][q]));
        }
        if constexpr (ns > 1 && TW::ASM_ROWS) {
#pragma unroll
            for (int q = 0; q < Q - 1; ++q) asm volatile("" : "+v"(w[0][q]));
        }
    }
#pragma unroll
    for (int gi = 0; gi < GPT && !ASM; ++gi) {
        const int ja = t + TB * gi;
        const int k = ja & (ns - 1);
        if (G % TB == 0 || ja < G) {
            if constexpr (ns > 1) {
#pragma unroll
                for (int q = 1; q < Q; ++q) w[gi][q - 1] = tw.template stage<ns, Q>((unsigned)k, q);
            }
            if constexpr (IN_REG) {
#pragma unroll
                for (int q = 0; q < Q; ++q) u[gi][q] = z[q];
            } else if constexpr (G % 8 == 0) {
                const rc2 *vj = v + rsl(ja);    // rsl(ja + q G) = rsl(ja) + q (G + G/8)
#pragma unroll
                for (int q = 0; q < Q; ++q) u[gi][q] = vj[q * (G + G / 8)];
            } else {
#pragma unroll
                for (int q = 0; q < Q; ++q) u[gi][q] = v[rsl(ja + q * G)];
            }
        }
    }
    gsync<C::TB / 64>();
#pragma unroll
    for (int gi = 0; gi < GPT; ++gi) {
        const int ja = t + TB * gi;
        if (G % TB == 0 || ja < G) {
            const int k = ja & (ns - 1);
            if constexpr (ns > 1) {
#pragma unroll
                for (int q = 1; q < Q; ++q) u[gi][q] = rot_cmul(u[gi][q], w[gi][q - 1]);
            }
            if constexpr (Q == 8) {
                rot_dft8(u[gi]);
            } else if constexpr (Q == 4) {
                rot_dft4(u[gi]);
            } else {
                const rc2 a = u[gi][0], b = u[gi][1];
                u[gi][0] = a + b;
                u[gi][1] = a - b;
            }
            const int base = ((ja >> LGS) << (LGS + R)) + k;
            if constexpr (OUT_REG) {
                static_assert(ns * Q == M, "only the last pass keeps its output");
#pragma unroll
                for (int q = 0; q < Q; ++q) z[q] = u[gi][q];
            } else if constexpr (ns % 8 == 0) {
                rc2 *vb = v + rsl(base);   // rsl(base + q ns) = rsl(base) + q (ns + ns/8)
#pragma unroll
                for (int q = 0; q < Q; ++q) vb[q * (ns + ns / 8)] = u[gi][q];
            } else {
                // ns = 1: base = Q ja, a multiple of 8 for Q = 8 (rsl(base + q) = rsl(base) + q)
                rc2 *vb = v + rsl(base);
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    if constexpr (Q == 8) vb[q] = u[gi][q];
                    else v[rsl(base + q)] = u[gi][q];
                }
            }
        }
    }
    gsync<C::TB / 64>();
}

// the full N/2-point FFT: passes of 3 stages (the last one shorter); IN_REG /
// OUT_REG: the first pass reads z / the last pass leaves its output in z
template <int N, int LG0 = 0, bool IN_REG = false, bool OUT_REG = false, typename TW>
__device__ __forceinline__ void rot_fft(rc2 *v, const TW &tw, int t, rc2 *z = nullptr)
{
    constexpr int LG = RotCfg<N>::LG;
    if constexpr (LG0 < LG) {
        constexpr int R = LG - LG0 >= 3 ? 3 : LG - LG0;
        constexpr bool LAST = LG0 + R >= LG;
        rot_pass<N, R, LG0, IN_REG && LG0 == 0, OUT_REG && LAST>(v, tw, t, z);
        rot_fft<N, LG0 + R, false, OUT_REG>(v, tw, t, z);
    }
}

// The inverse's half-length inputs Z'_k, Z'_q (q = M - k) from the transform's
// Z_k, Z_q in one linear map (phase_rotation.py _pair, oracle rot_pair): the
// real spectrum X_k = E_k + w O_k, the phasors and the inverse's packing
// composed, Z'_k = A_k Z_k + B_k conj(Z_q), Z'_q = A_q Z_q - conj(B_k) conj(Z_k),
// with w = exp(-2 pi i k / N) = (c, sn) and the signed phasors pk, pq.  Returns
// conj(Z'_k), conj(Z'_q) (what the inverse stores; the imaginary part as (-a) +
// (-b) of the two terms', the definition's order).  Packed: (h1, h2) = ((1 +
// sn), (1 - sn)) * 0.5; A_k = (h1 pk.r + h2 pq.r, h1 pk.i - h2 pq.i), A_q
// likewise; B_k = (pk.i + pq.i, pk.r - pq.r) * (-c/2, c/2) (-(x y) = (-x) y);
// A Z is rot_cmul; B_k conj(Z_q) = (b.r zq.r + b.i zq.i, b.i zq.r - b.r zq.i);
// -conj(B_k) conj(Z_k) = (b.i zk.i - b.r zk.r, b.i zk.r + b.r zk.i).
__device__ __forceinline__ void rot_pair(rc2 zk, rc2 zq, rc2 w, rc2 pk, rc2 pq, rc2 &ok, rc2 &oq)
{
    rc2 hh;
    const rc2 one = {1.0f, 1.0f};
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[0,1] neg_hi:[0,1]" : "=v"(hh) : "v"(one), "v"(w));
    hh = hh * (rc2){0.5f, 0.5f};
    const rc2 hcv = w.xx * (rc2){-0.5f, 0.5f};
    const rc2 ak = pk_nhi(hh.xx * pk, hh.yy * pq);
    const rc2 aq = pk_nhi(hh.xx * pq, hh.yy * pk);
    const rc2 b = pk_cross(pk, pq) * hcv;
    ok = pk_addc(rot_cmul(ak, zk), pk_nhi(b * zq.xx, b.yx * zq.yy));
    oq = pk_addc(rot_cmul(aq, zq), pk_nlo(b.yy * zk.yx, b.xx * zk));
}

// DC / Nyquist step of the post pass: X_0 = Z_0.r + Z_0.i and X_M = Z_0.r -
// Z_0.i times the real parts p0, pm of their phasors, back to the packed Z_0
__device__ __forceinline__ rc2 rot_dc_nyquist(rc2 z0, float p0, float pm)
{
    const float X0 = z0.x + z0.y, XM = z0.x - z0.y;
    const float Y0 = X0 * p0, YM = XM * pm;
    return (rc2){(Y0 + YM) * 0.5f, -((Y0 - YM) * 0.5f)};
}

// comprehensive_stats (ic.py:206-212) of the rotated residual row held by one
// wave in the direct layout: z[q] = point j = t + TB q, i.e. R[2j] = f32(z.re /
// M), R[2j + 1] = f32(-z.im / M) (k_rotate's store), X = f32(R w) (apply_weights,
// ic.py:111-117, 296).  Every value is k_diag_cl<N, DIAG_STATS>'s, bit for bit:
// - mean / var / ptp: X goes through the wave's LDS slots once (the padded
//   xaddr image) and each lane reads its pairwise chain (leaf t/8, accumulator
//   t%8: samples 128(t/8) + t%8 + 8q); the trees are chain_total's;
// - fftmax: k_diag_cl's first radix-8 stage reads the points t + 64 r of d =
//   f64(X) - mean, which is exactly the direct layout this lane holds, so the
//   rFFT starts from registers; the later stages are p2_fft's with its f64
//   table (tw_p2, which k_rotate stages in LDS: tw64), the spectrum's post
//   twiddles tw[k < M] from the same table's plain part.  v: the wave's LDS
//   work array (M f64 complex points).
template <int N>
__device__ __forceinline__ void rot_stats(const RotateArgs &a, size_t p, double2 *v, const double2 *tw64, int t,
                                          rc2 (&z)[8], float inv, float w)
{
    constexpr int M = RotCfg<N>::M, H = M / 2, TB = RotCfg<N>::TB, L = TB;
    static_assert(N == 1024 && TB == 64 && CLay<N>::L == 64, "one wave per profile, 16 samples per lane");
    static_assert(RotCfg<N>::TW_LDS, "the statistics FFT reads k_diag's table from the rotation's LDS copy (tw64)");
    float xr[16];   // sample 2(t + 64 q) + e at xr[2q + e]
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        xr[2 * q] = z[q].x * inv;
        xr[2 * q + 1] = (-z[q].y) * inv;
    }
    if (w != 1.0f) {   // fractional weights (w * 1 = w exactly: skipped)
#pragma unroll
        for (int e = 0; e < 16; ++e) xr[e] = xr[e] * w;
    }
    const bool valid = w != 0.0f;
    double mean = 0.0, sd = 0.0, fftv = 0.0, ptp = ptp_fill(false);
    if (valid) {
        // the row into LDS (the last pass's reads of v are done: rot_pass ends
        // with gsync), float pairs at xaddr(2j) = 2t + 136 q
        float *xs = (float *)v;
#pragma unroll
        for (int q = 0; q < 8; ++q) *(float2 *)(xs + 2 * t + 136 * q) = make_float2(xr[2 * q], xr[2 * q + 1]);
        wave_sync();
        float X[16];
        {
            const float *xc = xs + 136 * (t >> 3) + (t & 7);
#pragma unroll
            for (int q = 0; q < 16; ++q) X[q] = xc[8 * q];
        }
        // (k_diag_cl's chain arithmetic, ic_diag.hip, restated: edit both)
        float s = X[0];
#pragma unroll
        for (int q = 1; q < 16; ++q) s = s + X[q];
        float fs[1] = {s};
        const float s32 = 0.0f + chain_total<N, float>(fs, (float *)nullptr, 0, t);
        mean = (double)s32 / (double)N;
        double r = 0.0;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const double d = (double)X[q] - mean;
            const double sq = d * d;
            r = q == 0 ? sq : r + sq;
        }
        double rs[1] = {r};
        const double ss = 0.0 + chain_total<N, double>(rs, (double *)nullptr, 0, t);
        sd = sqrt(ss / (double)N);
        float mx = -INFINITY, mn = INFINITY;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            mx = OpMaxF()(mx, X[q]);
            mn = OpMinF()(mn, X[q]);
        }
        mx = group_tree<1, 64>(mx, OpMaxF(), (float *)nullptr, 0, t);
        mn = group_tree<1, 64>(mn, OpMinF(), (float *)nullptr, 0, t);
        int nan = 0;
        if (isnan(s32)) {
#pragma unroll
            for (int q = 0; q < 16; ++q) nan |= isnan(X[q]);
            nan = group_tree<1, 64>(nan, OpOr(), (int *)nullptr, 0, t);
        }
        ptp = nan ? (double)NAN : (double)(float)(mx - mn);
        // rfft of d (ic.py:210-212): stage 1 (radix 8, no twiddles) on the
        // lane's points t + 64 r, then k_diag_p2's stages in the complex work
        // array Cb = v (cidx slots, M entries: inside the rotation's padded
        // array).  The chain reads above precede the stores (one wave: its LDS
        // operations stay in order)
        double2 c8[8];
#pragma unroll
        for (int r8 = 0; r8 < 8; ++r8) c8[r8] = make_double2((double)xr[2 * r8] - mean, (double)xr[2 * r8 + 1] - mean);
        dft_small<8>(c8);
        double2 *Cb = v;
        {
            const int A = 8 * t + (t & 7);   // cidx(8t + r) = A ^ r
#pragma unroll
            for (int r8 = 0; r8 < 8; ++r8) Cb[A ^ r8] = c8[r8];
        }
        wave_sync();
        p2_fft<M, L, CLay<N>::LG, 3, 8, M, float, false>(Cb, (const float *)nullptr, 0.0, tw64, t);
        // the spectrum in conjugate bin pairs (k_diag_cl's post, 2 X_k)
        constexpr int JF = H / L;
        double best2 = 0.0;
#pragma unroll
        for (int j = 0; j < JF; ++j) {
            const int kk = t + L * j;
            const double2 zk = Cb[cidx(t) + L * j];
            const double2 zm = Cb[kk == 0 ? 0 : cidx(L - t) + (M - L * (j + 1))];
            spec_pair(zk, zm, tw64[kk], best2);
        }
        spec_self_pair(Cb[cidx(H)], tw64[H], best2);
        best2 = group_tree<1, 64>(best2, OpMaxF(), (double *)nullptr, 0, t);
        // a non-finite f32 sum means a NaN / Inf sample: some bin is NaN (k_diag_cl)
        fftv = isfinite(s32) ? 0.5 * sqrt(best2) : (double)NAN;
    } else {
        // w = 0: rfft of f64(X) = +-0 -> 0, unless R was non-finite (X NaN)
        int nanx = 0;
#pragma unroll
        for (int e = 0; e < 16; ++e) nanx |= isnan(xr[e]);
        nanx = group_tree<1, 64>(nanx, OpOr(), (int *)nullptr, 0, t);
        fftv = nanx ? NAN : 0.0;
    }
    if (t == 0) diag_store(a, p, valid, mean, sd, ptp, fftv);
}

// PP: per-profile delays (a.delay2, ic_set_delays2): each lane evaluates its
// phasors with ic_phasor instead of loading the channel's table row.
// ST: the residual's rotation measures its rows instead of storing them
// (RotateArgs.std_o; the direct layout only): the rotated row R, still in the
// lane's registers, becomes X = f32(R w0), whose mean / var / ptp run on the
// numpy pairwise chains (one LDS transposition into k_diag_cl's chain layout,
// the same trees: the same bits) and whose real spectrum comes from a third
// pass of the rotation's own FFT (max |rfft|, within 1e-9 of numpy like every
// diagnostics kernel's).  R never goes to HBM: the residual's 4N write and the
// statistics pass's 4N read are gone, and so is the R buffer.
template <int N, bool PP, bool ST = false>
// 3 waves per SIMD (137-167 VGPRs at N = 1024; 4 waves spill 2-13 VGPRs without
// the statistics: C2 fft 40.7 either way, fft_pp 40.9 -> 41.3 ms)
__global__ __launch_bounds__(RotCfg<N>::TB * RotCfg<N>::WPB, N <= 1024 ? 3 : 2) void k_rotate(RotateArgs a)
{
    using C = RotCfg<N>;
    constexpr int M = C::M, H = C::H, TB = C::TB, WPB = C::WPB;
    constexpr int NJ = (M / 2 + TB - 1) / TB;    // float4 rows per lane (4 samples = 2 points)
    constexpr int NK = H / TB + 1;               // spectrum pairs (k, M - k) per lane, k <= H
    // direct layout (every pass radix 8, one group per lane: N = 1024): lane t
    // loads points t + TB q (q < 8) straight into the first pass's registers and
    // stores the last pass's registers, which are the same points; two LDS round
    // trips per profile fewer
    constexpr bool DIRECT = C::LG % 3 == 0 && (M >> 3) == TB;
    // the wave's points (rot_slots f32 pairs); with the statistics the same
    // array holds their f64 FFT's M complex points
    constexpr int VS = ST ? 2 * M : rot_slots<M>();
    static_assert(rot_slots<M>() <= VS, "the rotation's slots fit");
    __shared__ __attribute__((aligned(16))) rc2 vv[WPB][VS];
    constexpr int TWE = p2_tw_entries(N);   // k_diag_p2's table: M plain + the stage tables
    // the twiddle table: f32 for the rotation, or f64 when the statistics FFT
    // needs it (the rotation then rounds each entry at its use)
    __shared__ rc2 tws32[C::TW_LDS ? (ST ? TWE - M : TWE) : 1];
    __shared__ double2 tws64[C::TW_LDS && ST ? TWE : 1];
    const int t = threadIdx.x % TB, wv = threadIdx.x / TB;
    rc2 *v = vv[wv];
    const unsigned nsub = (unsigned)a.nsub, nchan = (unsigned)a.nchan;
    const size_t P = (size_t)nsub * nchan;
    const float sg = a.sign > 0 ? 1.0f : -1.0f;
    const float inv = (float)(1.0 / (double)M);
    const __amdgpu_buffer_rsrc_t twr = rot_rsrc(a.tw_p2, 16u * TWE);
    const auto tw = [&]() {
        if constexpr (!C::TW_LDS) return TwGlobal<N>{twr};
        else if constexpr (ST) return TwLdsSt<N>{tws32, tws64};
        else return TwLds32<N>{tws32};
    }();
    if constexpr (C::TW_LDS) {
        for (int i = threadIdx.x; i < TWE; i += TB * WPB) {
            if constexpr (ST) {
                tws64[i] = a.tw_p2[i];
                if (i >= M) tws32[i - M] = rc2_of(a.tw_p2[i]);
            } else {
                tws32[i] = rc2_of(a.tw_p2[i]);
            }
        }
        __syncthreads();
    }
    // every global load of a profile in flight at once: one memory latency
    // per profile, not one per row (or per flag / fit lookup)
    auto load_rows = [&](size_t k, float4 (&xr)[NJ]) {
#pragma unroll
        for (int u = 0; u < NJ; ++u) {
            const int j2 = t + u * TB;
            if ((M / 2) % TB == 0 || j2 < M / 2)
            {
                // non-temporal, as the direct layout's (C5 fft 58.8 -> 57.4-57.9 ms,
                // C4 fft 3.90 -> 3.76 ms with the stores below)
                const fv4 xv = __builtin_nontemporal_load((const fv4 *)(a.in + d_ofs(k, 4 * j2, (int)a.ld_in, a.in_tiled)));
                xr[u] = make_float4(xv.x, xv.y, xv.z, xv.w);
            }
        }
    };
    // the profile is left out (uniform over the block): its subint's flag is 0,
    // or its late flag is not the one selected
    auto skip = [&](size_t p, unsigned s) {
        return (a.flags && a.flags[s] == 0) || (a.late && ((a.late[p] != 0) != (a.late_sel != 0)));
    };
    // a block's profiles are consecutive items (channel-major): they share a
    // channel's phasor row
    // items: channel-major over every profile, or the profiles of a round list
    // (RotateArgs.list: the diagnostics fork's second pass, the profiles still
    // fitting at its round - a scan of every profile for their late flags cost
    // that pass 2.7-3.4 ms per iteration on C2 for a tenth of the profiles)
    const RoundList rl(a.list, a.nctr, (long)P);
    const size_t nitems = a.list ? (size_t)rl.n() : P;
    for (size_t item = (size_t)blockIdx.x * WPB + wv; item < nitems; item += (size_t)gridDim.x * WPB) {
        unsigned c, s;
        size_t p;
        if (a.list) {
            p = (size_t)rl.at((long)item);
            c = (unsigned)(p % nchan);
            s = (unsigned)(p / nchan);
        } else {
            c = (unsigned)(item / nsub);
            s = (unsigned)(item % nsub);
            p = (size_t)s * nchan + c;
        }
        if (skip(p, s)) continue;
        // the channel's f32 phasor row (8 bytes per harmonic)
        const __amdgpu_buffer_rsrc_t phr = rot_rsrc(PP ? (const void *)a.tw : (const void *)(a.ph + 2 * (size_t)c * (M + 1)),
                                                    8u * (M + 1));
        const double dly = PP ? a.delay2[p] : 0.0;
        // PP, N >= 256 (M a multiple of 64): the lane's harmonics k = t + u TB
        // and M - k have the low parts lo1 = t mod 64 and lo2 = -t mod 64 in
        // every round, and high parts that are the same across the wave: w0 + u
        // TB for k, and M - 64 - w0 - u TB for M - k (M - w0 - u TB where lo1 =
        // 0), w0 = t - lo1.  So a lane evaluates P0(lo1), P0(lo2) and one of
        // the wave's 3 NK high parts (lane j), and every round reads its high
        // parts from lanes u, NK + u, 2 NK + u (ic_phasor's product form: 3
        // polynomials per lane instead of 2 NK)
        constexpr bool PPX = PP && N >= 256;
        const int lo1 = t & 63, w0 = t - lo1;
        double2 A1{}, A2{}, Bh{};
        if constexpr (PPX) {
            const int lo2 = (64 - lo1) & 63, j = lo1;
            int hv = j < NK ? w0 + j * TB : (j < 2 * NK ? M - 64 - w0 - (j - NK) * TB : M - w0 - (j - 2 * NK) * TB);
            if (j >= 3 * NK || hv < 0) hv = 0;
            A1 = ic_phasor0(lo1, dly, N);
            A2 = ic_phasor0(lo2, dly, N);
            Bh = ic_phasor0(hv, dly, N);
        }
        auto bcast = [&](int lane) {
            return make_double2(__hiloint2double(__builtin_amdgcn_readlane(__double2hiint(Bh.x), lane),
                                                 __builtin_amdgcn_readlane(__double2loint(Bh.x), lane)),
                                __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(Bh.y), lane),
                                                 __builtin_amdgcn_readlane(__double2loint(Bh.y), lane)));
        };
        // the post step's phasors one round ahead: the first round's are
        // requested with the rows, each later round's before the round before it
        // RM (N >= 256): the last round would hold k = H alone, in lane 0.  Lane
        // 0 takes it in round 0 instead of the DC / Nyquist bins, which it
        // finishes after the rounds: no round with one active lane and no
        // divergent branch in round 0 (the schedule only: the same operations).
        // Per-channel C2 46.8 -> 46.4 ms (f64 rotation); with per-profile
        // delays it spilled in f64 (48.1 -> 48.6), in f32 it gains (39.8 -> 39.6)
        constexpr bool RM = H % TB == 0;
        constexpr int NR = RM ? NK - 1 : NK;
        auto kof = [&](int u) { return (RM && u == 0 && t == 0) ? H : t + u * TB; };
        // the phasors (f64, ic_phasor) rounded to f32 at the use; the table's are f32
        auto ldph = [&](int u, rc2 (&pp)[2]) {
            const int k = kof(u);
            if constexpr (PPX) {
                const double2 b1 = bcast(u), b2 = bcast(NK + u), b3 = bcast(2 * NK + u);
                if (k <= H) {
                    pp[0] = rc2_of(lo1 == 0 ? b1 : (w0 + u * TB == 0 ? A1 : ic_phasor_mul(A1, b1)));
                    pp[1] = rc2_of(lo1 == 0 ? b3 : (M - 64 - w0 - u * TB == 0 ? A2 : ic_phasor_mul(A2, b2)));
                }
                if (RM && u == 0) {   // lane 0's k = H: P0(H) from the round NK - 1 parts
                    const double2 bh = bcast(NK - 1), bh3 = bcast(3 * NK - 1);
                    if (t == 0) {
                        pp[0] = rc2_of(bh);
                        pp[1] = rc2_of(bh3);
                    }
                }
            } else if (k <= H) {
                if constexpr (PP) {
                    pp[0] = rc2_of(ic_phasor(k, dly, N));
                    pp[1] = rc2_of(ic_phasor(M - k, dly, N));
                } else {
                    pp[0] = rot_ld2(phr, 8u * (unsigned)k, 0);
                    pp[1] = rot_ld2(phr, 8u * (unsigned)(M - k), 0);
                }
            }
        };
        rc2 phn[2];
        ldph(0, phn);
        rc2 z[8];
        static_assert(!ST || DIRECT, "the statistics epilogue needs the direct layout");
        float wst = 1.0f;   // ST: the profile's weight, requested with the rows
        if constexpr (ST) wst = a.w0[p];
        if constexpr (DIRECT) {
            const size_t k = p;
            float2 x2[8];
#pragma unroll
            for (int q = 0; q < 8; ++q)
            {
                // read once per rotation (non-temporal: C2 fft 39.25-39.42 -> 39.05-39.25 ms)
                const rc2 xv =
                    __builtin_nontemporal_load((const rc2 *)(a.in + d_ofs(k, 2 * (t + TB * q), (int)a.ld_in, a.in_tiled)));
                x2[q] = make_float2(xv.x, xv.y);
            }
            if (a.amp) {
                const __amdgpu_buffer_rsrc_t t64r = rot_rsrc(a.T64, 16u * M);
                double2 tt[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) tt[q] = rot_ld(t64r, 16u * (unsigned)t, 16u * (unsigned)(TB * q));
                const bool ok = fit_ok(a.info[p]);
                const double am = a.amp[p];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    float r[2] = {0.0f, 0.0f};
                    if (ok) {
                        const float pv[2] = {x2[q].x, x2[q].y};
                        const double tv[2] = {tt[q].x, tt[q].y};
#pragma unroll
                        for (int e = 0; e < 2; ++e) {
                            r[e] = residual_sample(am, tv[e], pv[e], 2 * (t + TB * q) + e, a);
                        }
                    }
                    z[q] = (rc2){r[0], r[1]};
                }
            } else {
                const float b = a.base ? a.base[p] : 0.0f;
#pragma unroll
                for (int q = 0; q < 8; ++q) z[q] = (rc2){x2[q].x, x2[q].y} - (rc2){b, b};
            }
            rot_fft<N, 0, true, false>(v, tw, t, z);
        } else {
        float4 xin[NJ];
        load_rows(p, xin);
        if (a.amp) {
            // the residual of the exact fit (k_residual's arithmetic), formed on the fly;
            // the template is requested with the rows, before the status is known
            // (behind the scattered amp / info loads it was a second latency)
            const __amdgpu_buffer_rsrc_t t64r = rot_rsrc(a.T64, 16u * M);
            double2 tt[NJ][2];
#pragma unroll
            for (int u = 0; u < NJ; ++u) {
                const int j2 = t + u * TB;
                if ((M / 2) % TB != 0 && j2 >= M / 2) break;
                tt[u][0] = rot_ld(t64r, 32u * (unsigned)t, 32u * (unsigned)(u * TB));
                tt[u][1] = rot_ld(t64r, 32u * (unsigned)t, 32u * (unsigned)(u * TB) + 16u);
            }
            const bool ok = fit_ok(a.info[p]);
            const double am = a.amp[p];
#pragma unroll
            for (int u = 0; u < NJ; ++u) {
                const int j2 = t + u * TB;
                if ((M / 2) % TB != 0 && j2 >= M / 2) break;
                float r[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                if (ok) {
                    const float pv[4] = {xin[u].x, xin[u].y, xin[u].z, xin[u].w};
                    const double tv[4] = {tt[u][0].x, tt[u][0].y, tt[u][1].x, tt[u][1].y};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        r[e] = residual_sample(am, tv[e], pv[e], 4 * j2 + e, a);
                    }
                }
                v[rsl(2 * j2)] = (rc2){r[0], r[1]};
                v[rsl(2 * j2 + 1)] = (rc2){r[2], r[3]};
            }
        } else {
            const float b = a.base ? a.base[p] : 0.0f;
#pragma unroll
            for (int u = 0; u < NJ; ++u) {
                const int j2 = t + u * TB;
                if ((M / 2) % TB != 0 && j2 >= M / 2) break;
                v[rsl(2 * j2)] = (rc2){xin[u].x, xin[u].y} - (rc2){b, b};
                v[rsl(2 * j2 + 1)] = (rc2){xin[u].z, xin[u].w} - (rc2){b, b};
            }
        }
        gsync<TB / 64>();
        rot_fft<N>(v, tw, t);
        }
        // the post step's twiddles, at their use
        // Re P(M) for the DC / Nyquist step after the rounds (RM); P(0) = (1, 0)
        // exactly for every delay, so Y_0 = X_0 * 1 = X_0
        float pmr = 0.0f;
        if constexpr (RM) {
            if constexpr (PPX) pmr = (float)bcast(2 * NK).x;   // P0(M), lane 2 NK of the wave's high parts
            else pmr = rot_ld2(phr, 8u * (unsigned)M, 0).x;
        }
        const rc2 sgv = {1.0f, sg};
#pragma unroll
        for (int u = 0; u < NR; ++u) {
            const int k = kof(u);
            const rc2 wk = k <= H ? tw.post((unsigned)(k & (M - 1))) : (rc2){0.0f, 0.0f};
            const rc2 pk = phn[0], pq = phn[1];
            if (u + 1 < NR) ldph(u + 1, phn);
            if (k <= H) {
                if (!RM && k == 0) {
                    v[rsl(0)] = rot_dc_nyquist(v[rsl(0)], pk.x, pq.x);
                } else {
                    const int q = M - k;
                    const rc2 zk = v[rsl(k)], zq = v[rsl(q)];
                    rc2 Zk, Zq;   // conjugated
                    rot_pair(zk, zq, wk, pk * sgv, pq * sgv, Zk, Zq);
                    v[rsl(q)] = Zq;
                    v[rsl(k)] = Zk;
                }
            }
        }
        if constexpr (RM) {
            if (t == 0) v[rsl(0)] = rot_dc_nyquist(v[rsl(0)], 1.0f, pmr);   // P(0) = 1: Y_0 = X_0 exactly
        }
        gsync<TB / 64>();
        float *o = a.out + p * (size_t)a.ldo;
        const rc2 scl = {inv, -inv};   // (r.re / M, -r.im / M): x (-1/M) = -(x) (1/M)
        if constexpr (ST) {
            rot_fft<N, 0, false, true>(v, tw, t, z);
            rot_stats<N>(a, p, (double2 *)v, tws64, t, z, inv, wst);
        } else if constexpr (DIRECT) {
            rot_fft<N, 0, false, true>(v, tw, t, z);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int j = t + TB * q;
                // written once, read by later kernels: non-temporal stores
                // (C2 fft 39.71-39.95 -> 39.43-39.53 ms; only out2's: 39.56-39.75)
                const rc2 yv = z[q] * scl;
                __builtin_nontemporal_store(yv, (rc2 *)(o + 2 * j));
                if (a.out2) __builtin_nontemporal_store(yv, (rc2 *)(a.out2 + d_ofs(p, 2 * j, (int)a.ldo2, a.out2_tiled)));
            }
        } else {
            rot_fft<N>(v, tw, t);
#pragma unroll
            for (int u = 0; u < NJ; ++u) {
                const int j2 = t + u * TB;
                if ((M / 2) % TB != 0 && j2 >= M / 2) break;
                const rc2 r0 = v[rsl(2 * j2)] * scl, r1 = v[rsl(2 * j2 + 1)] * scl;
                const float4 y = make_float4(r0.x, r0.y, r1.x, r1.y);
                const fv4 yv = {y.x, y.y, y.z, y.w};
                __builtin_nontemporal_store(yv, (fv4 *)(o + 4 * j2));
                if (a.out2) __builtin_nontemporal_store(yv, (fv4 *)(a.out2 + d_ofs(p, 4 * j2, (int)a.ldo2, a.out2_tiled)));
            }
        }
        gsync<TB / 64>();   // v is reused by the block's next profile
    }
}

// ---------------------------------------------------------------------------
// k_rotate_mr: the same rotation for the mixed-radix lengths (mr_supported:
// N = 2M, M = 2^a 3^b 5^c, N a multiple of 8, 64 .. 4096), N a runtime value.
// One wave per profile, blockDim.x / 64 waves per block; a wave's M complex
// points ping-pong between two LDS buffers (8 N bytes per wave), one Stockham
// stage per trip, and the block shares the f32 twiddle table (tw[q], q < N: 8 N
// bytes, staged once per block).  The host factors M (mr_plan: the stage order
// of phase_rotation.py stage_radices) and passes the radices as 4-bit fields;
// the kernel switches per stage to the radix-templated body.  Every complex
// operation is the packed f32 arithmetic of k_rotate (each half one IEEE f32
// operation of the definition), rows move as 16-byte accesses and every global
// load of a profile is issued before the first stage.  NJ: float4 rows per lane
// (N <= 256 NJ).  PP: per-profile delays (RotateArgs.delay2).
// DFT_3 / DFT_5 in the written order of phase_rotation.py (_dft3, _dft5)
__device__ __forceinline__ void rot_dft3(rc2 *b)
{
    constexpr float s3 = (float)0x1.bb67ae8584caap-1;   // f32(f64(sqrt(3)/2))
    const rc2 t = b[1] + b[2], d = b[1] - b[2];
    const rc2 m = b[0] - t * (rc2){0.5f, 0.5f};
    const rc2 e = d * (rc2){s3, s3};
    b[0] = b[0] + t;
    b[1] = pk_mi(m, e);   // m - i e
    b[2] = pk_pi(m, e);   // m + i e
}
__device__ __forceinline__ void rot_dft5(rc2 *b)
{
    constexpr float c1 = (float)0x1.3c6ef372fe950p-2;    // f32(f64(cos(2 pi/5)))
    constexpr float c2 = (float)-0x1.9e3779b97f4a8p-1;   // f32(f64(cos(4 pi/5)))
    constexpr float s1 = (float)0x1.e6f0e134454ffp-1;    // f32(f64(sin(2 pi/5)))
    constexpr float s2 = (float)0x1.2cf2304755a5ep-1;    // f32(f64(sin(4 pi/5)))
    const rc2 t1 = b[1] + b[4], t2 = b[2] + b[3], d1 = b[1] - b[4], d2 = b[2] - b[3];
    const rc2 m1 = (b[0] + t1 * (rc2){c1, c1}) + t2 * (rc2){c2, c2};
    const rc2 m2 = (b[0] + t1 * (rc2){c2, c2}) + t2 * (rc2){c1, c1};
    const rc2 e1 = d1 * (rc2){s1, s1} + d2 * (rc2){s2, s2};
    const rc2 e2 = d1 * (rc2){s2, s2} - d2 * (rc2){s1, s1};
    b[0] = b[0] + (t1 + t2);
    b[1] = pk_mi(m1, e1);
    b[2] = pk_mi(m2, e2);
    b[3] = pk_pi(m2, e2);
    b[4] = pk_pi(m1, e1);
}

// One stage of radix R and span ns (the product of the earlier radices) of the
// wave's FFT_M: butterfly j < G = M/R reads in[j + q G], multiplies by
// tw[q k step] (k = j mod ns, step = N/(R ns); not in the first stage), and
// writes DFT_R's y_p to out[(j - k) R + k + p ns].  magic = ceil(2^32 / ns):
// j / ns = (j magic) >> 32 exactly for j, ns < 2^16.
template <int R>
__device__ __forceinline__ void mr_stage(const rc2 *in, rc2 *out, const rc2 *tw, int M, int step, int ns, int lane)
{
    const int G = M / R;
    const unsigned magic = ns > 1 ? 0xffffffffu / (unsigned)ns + 1u : 0u;
    for (int j = lane; j < G; j += 64) {
        const int k = ns > 1 ? j - (int)__umulhi((unsigned)j, magic) * ns : 0;
        rc2 u[R];
#pragma unroll
        for (int q = 0; q < R; ++q) u[q] = in[j + q * G];
        if (ns > 1) {
            rc2 w[R];
#pragma unroll
            for (int q = 1; q < R; ++q) w[q] = tw[q * k * step];
#pragma unroll
            for (int q = 1; q < R; ++q) u[q] = rot_cmul(u[q], w[q]);
        }
        if constexpr (R == 8) {
            rot_dft8(u);
        } else if constexpr (R == 5) {
            rot_dft5(u);
        } else if constexpr (R == 4) {
            rot_dft4(u);
        } else if constexpr (R == 3) {
            rot_dft3(u);
        } else {
            const rc2 a = u[0], b = u[1];
            u[0] = a + b;
            u[1] = a - b;
        }
        rc2 *o = out + (j - k) * R + k;
#pragma unroll
        for (int p = 0; p < R; ++p) o[p * ns] = u[p];
    }
}

// FFT_M of the wave's points in `a` (stages ping-pong between a and b);
// returns the buffer that holds the result
__device__ __forceinline__ rc2 *mr_fft(rc2 *a, rc2 *b, const rc2 *tw, int M, int N, unsigned long long radices,
                                       int nst, int lane)
{
    int ns = 1, step = N;
    for (int s = 0; s < nst; ++s) {
        const int R = (int)((radices >> (4 * s)) & 15);
        step /= R;
        switch (R) {
        case 8: mr_stage<8>(a, b, tw, M, step, ns, lane); break;
        case 5: mr_stage<5>(a, b, tw, M, step, ns, lane); break;
        case 4: mr_stage<4>(a, b, tw, M, step, ns, lane); break;
        case 3: mr_stage<3>(a, b, tw, M, step, ns, lane); break;
        default: mr_stage<2>(a, b, tw, M, step, ns, lane); break;
        }
        ns *= R;
        rc2 *t = a;
        a = b;
        b = t;
        wave_sync();
    }
    return a;
}

template <int NJ, bool PP>
__global__ __launch_bounds__(256) void k_rotate_mr(RotateArgs a, unsigned long long radices, int nst)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char mr_sm[];
    const int N = a.nbin, M = N >> 1, H = M >> 1, NQ = N >> 2;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    rc2 *tws = (rc2 *)mr_sm;                      // [N] f32 of tw
    rc2 *v0 = tws + N + (size_t)wv * 2 * M;       // the wave's two buffers of M points
    rc2 *v1 = v0 + M;
    for (int i = threadIdx.x; i < N; i += blockDim.x) tws[i] = rc2_of(a.tw[i]);
    __syncthreads();
    const unsigned nsub = (unsigned)a.nsub, nchan = (unsigned)a.nchan;
    const size_t P = (size_t)nsub * nchan;
    const rc2 sgv = {1.0f, a.sign > 0 ? 1.0f : -1.0f};
    const float inv = (float)(1.0 / (double)M);
    const rc2 scl = {inv, -inv};   // (r.re / M, -r.im / M): x (-1/M) = -(x) (1/M)
    const RoundList rl(a.list, a.nctr, (long)P);
    const size_t nitems = a.list ? (size_t)rl.n() : P;
    // items and skips as k_rotate's, restated (a shared helper changed both kernels' code): edit both
    for (size_t item = (size_t)blockIdx.x * wpb + wv; item < nitems; item += (size_t)gridDim.x * wpb) {
        unsigned c, s;
        size_t p;
        if (a.list) {
            p = (size_t)rl.at((long)item);
            c = (unsigned)(p % nchan);
            s = (unsigned)(p / nchan);
        } else {
            c = (unsigned)(item / nsub);
            s = (unsigned)(item % nsub);
            p = (size_t)s * nchan + c;
        }
        if ((a.flags && a.flags[s] == 0) || (a.late && ((a.late[p] != 0) != (a.late_sel != 0)))) continue;
        // every global load of the profile in flight at once
        fv4 xin[NJ];
#pragma unroll
        for (int u = 0; u < NJ; ++u) {
            const int j4 = lane + 64 * u;
            if (j4 < NQ)
                xin[u] = __builtin_nontemporal_load((const fv4 *)(a.in + d_ofs(p, 4 * j4, (int)a.ld_in, a.in_tiled)));
        }
        // PP: the profile's phasor parts (ic_phasor's product form): lane l holds
        // the low part P0(l) and the high part P0(64 l) (64 l <= M), evaluated
        // once per profile
        double2 Alo{}, Bhi{};
        const float *phc = nullptr;
        if constexpr (PP) {
            const double dly = a.delay2[p];
            Alo = ic_phasor0(lane, dly, N);
            Bhi = ic_phasor0(64 * lane <= M ? 64 * lane : 0, dly, N);
        } else {
            phc = a.ph + 2 * (size_t)c * (M + 1);
        }
        // f32(ic_phasor(k, delay, N)), k <= M; every lane of the wave calls it together
        auto phasor = [&](int k) {
            if constexpr (PP) {
                const int lo = k & 63, hi = k >> 6;
                const double2 A = make_double2(__shfl(Alo.x, lo), __shfl(Alo.y, lo));
                const double2 B = make_double2(__shfl(Bhi.x, hi), __shfl(Bhi.y, hi));
                return rc2_of(lo == 0 ? B : (hi == 0 ? A : ic_phasor_mul(A, B)));
            } else {
                return *(const rc2 *)(phc + 2 * k);
            }
        };
        if (a.amp) {
            // the residual of the exact fit (k_residual's arithmetic), formed on the fly
            const bool ok = fit_ok(a.info[p]);
            const double am = a.amp[p];
#pragma unroll
            for (int u = 0; u < NJ; ++u) {
                const int j4 = lane + 64 * u;
                if (j4 >= NQ) break;
                float r[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                if (ok) {
                    const double2 ta = *(const double2 *)(a.T64 + 4 * j4), tb = *(const double2 *)(a.T64 + 4 * j4 + 2);
                    const float pv[4] = {xin[u].x, xin[u].y, xin[u].z, xin[u].w};
                    const double tv[4] = {ta.x, ta.y, tb.x, tb.y};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        r[e] = residual_sample(am, tv[e], pv[e], 4 * j4 + e, a);
                    }
                }
                *(fv4 *)(v0 + 2 * j4) = (fv4){r[0], r[1], r[2], r[3]};
            }
        } else {
            const float b = a.base ? a.base[p] : 0.0f;
#pragma unroll
            for (int u = 0; u < NJ; ++u) {
                const int j4 = lane + 64 * u;
                if (j4 >= NQ) break;
                *(fv4 *)(v0 + 2 * j4) = xin[u] - (fv4){b, b, b, b};
            }
        }
        wave_sync();
        rc2 *z = mr_fft(v0, v1, tws, M, N, radices, nst, lane);
        // pairs (k, M - k), k = 1 .. H, in place; lane 0's first slot is the DC /
        // Nyquist step.  Uniform trip count: the shuffles of phasor() need every lane
        for (int k0 = 0; k0 <= H; k0 += 64) {
            const int k = k0 + lane, kc = k <= H ? k : H;
            const rc2 pk = phasor(kc), pq = phasor(M - kc);
            if (k == 0) {
                z[0] = rot_dc_nyquist(z[0], pk.x, pq.x);
            } else if (k <= H) {
                const int q = M - k;
                rc2 Zk, Zq;   // conjugated
                rot_pair(z[k], z[q], tws[k], pk * sgv, pq * sgv, Zk, Zq);
                z[q] = Zq;
                z[k] = Zk;   // k = M/2 pairs with itself: the k values are stored last
            }
        }
        wave_sync();
        rc2 *r = mr_fft(z, z == v0 ? v1 : v0, tws, M, N, radices, nst, lane);
        float *o = a.out + p * (size_t)a.ldo;
#pragma unroll
        for (int u = 0; u < NJ; ++u) {
            const int j4 = lane + 64 * u;
            if (j4 >= NQ) break;
            const rc2 r0 = r[2 * j4] * scl, r1 = r[2 * j4 + 1] * scl;
            const fv4 yv = {r0.x, r0.y, r1.x, r1.y};
            __builtin_nontemporal_store(yv, (fv4 *)(o + 4 * j4));
            if (a.out2) __builtin_nontemporal_store(yv, (fv4 *)(a.out2 + d_ofs(p, 4 * j4, (int)a.ldo2, a.out2_tiled)));
        }
        wave_sync();   // the buffers are reused by the wave's next profile
    }
}

// ---------------------------------------------------------------------------
// k_rotate_czt: the opt-in rotation of any other length n in 16 .. 4096
// (czt_supported; phase_rotation.py rotate_czt), odd and prime n included, by
// Bluestein's chirp-z transform: DFT_n as a circular convolution of length
// L = czt_length(n) with the chirp w[j] = exp(-i pi j^2 / n),
//   conj(DFT_n(a)) L = FFT_L(conj(FFT_L(a w, zero-padded) B)),  B = FFT_L(conj w),
// run twice: on the real row, and on conj(Y) of the spectrum times the phasors.
//   1. v[j] = x'[j] w[j] (x' = f32(x - base), or the residual), 0 for j >= n
//   2. V = FFT_L(v); V = conj(V B); D = FFT_L(V)
//   3. k < n: X = (conj(D[k]) w[k]) / L; Y = X P (harmonic k <= n/2: (P.r,
//      sign P.i)[k]; k > n/2: its conjugate at n - k; the Nyquist harmonic of
//      an even n: both parts by P.r); v[k] = conj(Y) w[k], 0 for k >= n
//   4. step 2 again; out[j] = (Re(conj(D[j]) w[j]) / L) (1/n)
// One wave per profile, n and L runtime values; the wave's L complex points
// ping-pong between two LDS buffers (16 L bytes), one Stockham stage (mr_stage,
// radices 8 / 4 / 2) per trip.  The per-length tables (RotateArgs.czt: tw of L,
// B, w; f32 pairs in HBM, shared by every profile) are read through L1/L2,
// except that up to L = 4096 the block stages tw in LDS (TWG = false); at
// L = 8192 the two buffers take 128 KiB of the CU's 160 and tw stays global
// (TWG).  Rows of these lengths are not 16-byte aligned in general: every row
// access is a 4-byte one, a wave's 64 consecutive.  Every complex operation is
// the packed f32 arithmetic of k_rotate.  PP: per-profile delays.
template <bool PP, bool TWG>
__global__ __launch_bounds__(256) void k_rotate_czt(RotateArgs a, int L, unsigned long long radices, int nst)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char czt_sm[];
    const int n = a.nbin, hn = n >> 1;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    const rc2 *gtw = (const rc2 *)a.czt, *B = gtw + L, *ch = B + L;
    rc2 *tws = (rc2 *)czt_sm;                                   // [L] tw (not TWG)
    rc2 *v0 = tws + (TWG ? 0 : L) + (size_t)wv * 2 * L;         // the wave's two buffers of L points
    rc2 *v1 = v0 + L;
    if constexpr (!TWG) {
        for (int i = threadIdx.x; i < L; i += blockDim.x) tws[i] = gtw[i];
        __syncthreads();
    }
    const unsigned nsub = (unsigned)a.nsub, nchan = (unsigned)a.nchan;
    const size_t P = (size_t)nsub * nchan;
    const rc2 sgv = {1.0f, a.sign > 0 ? 1.0f : -1.0f};
    const rc2 cj = {1.0f, -1.0f};
    const float invL = 1.0f / (float)L;   // exact: L is a power of two
    const float invn = (float)(1.0 / (double)n);
    const RoundList rl(a.list, a.nctr, (long)P);
    const size_t nitems = a.list ? (size_t)rl.n() : P;
    // FFT_L of the points in `z`, times B, conjugated, FFT_L again: returns the buffer of D
    const auto convolve = [&](rc2 *z) {
        rc2 *o = z == v0 ? v1 : v0;
        if constexpr (TWG) z = mr_fft(z, o, gtw, L, L, radices, nst, lane);
        else z = mr_fft(z, o, tws, L, L, radices, nst, lane);
        for (int i = lane; i < L; i += 64) z[i] = rot_cmul(z[i], B[i]) * cj;
        wave_sync();
        o = z == v0 ? v1 : v0;
        if constexpr (TWG) return mr_fft(z, o, gtw, L, L, radices, nst, lane);
        else return mr_fft(z, o, tws, L, L, radices, nst, lane);
    };
    // items and skips as k_rotate's, restated (a shared helper changed both kernels' code): edit both
    for (size_t item = (size_t)blockIdx.x * wpb + wv; item < nitems; item += (size_t)gridDim.x * wpb) {
        unsigned c, s;
        size_t p;
        if (a.list) {
            p = (size_t)rl.at((long)item);
            c = (unsigned)(p % nchan);
            s = (unsigned)(p / nchan);
        } else {
            c = (unsigned)(item / nsub);
            s = (unsigned)(item % nsub);
            p = (size_t)s * nchan + c;
        }
        if ((a.flags && a.flags[s] == 0) || (a.late && ((a.late[p] != 0) != (a.late_sel != 0)))) continue;
        // PP: the profile's phasor parts as k_rotate_mr's
        double2 Alo{}, Bhi{};
        const float *phc = nullptr;
        if constexpr (PP) {
            const double dly = a.delay2[p];
            Alo = ic_phasor0(lane, dly, n);
            Bhi = ic_phasor0(64 * lane <= hn ? 64 * lane : 0, dly, n);
        } else {
            phc = a.ph + 2 * (size_t)c * (hn + 1);
        }
        // f32(ic_phasor(k, delay, n)), k <= n/2; every lane of the wave calls it together
        auto phasor = [&](int k) {
            if constexpr (PP) {
                const int lo = k & 63, hi = k >> 6;
                const double2 A = make_double2(__shfl(Alo.x, lo), __shfl(Alo.y, lo));
                const double2 Bh = make_double2(__shfl(Bhi.x, hi), __shfl(Bhi.y, hi));
                return rc2_of(lo == 0 ? Bh : (hi == 0 ? A : ic_phasor_mul(A, Bh)));
            } else {
                return *(const rc2 *)(phc + 2 * k);
            }
        };
        {
            const bool res = a.amp != nullptr;
            const bool ok = res && fit_ok(a.info[p]);
            const double am = res ? a.amp[p] : 0.0;
            const float b = (!res && a.base) ? a.base[p] : 0.0f;
            for (int j = lane; j < L; j += 64) {
                rc2 v = {0.0f, 0.0f};
                if (j < n) {
                    const float xin = a.in[d_ofs(p, j, (int)a.ld_in, a.in_tiled)];
                    // the residual of the exact fit (k_residual's arithmetic), formed on the fly
                    const float x = res ? (ok ? residual_sample(am, a.T64[j], xin, j, a) : 0.0f) : xin - b;
                    v = (rc2){x, x} * ch[j];
                }
                v0[j] = v;
            }
        }
        wave_sync();
        rc2 *z = convolve(v0);
        // the spectrum times the phasors, conjugated, times the chirp.  Uniform
        // trip count: the shuffles of phasor() need every lane
        for (int k0 = 0; k0 < L; k0 += 64) {
            const int k = k0 + lane;
            if (k0 < n) {
                const int kc = k < n ? k : n - 1;
                const bool up = kc > hn;
                rc2 pk = phasor(up ? n - kc : kc) * sgv;
                if (up) pk = pk * cj;
                if (k < n) {
                    const rc2 w = ch[k];
                    const rc2 X = rot_cmul(z[k] * cj, w) * (rc2){invL, invL};
                    const rc2 Y = (2 * k == n) ? X * pk.xx : rot_cmul(X, pk);
                    z[k] = rot_cmul(Y * cj, w);
                }
            }
            if (k >= n && k < L) z[k] = (rc2){0.0f, 0.0f};   // L may be 32
        }
        wave_sync();
        const rc2 *r = convolve(z);
        float *o = a.out + p * (size_t)a.ldo;
        for (int j = lane; j < n; j += 64) {
            const float y = (rot_cmul(r[j] * cj, ch[j]).x * invL) * invn;
            o[j] = y;
            if (a.out2) a.out2[d_ofs(p, j, (int)a.ldo2, a.out2_tiled)] = y;
        }
        wave_sync();   // the buffers are reused by the wave's next profile
    }
}

// The channel phasor table of the FFT dedispersion (RotateArgs.ph) from the
// channels' delays on the device: ph[c][k] = f32(ic_phasor(k, delay[c], nbin)),
// k <= nbin/2.  One element per thread, k fastest (a wave stores 512
// contiguous bytes), grid-stride.  ic_phasor is the function the host's table
// (make_phasors) and k_rotate's per-profile path evaluate; with
// -ffp-contract=off its separately rounded f64 operations give the same bits
// here.  n < 2^31 (launch_phasor_table).
__global__ __launch_bounds__(256) void k_phasor_table(const double *__restrict__ delay, float2 *__restrict__ ph,
                                                      uint32_t n, uint32_t row, int nbin)
{
    const uint32_t step = gridDim.x * blockDim.x;
    // i + step cannot wrap: n < 2^31 and step <= 65536 * 256
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
        const uint32_t c = i / row, k = i - c * row;
        const double2 v = ic_phasor((int)k, delay[c], nbin);
        ph[i] = make_float2((float)v.x, (float)v.y);
    }
}

// ============================================================ launchers

hipError_t launch_phasor_table(hipStream_t st, const double *delay, int nchan, int nbin, float *ph, int grid_cap)
{
    if (nchan < 1 || nbin < 2 || !delay || !ph) return hipErrorInvalidValue;
    const size_t row = (size_t)nbin / 2 + 1, n = (size_t)nchan * row;
    if (n >= ((size_t)1 << 31)) return hipErrorInvalidValue;
    const unsigned grid = cap_grid(std::min<size_t>(cdiv(n, 256), 65536), grid_cap);
    IC_GGL(k_phasor_table, dim3(grid), dim3(256), 0, st, delay, (float2 *)ph, (uint32_t)n, (uint32_t)row, nbin);
    return hipGetLastError();
}

bool rotate_supported(int nbin) { return p2_supported(nbin) || mr_supported(nbin); }

// k_rotate_mr: the stages from mr_plan (ic_internal.h); waves per block from the LDS it needs, 8 nbin bytes for the
// block's f32 twiddle table and 8 nbin per wave, within kMrLdsBytes
static hipError_t launch_rotate_mr(hipStream_t st, const RotateArgs &a, size_t P)
{
    unsigned long long radices = 0;
    const int nst = mr_plan(a.nbin, &radices);
    if (!nst) return hipErrorInvalidValue;
    const size_t unit = 8 * (size_t)a.nbin;
    const int wpb = (int)std::min<size_t>(4, kMrLdsBytes / unit - 1);
    if (wpb < 1) return hipErrorInvalidValue;
    const size_t shm = unit * (size_t)(1 + wpb);
    const dim3 grid(cap_grid(std::min<size_t>(cdiv(P, wpb), 2048), a.grid_cap)), block(64 * wpb);
    const int rows = (a.nbin / 4 + 63) / 64;   // float4 rows per lane
#define IC_ROT_MR(NJ)                                                                              \
    if (rows <= NJ) {                                                                              \
        if (a.delay2) IC_GGL((k_rotate_mr<NJ, true>), grid, block, shm, st, a, radices, nst);      \
        else IC_GGL((k_rotate_mr<NJ, false>), grid, block, shm, st, a, radices, nst);              \
        return hipGetLastError();                                                                  \
    }
    IC_ROT_MR(4)
    IC_ROT_MR(8)
    IC_ROT_MR(16)
#undef IC_ROT_MR
    return hipErrorInvalidValue;
}

// k_rotate_czt: FFT_L's stages from mr_plan(2 L); waves per block from the LDS it needs, 16 L bytes per wave and 8 L
// for the block's f32 twiddle table (L <= 4096), within kMrLdsBytes where one wave fits there: L = 4096 takes 96 KiB
// for its one wave, L = 8192 128 KiB without the table
static hipError_t launch_rotate_czt(hipStream_t st, const RotateArgs &a, size_t P)
{
    const int L = czt_length(a.nbin);
    unsigned long long radices = 0;
    const int nst = mr_plan(2 * L, &radices);
    if (!nst || L < 32 || L > 8192) return hipErrorInvalidValue;
    const bool twg = L > 4096;
    const size_t tab = twg ? 0 : 8 * (size_t)L, unit = 16 * (size_t)L;
    const int wpb = kMrLdsBytes > tab + unit ? (int)std::min<size_t>(4, (kMrLdsBytes - tab) / unit) : 1;
    const size_t shm = tab + unit * (size_t)wpb;
    if (shm > kLdsBudget) return hipErrorInvalidValue;
    const dim3 grid(cap_grid(std::min<size_t>(cdiv(P, wpb), 2048), a.grid_cap)), block(64 * wpb);
    if (twg) {
        if (a.delay2) IC_GGL((k_rotate_czt<true, true>), grid, block, shm, st, a, L, radices, nst);
        else IC_GGL((k_rotate_czt<false, true>), grid, block, shm, st, a, L, radices, nst);
    } else {
        if (a.delay2) IC_GGL((k_rotate_czt<true, false>), grid, block, shm, st, a, L, radices, nst);
        else IC_GGL((k_rotate_czt<false, false>), grid, block, shm, st, a, L, radices, nst);
    }
    return hipGetLastError();
}

bool rotate_stats_supported(int nbin, bool data_f64) { return nbin == 1024 && !data_f64; }

// The identity "rotation" of an archive stored dedispersed (its dedisperse is a
// no-op, archive.py dedisperse): out[p] = f32(in[p] - base[p]) (and out2), for
// the subints flags selects; a wave per profile, 16-byte rows (4-byte accesses
// where nbin or a stride is no multiple of 4: the chirp-z lengths).
__global__ __launch_bounds__(256) void k_rotate_identity(RotateArgs a)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t P = (size_t)a.nsub * a.nchan;
    for (size_t p = (size_t)blockIdx.x * 4 + wave; p < P; p += (size_t)gridDim.x * 4) {
        if (a.flags && a.flags[p / (unsigned)a.nchan] == 0) continue;
        const float b = a.base ? a.base[p] : 0.0f;
        if ((a.nbin | a.ld_in | a.ldo | a.ldo2) & 3) {   // a chirp-z length: rows of any alignment
            for (int j = lane; j < a.nbin; j += 64) {
                const float y = a.in[d_ofs(p, j, (int)a.ld_in, a.in_tiled)] - b;
                a.out[p * (size_t)a.ldo + j] = y;
                if (a.out2) a.out2[d_ofs(p, j, (int)a.ldo2, a.out2_tiled)] = y;
            }
            continue;
        }
        for (int j = 4 * lane; j < a.nbin; j += 256) {
            const float4 x = *(const float4 *)(a.in + d_ofs(p, j, (int)a.ld_in, a.in_tiled));
            const float4 y = make_float4(x.x - b, x.y - b, x.z - b, x.w - b);
            *(float4 *)(a.out + p * (size_t)a.ldo + j) = y;
            if (a.out2) *(float4 *)(a.out2 + d_ofs(p, j, (int)a.ldo2, a.out2_tiled)) = y;
        }
    }
}

// k_rotate<NN>: the per-channel or per-profile (delay2) form, ST with the fused statistics
template <int NN, bool ST>
static void rotate_p2(hipStream_t st, const RotateArgs &a, size_t P)
{
    using C = RotCfg<NN>;
    const dim3 grid(cap_grid(std::min<size_t>(cdiv(P, C::WPB), 16384 / C::WPB), a.grid_cap)), block(C::TB * C::WPB);
    if (a.delay2) IC_GGL((k_rotate<NN, true, ST>), grid, block, 0, st, a);
    else IC_GGL((k_rotate<NN, false, ST>), grid, block, 0, st, a);
}

hipError_t launch_rotate(hipStream_t st, const RotateArgs &a)
{
    const size_t P = (size_t)a.nsub * a.nchan;
    if (P == 0) return hipSuccess;
    const bool stats = a.std_o != nullptr;
    if (stats && (!rotate_stats_supported(a.nbin, false) || !a.amp || a.sign > 0 || a.out2 || !a.w0 || !a.mean_o ||
                  !a.ptp_o || !a.fft_o))
        return hipErrorInvalidValue;
    const bool mr = mr_supported(a.nbin);
    // the chirp-z lengths: opted in by their tables; rows of any stride (4-byte accesses)
    const bool czt = a.czt && czt_supported(a.nbin);
    const int ldm = czt ? 0 : 3;
    if ((!rotate_supported(a.nbin) && !czt) || !a.in || (!a.out && !stats) || (!czt && !a.tw) ||
        (!mr && !czt && !a.tw_p2) || a.ld_in < a.nbin ||
        (!stats && a.ldo < a.nbin) ||
        (!a.ph && !a.delay2 && !a.identity) ||
        (a.ld_in & ldm) || (a.ldo & ldm) || (a.out2 && (a.ldo2 < a.nbin || (a.ldo2 & ldm))) ||
        (a.amp && (!a.T64 || !a.info)) || (a.in_tiled && (a.ld_in & 31)) || (a.out2_tiled && (a.ldo2 & 31)) ||
        (a.identity && (a.amp || a.late || a.list)) || (a.list && !a.nctr))
        return hipErrorInvalidValue;
    if (a.identity) {
        const unsigned grid = cap_grid(std::min<size_t>(cdiv(P, 4), 16384), a.grid_cap);
        IC_GGL(k_rotate_identity, dim3(grid), dim3(256), 0, st, a);
        return hipGetLastError();
    }
    if (mr) return launch_rotate_mr(st, a, P);
    if (czt) return launch_rotate_czt(st, a, P);
    if (stats) {   // nbin 1024 (rotate_stats_supported)
        rotate_p2<1024, true>(st, a, P);
        return hipGetLastError();
    }
#define IC_ROT(NN)                                                                                 \
    case NN: rotate_p2<NN, false>(st, a, P); break;
    switch (a.nbin) {
        IC_P2_SIZES(IC_ROT)
    default: return hipErrorInvalidValue;
    }
#undef IC_ROT
    return hipGetLastError();
}

}  // namespace icgpu
