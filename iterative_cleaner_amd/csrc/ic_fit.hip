// ic_fit.hip -- the exact fit: scipy leastsq(a*T-p, [1.0]) per profile
// (ic.py:278) as MINPACK's lmdif, split into a state machine and data sweeps,
// with its launchers.  The non-inlined lm_* / lmpar1 / qrsolv1 live here with
// all their callers (k_fit_state, k_fit_tail, fit_transition).
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see Makefile).
// -ffp-contract=off is load-bearing: every f64/f32 operation below must be an
// individually rounded IEEE op in the order written, so that results equal
// numpy / scipy (MINPACK) bit-for-bit.  Explicit fma() is never used on an
// exact path.
//
// Kernels (per cleaning iteration, in launch order):
//   k_fit_init       per-profile lmdif state at x = 1, round counters zeroed
//   k_fit_prep       the first outer iteration's profile-independent qrfac
//   k_fit_pass       one data sweep (A: norms, B: dot) per requesting profile
//   k_fit_state      the lmdif step between two sweeps; writes the next list
//   k_mark_list      flags the profiles of a round list
//   k_fit_tail       the last few thousand profiles, one wave each, to the end
#include <algorithm>
#include <float.h>
#include <math.h>

#include "ic_wave.h"

namespace icgpu {

__device__ constexpr double kRdwarf = 3.834e-20;
__device__ constexpr double kRgiant = 1.304e19;

// ============================================================ exact lmdif

struct Enorm {
    double s1, s2, s3, x1max, x3max;
};

__device__ __forceinline__ void en_zero(Enorm &e) { e.s1 = e.s2 = e.s3 = e.x1max = e.x3max = 0.0; }

// MINPACK enorm, one component (rare branches kept exactly).
__device__ __forceinline__ void en_add(Enorm &e, double v, double agiant)
{
    const double xabs = fabs(v);
    if (xabs > kRdwarf && xabs < agiant) {
        e.s2 += xabs * xabs;
    } else if (xabs <= kRdwarf) {
        if (xabs > e.x3max) {
            const double t = e.x3max / xabs;
            e.s3 = 1.0 + e.s3 * (t * t);
            e.x3max = xabs;
        } else if (xabs != 0.0) {
            const double t = xabs / e.x3max;
            e.s3 += t * t;
        }
    } else {
        if (xabs > e.x1max) {
            const double t = e.x1max / xabs;
            e.s1 = 1.0 + e.s1 * (t * t);
            e.x1max = xabs;
        } else {
            const double t = xabs / e.x1max;
            e.s1 += t * t;
        }
    }
}

__device__ __forceinline__ double en_fin(const Enorm &e)
{
    if (e.s1 != 0.0) return e.x1max * sqrt(e.s1 + (e.s2 / e.x1max) / e.x1max);
    if (e.s2 != 0.0) {
        if (e.s2 >= e.x3max) return sqrt(e.s2 * (1.0 + (e.x3max / e.s2) * (e.x3max * e.s3)));
        return sqrt(e.x3max * ((e.s2 / e.x3max) + (e.x3max * e.s3)));
    }
    return e.x3max * sqrt(e.s3);
}

__device__ __forceinline__ double enorm1(double v)
{
    Enorm e;
    en_zero(e);
    en_add(e, v, kRgiant);
    return en_fin(e);
}

__device__ __forceinline__ double dmax_(double a, double b) { return a >= b ? a : b; }
__device__ __forceinline__ double dmin_(double a, double b) { return a <= b ? a : b; }

// MINPACK qrsolv, n = 1
__device__ double qrsolv1(double r, double w, double qtb, double *sdiag)
{
    double rr = r, wa = qtb;
    if (w != 0.0) {
        const double sd = w;
        const double qtbpj = 0.0;
        double cs, sn;
        if (fabs(rr) >= fabs(sd)) {
            const double tn = sd / rr;
            cs = 0.5 / sqrt(0.25 + 0.25 * (tn * tn));
            sn = cs * tn;
        } else {
            const double ct = rr / sd;
            sn = 0.5 / sqrt(0.25 + 0.25 * (ct * ct));
            cs = sn * ct;
        }
        rr = cs * rr + sn * sd;
        const double t1 = cs * wa;
        const double t2 = sn * qtbpj;
        wa = t1 + t2;
    }
    *sdiag = rr;
    if (rr == 0.0) return 0.0;
    const double sum = 0.0;
    return (wa - sum) / rr;
}

// MINPACK lmpar, n = 1
__device__ double lmpar1(double r, double diag, double qtb, double delta, double *par_io)
{
    const double p1 = 0.1, p001 = 0.001, dwarf = DBL_MIN;
    double par = *par_io;
    const int nsing = (r == 0.0) ? 0 : 1;
    double wa1 = qtb;
    if (nsing < 1) wa1 = 0.0;
    if (nsing >= 1) wa1 = wa1 / r;
    double x = wa1;
    int iter = 0;
    double wa2 = diag * x;
    double dxnorm = enorm1(wa2);
    double fp = dxnorm - delta;
    if (!(fp <= p1 * delta)) {
        double parl = 0.0;
        if (nsing >= 1) {
            double t = diag * (wa2 / dxnorm);
            const double sum = 0.0;
            t = (t - sum) / r;
            const double temp = enorm1(t);
            parl = ((fp / delta) / temp) / temp;
        }
        double sum = 0.0;
        sum += r * qtb;
        const double g = sum / diag;
        const double gnorm = enorm1(g);
        double paru = gnorm / delta;
        if (paru == 0.0) paru = dwarf / dmin_(delta, p1);
        par = dmax_(par, parl);
        par = dmin_(par, paru);
        if (par == 0.0) par = gnorm / dxnorm;
        for (;;) {
            ++iter;
            if (par == 0.0) par = dmax_(dwarf, p001 * paru);
            double temp = sqrt(par);
            const double w = temp * diag;
            double sdiag;
            x = qrsolv1(r, w, qtb, &sdiag);
            wa2 = diag * x;
            dxnorm = enorm1(wa2);
            temp = fp;
            fp = dxnorm - delta;
            if (fabs(fp) <= p1 * delta || (parl == 0.0 && fp <= temp && temp < 0.0) || iter == 10) break;
            double t = diag * (wa2 / dxnorm);
            t = t / sdiag;
            const double tn = enorm1(t);
            const double parc = ((fp / delta) / tn) / tn;
            if (fp > 0.0) parl = dmax_(parl, par);
            if (fp < 0.0) paru = dmin_(paru, par);
            par = dmax_(parl, par + parc);
        }
    }
    if (iter == 0) par = 0.0;
    *par_io = par;
    return x;
}

enum FitState { ST_A0 = 0, ST_A2 = 1, ST_B = 2, ST_DONE = 3 };

// Per-lane lmdif state (scipy leastsq, n = 1, m = nbin).
struct LmState {
    double x, fnorm, par, delta, diag, xnorm;
    double acnorm, J0, f0;       // Jacobian norm, J[0], fvec[0] at x
    double acn2, J02, f02;       // the same at x2 (speculative Jacobian)
    double aj, r, Jn0, qtf;
    double gnorm, x2, pnorm, wa1;
    int iter, nfev, info;
};

__device__ int lm_start_inner(LmState &L)
{
    const double step = lmpar1(L.r, L.diag, L.qtf, L.delta, &L.par);
    L.wa1 = -step;
    L.x2 = L.x + L.wa1;
    L.pnorm = enorm1(L.diag * L.wa1);
    if (L.iter == 1) L.delta = dmin_(L.delta, L.pnorm);
    return ST_A2;
}

__device__ int lm_after_qtf(LmState &L)
{
    L.gnorm = 0.0;
    if (L.fnorm != 0.0 && L.acnorm != 0.0) {
        double sum = 0.0;
        sum += L.r * (L.qtf / L.fnorm);
        // scipy's MINPACK keeps gnorm = 0 when the term is NaN (a non-finite
        // profile): info 4 at once, x = 1 (probed against scipy 1.15.3;
        // tests/golden/leastsq_nonfinite.npz)
        const double g = fabs(sum / L.acnorm);
        if (g > L.gnorm) L.gnorm = g;
    }
    if (L.gnorm <= 0.0) {  // gtol = 0
        L.info = 4;
        return ST_DONE;
    }
    L.diag = dmax_(L.diag, L.acnorm);
    return lm_start_inner(L);
}

// start of an outer iteration: fdjac2 done (acnorm, J0, f0 at x); qrfac + qtf setup
__device__ int lm_outer(LmState &L)
{
    L.nfev += 1;
    double ajnorm = L.acnorm;
    L.Jn0 = L.J0;
    if (ajnorm != 0.0) {
        if (L.J0 < 0.0) ajnorm = -ajnorm;
        L.Jn0 = L.J0 / ajnorm;
        L.Jn0 = L.Jn0 + 1.0;
    }
    L.aj = ajnorm;
    L.r = -ajnorm;
    if (L.iter == 1) {
        L.diag = L.acnorm;
        if (L.diag == 0.0) L.diag = 1.0;
        L.xnorm = enorm1(L.diag * L.x);
        L.delta = 100.0 * L.xnorm;
        if (L.delta == 0.0) L.delta = 100.0;
    }
    if (L.Jn0 != 0.0) return ST_B;  // needs sum_i Jn_i * fvec_i
    L.qtf = L.f0;
    return lm_after_qtf(L);
}

__device__ int lm_after_b(LmState &L, double sum)
{
    const double t = -sum / L.Jn0;
    L.qtf = L.f0 + L.Jn0 * t;
    return lm_after_qtf(L);
}

__device__ int lm_after_a2(LmState &L, double fnorm1, bool *accepted = nullptr)
{
    const double ftol = 1.49012e-8, xtol = 1.49012e-8, epsmch = DBL_EPSILON;
    L.nfev += 1;
    double actred = -1.0;
    if (0.1 * fnorm1 < L.fnorm) {
        const double t = fnorm1 / L.fnorm;
        actred = 1.0 - t * t;
    }
    double w3 = 0.0;
    w3 += L.r * L.wa1;
    const double temp1 = enorm1(w3) / L.fnorm;
    const double temp2 = (sqrt(L.par) * L.pnorm) / L.fnorm;
    const double prered = temp1 * temp1 + temp2 * temp2 / 0.5;
    const double dirder = -(temp1 * temp1 + temp2 * temp2);
    double ratio = 0.0;
    if (prered != 0.0) ratio = actred / prered;
    if (ratio <= 0.25) {
        double tt = 0.0;
        if (actred >= 0.0) tt = 0.5;
        if (actred < 0.0) tt = 0.5 * dirder / (dirder + 0.5 * actred);
        if (0.1 * fnorm1 >= L.fnorm || tt < 0.1) tt = 0.1;
        L.delta = tt * dmin_(L.delta, L.pnorm / 0.1);
        L.par = L.par / tt;
    } else if (L.par == 0.0 || ratio >= 0.75) {
        L.delta = L.pnorm / 0.5;
        L.par = 0.5 * L.par;
    }
    if (accepted) *accepted = ratio >= 1e-4;
    if (ratio >= 1e-4) {
        L.x = L.x2;
        L.xnorm = enorm1(L.diag * L.x);
        L.fnorm = fnorm1;
        L.iter += 1;
        L.acnorm = L.acn2;
        L.J0 = L.J02;
        L.f0 = L.f02;
    }
    int info = 0;
    if (fabs(actred) <= ftol && prered <= ftol && 0.5 * ratio <= 1.0) info = 1;
    if (L.delta <= xtol * L.xnorm) info = 2;
    if (fabs(actred) <= ftol && prered <= ftol && 0.5 * ratio <= 1.0 && info == 2) info = 3;
    if (info == 0) {
        if (L.nfev >= 400) info = 5;
        if (fabs(actred) <= epsmch && prered <= epsmch && 0.5 * ratio <= 1.0) info = 6;
        if (L.delta <= epsmch * L.xnorm) info = 7;
        if (L.gnorm <= epsmch) info = 8;
    }
    if (info != 0) {
        L.info = info;
        return ST_DONE;
    }
    if (ratio < 1e-4) return lm_start_inner(L);
    return lm_outer(L);
}

// Exact fast path.  enorm: while every component is 0 or inside
// (RDWARF, agiant) MINPACK's enorm reduces to sqrt(sum_seq a*a).  The range is
// verified per lane without per-sample work after the first 32 samples:
//  * upper: the sequential sum of the nonnegative squares bounds every square
//    (RN is monotone), so hi(RN(s2)) < hi(RN(agiant^2)) at the end implies
//    |a| < agiant for every component (NaN/Inf fail the compare);
//  * lower: over the first 32 samples (the peeled first tile pair) every
//    nonzero square is checked, hi(RN(a^2)) > hi(RN(RDWARF^2)) implies
//    |a| > RDWARF (equal high words count as out of range); after them the
//    running sum must be >= 2^-40.  A later component with |a| <= RDWARF then
//    adds RN(a^2) <= 2^-129 < ulp(s2)/2 to s2, a no-op, exactly as MINPACK
//    leaves it out of s2; MINPACK's final factor 1 + (x3max/s2)(x3max s3) <=
//    1 + n RDWARF^2 / 2^-40 rounds to 1 for any n < 2^50, and s2 >= x3max, so
//    its result is sqrt(s2) as well.
// A nonzero a whose square underflowed to 0 would slip through the first-tile
// check, so the A sweep takes this path only for |x| in [2^-100, 2^100]:
// there every nonzero f = RN(RN(x t) - p) (t, p from f32) is >= 2^-301 and
// every nonzero J >= 2^-427 in magnitude, |J| <= 2^355, and all squares are
// normal.  Division q = RN(a/b): y = RN(1/b) and ylo = RN((1 - b y) y) (1 - b y
// is exact) approximate 1/b to 2^-105 relative, so q0 = RN(a y + RN(a ylo)) is
// within 2^-104 |a/b| + ulp/2, i.e. faithful, and one Markstein correction
// q = RN(q0 + RN(a - b q0) y) (the remainder exact) is RN(a/b), barring
// over/underflow — which would push J out of the verified enorm range and send
// the lane to the exact pass.
struct FastAcc {
    double s2;
    uint32_t minhm1;
};

__device__ __forceinline__ void fa_zero(FastAcc &a)
{
    a.s2 = 0.0;
    a.minhm1 = 0xffffffffu;
}

template <bool CHK>
__device__ __forceinline__ void fa_add(FastAcc &a, double v)
{
    const double sq = v * v;   // == RN(|v| * |v|)
    a.s2 = a.s2 + sq;
    if (CHK) {
        const uint32_t hi = (uint32_t)((unsigned long long)__double_as_longlong(sq) >> 32);
        a.minhm1 = min(a.minhm1, hi - 1u);   // zero -> 0xffffffff
    }
}

// after the checked samples: no nonzero square at or below RDWARF^2, and the
// running sum large enough to absorb any later one
__device__ __forceinline__ bool fa_lo_ok(const FastAcc &a, uint32_t hr1)
{
    return ((a.minhm1 == 0xffffffffu) || (a.minhm1 + 1u >= hr1)) && a.s2 >= 0x1p-40;
}

__device__ __forceinline__ bool fa_hi_ok(const FastAcc &a, uint32_t hg)
{
    return (uint32_t)((unsigned long long)__double_as_longlong(a.s2) >> 32) < hg;
}

__device__ __forceinline__ double fa_fin(const FastAcc &a) { return a.s2 != 0.0 ? sqrt(a.s2) : 0.0; }

// low part of 1/b given y = RN(1/b)
__device__ __forceinline__ double recip_lo(double b, double y) { return fma(-b, y, 1.0) * y; }

__device__ __forceinline__ double mdiv(double a, double b, double y, double ylo)
{
    const double q0 = fma(a, y, a * ylo);
    const double r0 = fma(-b, q0, a);
    return fma(r0, y, q0);
}

__device__ __forceinline__ bool x_in_fast_range(double x)
{
    const double ax = fabs(x);
    return ax >= 0x1p-500 && ax <= 0x1p500;
}

// the A sweep's squared-high-word range check (see fa_add) needs the tighter range
__device__ __forceinline__ bool x_in_sq_range(double x)
{
    const double ax = fabs(x);
    return ax >= 0x1p-100 && ax <= 0x1p100;
}

// ---- data movement of a sweep: LDS-DMA, double buffered ----------------------
// A wave owns 64 profiles (one per lane) and streams their rows of D through
// two 4-KiB LDS buffers, 16 bins per tile, with global_load_lds_dwordx4: the
// next tile is in flight while the current one is consumed, and no VGPRs hold
// it on the way.  A DMA writes 1 KiB lane-linearly (slot = lane), so the
// transpose to "lane p reads its own profile" is done on the SOURCE side:
// instruction m, lane l fetches chunk c = (l&3) ^ ((l>>4)&3) (4 bins) of
// profile 16m + l/4.  Profile p's chunk c then sits in slot
// 64(p>>4) + 4(p&15) + (c ^ ((p>>2)&3)), and the ds_read_b128 of one chunk by
// all 64 lanes hits 16 distinct 16-B slots in each 16-lane bank group.
// D is padded to [roundup(P,64)][ldD], ldD a multiple of 32: no guards.
#define FIT_TB 16
#define FIT_BUF 4096

struct DmaTiles {
    const float *src[4];   // this lane's DMA source for instruction m at bin 0
    int tiled;             // fit cube layout (dt_ofs): bin b0 of a row is at + (b0/32) 2048 + b0 % 32
    uint32_t rd[4];        // LDS byte address of this lane's chunk c in buffer 0
    char *lds;             // buffer 0 (buffer 1 at +FIT_BUF)
};

__device__ __forceinline__ void dma_tile(const DmaTiles &d, char *buf, int b0)
{
    const int off = d.tiled ? ((b0 >> 5) << 11) + (b0 & 31) : b0;
#pragma unroll
    for (int m = 0; m < 4; ++m)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(d.src[m] + off),
                                         (__attribute__((address_space(3))) void *)(buf + m * 1024), 16, 0,
                                         0);   // default cache policy (nt: 15.7 -> 18.8 ms per C2 clean)
}

// ds_read in asm: the compiler would otherwise order every LDS read behind a
// vmcnt(0) for the DMAs, draining the prefetch.  Ordering against the DMA is
// the explicit counted vmcnt in sweep_dma; the lgkmcnt wait ties the values.
template <int OFF>
__device__ __forceinline__ void read_tile(const DmaTiles &d, fv4 (&v)[4])
{
#pragma unroll
    for (int c = 0; c < 4; ++c) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v[c]) : "v"(d.rd[c]), "i"(OFF));
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]));
}

// one pair of tiles (t, t + 1) = one 128-B line of each of the wave's 64 rows;
// CHK: the body runs its per-sample range checks.  Both halves of the next line
// are requested together, right after tile t + 1 has been read into registers
// (a half line requested alone is refetched when the L2 drops the line in
// between: measured 1.2 % faster than refilling each buffer as soon as it is
// read).  The ds_reads complete before the DMA that overwrites their buffer is
// issued (read_tile waits on lgkmcnt, and the memory clobber keeps the compiler
// from hoisting the DMA above them).
template <bool CHK, typename Body>
__device__ __forceinline__ void sweep_pair(const DmaTiles &d, int t, int nt, Body &body)
{
    fv4 v[4];
    body.load_T(t * FIT_TB);   // scalar loads issued ahead of the waits
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // tiles t and t + 1 landed
    read_tile<0>(d, v);
    body.template run<CHK>(t * FIT_TB, v);
    body.fence();   // keep tile t's arithmetic ahead of the DMA issue below
    body.load_T((t + 1) * FIT_TB);
    read_tile<FIT_BUF>(d, v);
    asm volatile("" ::: "memory");
    if (t + 2 < nt) {
        dma_tile(d, d.lds, (t + 2) * FIT_TB);
        dma_tile(d, d.lds + FIT_BUF, (t + 3) * FIT_TB);
    }
    body.template run<CHK>((t + 1) * FIT_TB, v);
    body.fence();
}

// Body::kPeel: the first pair (32 samples) is peeled with the checks on, then
// body.checked().  issued: the first tile pair's DMA is already in flight
// (k_fit_pass issues it before it loads the lanes' lmdif state)
template <typename Body>
__device__ __forceinline__ void sweep_dma(const DmaTiles &d, int ldD, Body &body, bool issued = false)
{
    const int nt = ldD / FIT_TB;   // even, >= 2
    if (!issued) {
        dma_tile(d, d.lds, 0);
        dma_tile(d, d.lds + FIT_BUF, FIT_TB);
    }
    int t = 0;
    if constexpr (Body::kPeel) {
        sweep_pair<true>(d, 0, nt, body);
        body.checked();
        t = 2;
    }
    for (; t < nt; t += 2) sweep_pair<false>(d, t, nt, body);
}

struct PassIn {
    bool A, B;                   // lane takes part in pass A / B
    double xa, xha, ha, yha, yla;  // A: f(xa) and J(xa)
    double xb, xhb, hb, yhb, ylb, ajb, yaj, ylj;  // B: sum Jn*f at xb
};

struct PassOut {
    double fnorm, acnorm, sum;
    float p0;                    // the profile's first sample (round 0: k_fit_state's f0 / J0)
    bool bad;                    // fast path left its verified range
    bool jt;                     // FUSE: J(1) == T, sum is qtf's dot
};

// Fast sweep body: straight-line over a 16-bin tile, wave-uniform predicates
// only (lanes that did not request the sweep compute on defaults; their
// results are discarded).  Zero-padded samples (p = 0, T = 0) are exact
// no-ops: f = J = 0 adds nothing to either norm, and Jn*f = 0 to the dot.
// FUSE (round 0: DA at x = 1 for every lane, k_fit_init): the A sweep at
// x = 1 specialised (1 t = t; h = 2^-26, so J = RN(d / h) = d 2^26 exactly,
// which is what mdiv gives), plus the dot of the B sweep that would follow,
// sum_i RN(Jn_i f_i) with Jn_i = RN(J_i / aj) (+1 at i = 0) and the shared aj
// of k_fit_prep, and jt = (J_i == T_i for every i): when that holds, and the
// profile's own qrfac is k_fit_prep's, the dot is the B sweep's own.
template <bool DA, bool DB, bool FUSE = false>
struct FastBody {
    static constexpr bool kPeel = true;
    const PassIn &in;
    const double *__restrict__ T64;
    FastAcc fF, fJ;
    double sum, fsum;
    float p00;   // FUSE: the first sample
    int lo_ok;
    bool jt;

    __device__ __forceinline__ FastBody(const PassIn &i, const double *T) : in(i), T64(T)
    {
        fa_zero(fF);
        fa_zero(fJ);
        sum = fsum = 0.0;
        p00 = 0.0f;
        lo_ok = 1;
        jt = true;
    }

    // the flag is materialised here (empty asm): otherwise the compiler sinks
    // the per-sample minima below the sweep loop and keeps the squares live
    __device__ __forceinline__ void checked()
    {
        if (DA) {
            const uint32_t hr1 = (uint32_t)((unsigned long long)__double_as_longlong(kRdwarf * kRdwarf) >> 32) + 1u;
            lo_ok = (fa_lo_ok(fF, hr1) && fa_lo_ok(fJ, hr1)) ? 1 : 0;
            asm volatile("" : "+v"(lo_ok));
        }
    }

    // empty asm on the accumulators: the compiler may not sink a tile's
    // arithmetic below the following s_waitcnt (asm statements keep their order)
    __device__ __forceinline__ void fence()
    {
        asm volatile("" : "+v"(fF.s2), "+v"(fJ.s2), "+v"(sum), "+v"(fF.minhm1), "+v"(fJ.minhm1));
        if (FUSE) asm volatile("" : "+v"(fsum));
    }

    double tv[FIT_TB];   // the tile's template values (wave-uniform: SGPRs)
    __device__ __forceinline__ void load_T(int b0)
    {
#pragma unroll
        for (int i = 0; i < FIT_TB; ++i) tv[i] = T64[b0 + i];
    }

    // Four samples at a time, stage by stage: the four dependent chains (the
    // products, the differences, the four-step divisions) are interleaved so
    // that every f64 op has independent neighbours to hide its latency behind;
    // the accumulations still run in sample order.  Per sample: A = f(x),
    // f(x + h), J = RN((f(x + h) - f(x))/h), f^2 and J^2 summed; B = the same f
    // and J, Jn = RN(J/ajnorm) (+1 on sample 0), sum += Jn f.
    template <bool CHK>
    __device__ __forceinline__ void group4(const double (&t)[4], const fv4 &pv4, bool first)
    {
        const float pf[4] = {pv4.x, pv4.y, pv4.z, pv4.w};
        double p[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) p[k] = (double)pf[k];
        if (DA && FUSE) {
            // x = 1: f = RN(t - p), d = RN(RN((1 + 2^-26) t) - p) - f, J = d 2^26
            constexpr double xh1 = 1.0 + 0x1p-26;
            double f[4], d[4], q[4], r[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) d[k] = xh1 * t[k];
#pragma unroll
            for (int k = 0; k < 4; ++k) f[k] = t[k] - p[k];
#pragma unroll
            for (int k = 0; k < 4; ++k) d[k] = d[k] - p[k];
#pragma unroll
            for (int k = 0; k < 4; ++k) d[k] = d[k] - f[k];
#pragma unroll
            for (int k = 0; k < 4; ++k) q[k] = d[k] * 0x1p26;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                fa_add<CHK>(fF, f[k]);
                fa_add<CHK>(fJ, q[k]);
            }
            if (first) p00 = pf[0];
            // Jn = mdiv(J, aj, yaj, ylj) (the B sweep's), dot in sample order
#pragma unroll
            for (int k = 0; k < 4; ++k) d[k] = q[k] * in.ylj;
#pragma unroll
            for (int k = 0; k < 4; ++k) d[k] = fma(q[k], in.yaj, d[k]);
#pragma unroll
            for (int k = 0; k < 4; ++k) r[k] = fma(-in.ajb, d[k], q[k]);
#pragma unroll
            for (int k = 0; k < 4; ++k) d[k] = fma(r[k], in.yaj, d[k]);
            if (first) d[0] = d[0] + 1.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                jt = jt && (q[k] == t[k]);
                d[k] = d[k] * f[k];
                fsum = fsum + d[k];
            }
        } else if (DA) {
            double f[4], d[4], q[4], r[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) f[k] = in.xa * t[k];
#pragma unroll
            for (int k = 0; k < 4; ++k) d[k] = in.xha * t[k];
#pragma unroll
            for (int k = 0; k < 4; ++k) f[k] = f[k] - p[k];
#pragma unroll
            for (int k = 0; k < 4; ++k) d[k] = d[k] - p[k];
#pragma unroll
            for (int k = 0; k < 4; ++k) d[k] = d[k] - f[k];
            // J = mdiv(d, ha, yha, yla), stage-interleaved
#pragma unroll
            for (int k = 0; k < 4; ++k) q[k] = d[k] * in.yla;
#pragma unroll
            for (int k = 0; k < 4; ++k) q[k] = fma(d[k], in.yha, q[k]);
#pragma unroll
            for (int k = 0; k < 4; ++k) r[k] = fma(-in.ha, q[k], d[k]);
#pragma unroll
            for (int k = 0; k < 4; ++k) q[k] = fma(r[k], in.yha, q[k]);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                fa_add<CHK>(fF, f[k]);
                fa_add<CHK>(fJ, q[k]);
            }
        }
        if (DB) {
            double f[4], d[4], q[4], r[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) f[k] = in.xb * t[k];
#pragma unroll
            for (int k = 0; k < 4; ++k) d[k] = in.xhb * t[k];
#pragma unroll
            for (int k = 0; k < 4; ++k) f[k] = f[k] - p[k];
#pragma unroll
            for (int k = 0; k < 4; ++k) d[k] = d[k] - p[k];
#pragma unroll
            for (int k = 0; k < 4; ++k) d[k] = d[k] - f[k];
            // J = mdiv(d, hb, yhb, ylb)
#pragma unroll
            for (int k = 0; k < 4; ++k) q[k] = d[k] * in.ylb;
#pragma unroll
            for (int k = 0; k < 4; ++k) q[k] = fma(d[k], in.yhb, q[k]);
#pragma unroll
            for (int k = 0; k < 4; ++k) r[k] = fma(-in.hb, q[k], d[k]);
#pragma unroll
            for (int k = 0; k < 4; ++k) q[k] = fma(r[k], in.yhb, q[k]);
            // Jn = mdiv(J, ajb, yaj, ylj)
#pragma unroll
            for (int k = 0; k < 4; ++k) d[k] = q[k] * in.ylj;
#pragma unroll
            for (int k = 0; k < 4; ++k) d[k] = fma(q[k], in.yaj, d[k]);
#pragma unroll
            for (int k = 0; k < 4; ++k) r[k] = fma(-in.ajb, d[k], q[k]);
#pragma unroll
            for (int k = 0; k < 4; ++k) d[k] = fma(r[k], in.yaj, d[k]);
            if (first) d[0] = d[0] + 1.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) d[k] = d[k] * f[k];
#pragma unroll
            for (int k = 0; k < 4; ++k) sum = sum + d[k];
        }
    }

    template <bool CHK>
    __device__ __forceinline__ void run(int b0, const fv4 (&v)[4])
    {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const double t4[4] = {tv[4 * c], tv[4 * c + 1], tv[4 * c + 2], tv[4 * c + 3]};
            group4<CHK>(t4, v[c], CHK && c == 0 && b0 == 0);
        }
    }
};

// Exact sweep body: MINPACK's branchy enorm and true divisions, per lane.
struct ExactBody {
    static constexpr bool kPeel = false;
    const PassIn &in;
    const double *__restrict__ T64;
    double agiant;
    Enorm eF, eJ;
    double sum;
    float p00;   // the first sample

    __device__ __forceinline__ ExactBody(const PassIn &i, const double *T, double ag) : in(i), T64(T), agiant(ag)
    {
        en_zero(eF);
        en_zero(eJ);
        sum = 0.0;
        p00 = 0.0f;
    }

    __device__ void sample(double t, double pv, bool first)
    {
        if (in.A) {
            const double u = in.xa * t;
            const double f = u - pv;
            const double uh = in.xha * t;
            const double wa = uh - pv;
            const double d = wa - f;
            en_add(eF, f, agiant);
            const double J = d / in.ha;
            en_add(eJ, J, agiant);
            if (first) p00 = (float)pv;
        }
        if (in.B) {
            const double u = in.xb * t;
            const double f = u - pv;
            const double uh = in.xhb * t;
            const double wa = uh - pv;
            const double d = wa - f;
            const double J = d / in.hb;
            double Jn = J / in.ajb;
            if (first) Jn = Jn + 1.0;
            const double pr = Jn * f;
            sum = sum + pr;
        }
    }

    __device__ __forceinline__ void fence() {}
    __device__ __forceinline__ void load_T(int) {}
    template <bool CHK>
    __device__ void run(int b0, const fv4 (&v)[4])
    {
        for (int c = 0; c < 4; ++c) {
            const int i = b0 + 4 * c;
            sample(T64[i], (double)v[c].x, i == 0);
            sample(T64[i + 1], (double)v[c].y, false);
            sample(T64[i + 2], (double)v[c].z, false);
            sample(T64[i + 3], (double)v[c].w, false);
        }
    }
};

template <bool DA, bool DB, bool FUSE = false>
__device__ __forceinline__ void fast_sweep(const DmaTiles &d, int ldD, const PassIn &in,
                                           const double *__restrict__ T64, double agiant, PassOut &out,
                                           bool issued = false)
{
    FastBody<DA, DB, FUSE> body(in, T64);
    sweep_dma(d, ldD, body, issued);
    const uint32_t hg = (uint32_t)((unsigned long long)__double_as_longlong(agiant * agiant) >> 32);
    out.p0 = body.p00;
    out.sum = FUSE ? body.fsum : body.sum;
    out.fnorm = fa_fin(body.fF);
    out.acnorm = fa_fin(body.fJ);
    out.bad = DA && in.A && !(body.lo_ok && fa_hi_ok(body.fF, hg) && fa_hi_ok(body.fJ, hg));
    // the dot counts only where J stayed in the fast path's verified range (mdiv = RN division)
    out.jt = FUSE && body.jt && !out.bad;
}

// ---- split lmdif: state machine (k_fit_state) <-> data sweeps (k_fit_pass) ----
// Per-profile state lives in HBM as structure-of-arrays (FitState below);
// a round is one k_fit_pass (every profile with a pending request reads its
// samples once) followed by one k_fit_state (each lane consumes its sweep
// result and runs MINPACK's scalar logic up to its next data request).

__device__ __forceinline__ void lm_load(LmState &L, const FitStateArrays &S, long k)
{
    L.x = S.x[k]; L.fnorm = S.fnorm[k]; L.par = S.par[k]; L.delta = S.delta[k]; L.diag = S.diag[k];
    L.xnorm = S.xnorm[k]; L.acnorm = S.acnorm[k]; L.J0 = S.J0[k]; L.f0 = S.f0[k];
    L.aj = S.aj[k]; L.r = S.r[k]; L.Jn0 = S.Jn0[k]; L.qtf = S.qtf[k]; L.gnorm = S.gnorm[k];
    L.x2 = S.x2[k]; L.pnorm = S.pnorm[k]; L.wa1 = S.wa1[k];
    L.iter = S.iter[k]; L.nfev = S.nfev[k]; L.info = 0;
    L.acn2 = 0.0; L.J02 = 0.0; L.f02 = 0.0;
}

__device__ __forceinline__ void lm_store(const LmState &L, const FitStateArrays &S, long k)
{
    S.x[k] = L.x; S.fnorm[k] = L.fnorm; S.par[k] = L.par; S.delta[k] = L.delta; S.diag[k] = L.diag;
    S.xnorm[k] = L.xnorm; S.acnorm[k] = L.acnorm; S.J0[k] = L.J0; S.f0[k] = L.f0;
    S.aj[k] = L.aj; S.r[k] = L.r; S.Jn0[k] = L.Jn0; S.qtf[k] = L.qtf; S.gnorm[k] = L.gnorm;
    S.x2[k] = L.x2; S.pnorm[k] = L.pnorm; S.wa1[k] = L.wa1;
    S.iter[k] = L.iter; S.nfev[k] = L.nfev;
}

// m[k] = v for every profile k of a round list (the second fork: the profiles
// handed to k_fit_tail)
__global__ __launch_bounds__(256) void k_mark_list(const int32_t *__restrict__ list,
                                                   const unsigned long long *__restrict__ nctr, long P,
                                                   uint8_t *__restrict__ m, uint8_t v)
{
    const RoundList rl(list, nctr, P);
    const long slot = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (slot < rl.n()) m[rl.at(slot)] = v;
}

// request encoding in S.mode: ST_A0 / ST_A2 -> sweep A at S.xa; ST_B -> sweep B
// at (S.x, S.aj); ST_DONE -> nothing.  S.slow: J at x came from an exact sweep.
// also zeroes the round counters (nz32 words) and the late flags (P bytes, optional)
__global__ __launch_bounds__(256) void k_fit_init(FitStateArrays S, long P, int32_t *__restrict__ z32, int nz32,
                                                  uint8_t *__restrict__ late)
{
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < nz32) z32[k] = 0;
    if (k >= P) return;
    if (late) late[k] = 0;
    S.mode[k] = ST_A0;
    S.xa[k] = 1.0;
    S.x[k] = 1.0; S.par[k] = 0.0; S.iter[k] = 1; S.nfev[k] = 0; S.slow[k] = 0;
}

// The first outer iteration, at x = 1 for every profile, has a Jacobian that is
// the template itself: h = eps |x| = 2^-26 exactly, (1 + 2^-26) t is exact for
// an f32 t, and whenever RN(t - p) and RN(RN((1 + 2^-26) t) - p) are exact (t
// and p within ~2^29 of each other, or p = 0) the forward difference is
// (2^-26 t) / 2^-26 = t exactly.  Then enorm(J) (= acnorm = ajnorm), the sign,
// Jn_0 and qtf's weights Jn_i = RN(J_i / aj) are the same for every profile
// (lm_outer, MINPACK qrfac with n = 1), and the B sweep's dot
// sum_i RN(Jn_i f_i) can be summed in round 0 together with the A sweep, which
// has the same f_i: one full sweep of the fit cube less per iteration.  A
// profile whose J differs anywhere (k_fit_pass checks J_i == T_i), or whose
// own acnorm / aj / Jn0 differ, sends its B request as before.
// R0: the round-0 form (list == nullptr, every request A at x = 1), which sums
// the first B sweep's dot in the same sweep (k_fit_prep's U); a kernel of its
// own so that the other rounds keep their register allocation (and occupancy)
template <bool R0>
__global__ __launch_bounds__(64) void k_fit_pass(const float *__restrict__ D, const double *__restrict__ T64,
                                                 long P, int nbin, int ldD, int nsw, int dtiled,
                                                 const int32_t *__restrict__ list,
                                                 const unsigned long long *__restrict__ nctr, FitStateArrays S,
                                                 const double *__restrict__ U)
{
    __shared__ __attribute__((aligned(16))) char lbuf[2 * FIT_BUF];
    const int lane = threadIdx.x;
    const long slot = (long)blockIdx.x * 64 + lane;
    const RoundList rl(list, nctr, P);
    const long nact = rl.n();   // the grid is only an upper bound
    if ((long)blockIdx.x * 64 >= nact) return;
    DmaTiles dt;
    dt.lds = lbuf;
    dt.tiled = dtiled;
    {
        const int c = (lane & 3) ^ ((lane >> 4) & 3);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const long sl = (long)blockIdx.x * 64 + m * 16 + (lane >> 2);
            long kr = 0;   // empty slots read row 0 (valid: D is padded)
            if (sl < nact) kr = rl.at(sl);
            dt.src[m] = D + d_ofs(kr, 4 * c, ldD, dtiled);
        }
        const uint32_t base = lds_u32(lbuf) + 16u * (uint32_t)(64 * (lane >> 4) + 4 * (lane & 15));
        const int g = (lane >> 2) & 3;
#pragma unroll
        for (int c2 = 0; c2 < 4; ++c2) dt.rd[c2] = base + 16u * (uint32_t)(c2 ^ g);
    }
    // the first tile pair is requested from the list alone, before the lanes'
    // lmdif state is read: the state's dependent loads (list -> mode -> x, aj)
    // then overlap the pair's memory latency instead of preceding it
    dma_tile(dt, dt.lds, 0);
    dma_tile(dt, dt.lds + FIT_BUF, FIT_TB);
    const bool in_range = slot < nact;
    const long k = in_range ? rl.at(slot) : 0;
    const int st = in_range ? S.mode[k] : ST_DONE;
    const bool reqA = (st == ST_A0) || (st == ST_A2);
    const bool reqB = (st == ST_B);
    if (!__any(reqA || reqB)) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // no DMA may outlive the block's LDS
        return;
    }
    const double agiant = kRgiant / (double)nbin;
    const double eps = sqrt(DBL_EPSILON);
    PassIn in;
    in.xa = reqA ? S.xa[k] : 1.0;
    in.ha = eps * fabs(in.xa);
    if (in.ha == 0.0) in.ha = eps;
    in.xha = in.xa + in.ha;
    in.yha = 1.0 / in.ha;
    in.yla = recip_lo(in.ha, in.yha);
    in.xb = reqB ? S.x[k] : 1.0;
    in.hb = eps * fabs(in.xb);
    if (in.hb == 0.0) in.hb = eps;
    in.xhb = in.xb + in.hb;
    in.yhb = 1.0 / in.hb;
    in.ylb = recip_lo(in.hb, in.yhb);
    in.ajb = reqB ? S.aj[k] : 1.0;
    in.yaj = 1.0 / in.ajb;
    in.ylj = recip_lo(in.ajb, in.yaj);
    const bool slow = reqB && S.slow[k];
    const bool fastA = reqA && x_in_sq_range(in.xa);
    const bool fastB = reqB && !slow && x_in_fast_range(in.xb) && x_in_fast_range(in.ajb);
    in.A = fastA;
    in.B = fastB;
    PassOut o;
    o.bad = o.jt = false;
    o.fnorm = o.acnorm = o.sum = 0.0;
    o.p0 = 0.0f;
    const bool anyA = __any(fastA), anyB = __any(fastB);
    if constexpr (R0) {
        // every profile at x = 1: the first B sweep's dot rides along (k_fit_prep)
        // (the dot is summed even when k_fit_prep found no shared qrfac, U[0] == 0:
        // k_fit_state then ignores it)
        in.ajb = U[2];
        in.yaj = 1.0 / in.ajb;
        in.ylj = recip_lo(in.ajb, in.yaj);
        // uniform, but held in VGPRs: the sweep's scalars (a tile of template
        // values) already fill the SGPR file
        asm volatile("" : "+v"(in.ajb), "+v"(in.yaj), "+v"(in.ylj));
        if (anyA) fast_sweep<true, false, true>(dt, nsw, in, T64, agiant, o, true);
    } else {
        if (anyA && anyB)
            fast_sweep<true, true>(dt, nsw, in, T64, agiant, o, true);
        else if (anyA)
            fast_sweep<true, false>(dt, nsw, in, T64, agiant, o, true);
        else if (anyB)
            fast_sweep<false, true>(dt, nsw, in, T64, agiant, o, true);
    }
    const bool exA = reqA && (!fastA || o.bad);
    const bool exB = reqB && !fastB;
    if (__any(exA || exB)) {
        PassIn ie = in;
        ie.A = exA;
        ie.B = exB;
        ExactBody body(ie, T64, agiant);
        // the early tile pair is still pending when no fast sweep consumed it
        const bool fast_ran = R0 ? anyA : (anyA || anyB);
        sweep_dma(dt, nsw, body, !fast_ran);
        if (exA || exB) {
            if (exA) o.p0 = body.p00;
            o.sum = body.sum;
            o.fnorm = en_fin(body.eF);
            o.acnorm = en_fin(body.eJ);
        }
    }
    // The outputs, as few bytes as possible: written into the sweep's read
    // stream, a DRAM write costs ~10x its size (tools/ubench_sweep: five 8-B
    // fields per profile +90 us per 4.7-GB round, one +20 us).  The two norms
    // carry the flags in their sign bits (both are >= 0 or NaN, whose sign
    // nothing reads): exA on fnorm, jt on acnorm.  f0 and J0, the residual and
    // the Jacobian at sample 0, are recomputed by k_fit_state from the first
    // sample, which round 0 stores once (OutS::f0J0).
    if (reqA) {
        // both norms in one 16-B store (o_fnorm's and o_acnorm's arrays are
        // adjacent: read as one double2 array of P entries)
        ((double2 *)S.o_fnorm)[k] = make_double2(exA ? -fabs(o.fnorm) : fabs(o.fnorm),
                                                 o.jt ? -fabs(o.acnorm) : fabs(o.acnorm));
        if (o.jt) S.o_sum[k] = o.sum;
        if (R0) S.p0[k] = o.p0;
    }
    if (reqB) S.o_sum[k] = o.sum;
}

// One profile's MINPACK transition after its sweep (k_fit_state): request
// st, the sweep's results from o (OutS: k_fit_pass's o_* fields), the lmdif
// state read from and written to S; returns the next request (ST_DONE: amp /
// info written).
struct OutS {
    const FitStateArrays &S;
    long k;
    __device__ __forceinline__ double fnorm() const { return fabs(((const double2 *)S.o_fnorm)[k].x); }
    __device__ __forceinline__ double acnorm() const { return fabs(((const double2 *)S.o_fnorm)[k].y); }
    __device__ __forceinline__ double sum() const { return S.o_sum[k]; }
    // bit 0: the A sweep took the exact path; bit 1: J(1) == T (round 0)
    __device__ __forceinline__ int exact() const
    {
        const double2 n = ((const double2 *)S.o_fnorm)[k];
        return (signbit(n.x) ? 1 : 0) | (signbit(n.y) ? 2 : 0);
    }
    // the residual f0 and the Jacobian J0 at sample 0 of the A sweep at x: the
    // sweep's own operations on its first sample (ExactBody::sample; the fast
    // bodies' four-op division is RN(d / h) wherever their result is used, and
    // at x = 1 d 2^26 = d / 2^-26), from the first sample round 0 stored
    __device__ __forceinline__ void f0J0(double x, double &f0, double &J0) const
    {
        const double eps = sqrt(DBL_EPSILON);
        double h = eps * fabs(x);
        if (h == 0.0) h = eps;
        const double xh = x + h;
        const double t = S.T64[0], pv = (double)S.p0[k];
        const double u = x * t;
        const double f = u - pv;
        const double uh = xh * t;
        const double wa = uh - pv;
        const double d = wa - f;
        f0 = f;
        J0 = d / h;
    }
};
template <typename Out>
__device__ __forceinline__ int fit_transition(const FitStateArrays &S, long k, int st, const Out &o,
                                              double *__restrict__ amp_o, int32_t *__restrict__ info_o)
{
    LmState L;
    if (st == ST_B) {
        // after a B sweep only qtf and the inner-loop start change: read the
        // fields lm_after_b / lm_after_qtf / lm_start_inner use, write the
        // ones they set (half the state traffic of a full load/store)
        L.Jn0 = S.Jn0[k]; L.f0 = S.f0[k]; L.fnorm = S.fnorm[k]; L.acnorm = S.acnorm[k]; L.r = S.r[k];
        L.diag = S.diag[k]; L.delta = S.delta[k]; L.par = S.par[k]; L.x = S.x[k]; L.iter = S.iter[k];
        L.info = 0;
        st = lm_after_b(L, o.sum());
        S.qtf[k] = L.qtf; S.gnorm[k] = L.gnorm; S.diag[k] = L.diag; S.par[k] = L.par;
        S.delta[k] = L.delta; S.wa1[k] = L.wa1; S.x2[k] = L.x2; S.pnorm[k] = L.pnorm;
    } else if (st == ST_A0) {
        // the first transition: the state is k_fit_init's (x = 1, par = 0,
        // iter = 1) and lm_outer reads nothing else; on the usual way out (a B
        // request) only the fields it set are written
        L.x = 1.0; L.par = 0.0; L.iter = 1; L.info = 0;
        L.acn2 = 0.0; L.J02 = 0.0; L.f02 = 0.0;
        L.fnorm = o.fnorm();
        L.nfev = 1;
        L.acnorm = o.acnorm();
        o.f0J0(1.0, L.f0, L.J0);
        const int oe = o.exact();
        S.slow[k] = oe & 1;
        st = lm_outer(L);
        // J(1) == T and the same qrfac as k_fit_prep's: the round-0 sweep
        // already summed qtf's dot, so the B request is answered here
        if (st == ST_B && (oe & 2) && S.U[0] != 0.0 && L.acnorm == S.U[1] && L.aj == S.U[2] &&
            L.Jn0 == S.U[3]) {
            st = lm_after_b(L, o.sum());
            lm_store(L, S, k);
        } else if (st == ST_B) {
            S.fnorm[k] = L.fnorm; S.nfev[k] = L.nfev; S.acnorm[k] = L.acnorm; S.f0[k] = L.f0;
            S.J0[k] = L.J0; S.Jn0[k] = L.Jn0; S.aj[k] = L.aj; S.r[k] = L.r; S.diag[k] = L.diag;
            S.xnorm[k] = L.xnorm; S.delta[k] = L.delta;
        } else {
            lm_store(L, S, k);
        }
    } else if (st == ST_A2) {
        // lm_after_a2 and what follows it read 14 of the 19 fields (acnorm, J0,
        // f0, aj and Jn0 are set anew on the way that uses them), and write: on
        // a rejected step, the inner loop's 6 (nfev, par, delta, wa1, x2,
        // pnorm); on an accepted one those and the outer iteration's 13; on
        // ST_DONE, nothing but amp / info (most profiles end here)
        L.x = S.x[k]; L.fnorm = S.fnorm[k]; L.par = S.par[k]; L.delta = S.delta[k]; L.diag = S.diag[k];
        L.xnorm = S.xnorm[k]; L.r = S.r[k]; L.qtf = S.qtf[k]; L.gnorm = S.gnorm[k]; L.x2 = S.x2[k];
        L.pnorm = S.pnorm[k]; L.wa1 = S.wa1[k]; L.iter = S.iter[k]; L.nfev = S.nfev[k]; L.info = 0;
        L.acnorm = L.J0 = L.f0 = L.aj = L.Jn0 = 0.0;   // not read before they are set
        L.acn2 = o.acnorm();
        o.f0J0(L.x2, L.f02, L.J02);   // the A request was at the trial point x2
        bool accepted = false;
        st = lm_after_a2(L, o.fnorm(), &accepted);
        if (st != ST_DONE) {
            S.nfev[k] = L.nfev; S.par[k] = L.par; S.delta[k] = L.delta; S.wa1[k] = L.wa1; S.x2[k] = L.x2;
            S.pnorm[k] = L.pnorm;
            if (accepted) {
                S.x[k] = L.x; S.xnorm[k] = L.xnorm; S.fnorm[k] = L.fnorm; S.iter[k] = L.iter;
                S.acnorm[k] = L.acnorm; S.J0[k] = L.J0; S.f0[k] = L.f0; S.aj[k] = L.aj; S.r[k] = L.r;
                S.Jn0[k] = L.Jn0; S.qtf[k] = L.qtf; S.gnorm[k] = L.gnorm; S.diag[k] = L.diag;
                S.slow[k] = o.exact() & 1;   // J at the new x came from this sweep
            }
        }
    } else if (st != ST_DONE) {
        return st;   // (no other request exists)
    } else {
        return ST_DONE;
    }
    S.mode[k] = st;
    if (st == ST_A2) S.xa[k] = L.x2;
    if (st == ST_DONE) {
        amp_o[k] = L.x;
        info_o[k] = L.info;
    }
    return st;
}

// Consume the sweep result, run lmdif's scalar logic to the next request.
// Survivors (profiles still needing a sweep) are appended to next_list;
// *next_n counts them (order within the list is irrelevant: profiles are
// independent).  The append is aggregated per block (one atomic per 512
// profiles), and the last block to finish publishes the final count to
// host-mapped memory (host_n), so the host needs no copy dispatch to learn it.
// BS threads per block: 512 for rounds of kStateSmallP profiles or more,
// 256 below (twice the blocks: C5 47.8 -> 45.6-46.3 ms per clean; C2's late
// rounds 25.41-25.43 -> 25.29-25.31; 256 for C2's full rounds too: 26.55
// against 26.44-26.49)
constexpr long kStateSmallP = 524288;
template <int BS>
__global__ __launch_bounds__(BS) void k_fit_state(FitStateArrays S, long P, const int32_t *__restrict__ list,
                                                            const unsigned long long *__restrict__ nctr,
                                                            double *__restrict__ amp_o, int32_t *__restrict__ info_o,
                                                            int32_t *__restrict__ next_list,
                                                            unsigned long long *__restrict__ ctr,
                                                            unsigned *__restrict__ done, int32_t *host_n,
                                                            uint8_t *__restrict__ late)
{
    __shared__ int wcnt[BS / 64];
    __shared__ int woff[BS / 64];
    __shared__ int wcntB[BS / 64];
    __shared__ int woffB[BS / 64];
    const long slot = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const RoundList rl(list, nctr, P);
    const long nact = rl.n();
    // the grid is sized from an upper bound: blocks past the list return at
    // once, and only the nblk blocks with work take part in the append (a
    // same-address atomic each, ~12 ns apiece, serialised)
    const long nblk = (nact + blockDim.x - 1) / blockDim.x;
    if ((long)blockIdx.x >= nblk) {
        if (nblk == 0 && blockIdx.x == 0 && threadIdx.x == 0)   // empty list: the count is 0
            __hip_atomic_store(host_n, 0, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    int still = 0, stillB = 0;
    long k = 0;
    if (slot < nact) {
        k = rl.at(slot);
        const int st = fit_transition(S, k, S.mode[k], OutS{S, k}, amp_o, info_o);
        if (st != ST_DONE) still = st == ST_B ? 2 : 1;   // B requests go to the list's end
    }
    if (late && still) late[k] = 1;   // the fork round: still fitting after it
    // block-aggregated append, partitioned by request (RoundList)
    stillB = still == 2;
    still = still == 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(still), mB = __ballot(stillB);
    if (lane == 0) {
        wcnt[wave] = __popcll(m);
        wcntB[wave] = __popcll(mB);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0, totB = 0;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) {
            tot += wcnt[w];
            totB += wcntB[w];
        }
        // one atomic per block for both list offsets (B count, A count)
        const unsigned long long old = atomicAdd(ctr, rl_pack((unsigned)totB, (unsigned)tot));
        long base = (long)(old & 0xffffffffull), baseB = (long)(old >> 32);
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) {
            woff[w] = (int)base;
            base += wcnt[w];
            woffB[w] = (int)baseB;
            baseB += wcntB[w];
        }
        // then the finished-block count.  Both atomics are performed where
        // device-scope atomics are (coherent across XCDs) and return only once
        // performed; the wait below keeps a block's count behind its offset
        // atomic's return, so when the last block's count returns nblk - 1
        // every block's offsets were performed, and its load of ctr sees the
        // final counts of the round.  (An acq_rel count instead - an L2
        // write-back and invalidate per block - cost 1.4 ms per C2 clean.)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned fin = __hip_atomic_fetch_add(done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (fin == (unsigned)nblk - 1) {
            // (the last block only.  What makes its load of ctr see every
            // block's offset atomic is the hardware order above: each block's
            // returning offset atomic, then its vmcnt(0), then its count.  The
            // counts are relaxed - no release pairs with this acquire - so the
            // acquire fence only keeps the compiler and the L1 from serving the
            // load early; it is not a memory-model synchronisation.)
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            const unsigned long long v = __hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(host_n, (int32_t)((v & 0xffffffffull) + (v >> 32)), __ATOMIC_RELEASE,
                               __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    __syncthreads();
    if (still) next_list[woff[wave] + __popcll(m & ((1ull << lane) - 1ull))] = (int32_t)k;
    if (stillB) next_list[P - 1 - (woffB[wave] + __popcll(mB & ((1ull << lane) - 1ull)))] = (int32_t)k;
}

// ---- tail: the last few thousand profiles, one wave each, to completion ----
// Rounds over a small active list are latency-bound (a lone wave sweeping 64
// profiles).  Here one wave owns ONE profile: lanes compute the per-sample
// terms of a chunk in parallel (exact divisions), then every lane runs the
// sequential MINPACK accumulation over the chunk in LDS (same values in all
// lanes: uniform control flow), and the lmdif state machine runs in registers
// between sweeps — no host round trips, no state traffic.  All arithmetic is
// the exact path (true divisions, branchy enorm), so it matches k_fit_pass
// bit for bit whatever the lane's range.
#define TAIL_CH 256
#define TAIL_WAVES 2   // waves (profiles) per block: C4 2.88-2.92 -> 2.85-2.90 ms against 4; C2, C5 the same

// s += a[0], s += a[1], ... in order (and t over b, a second chain interleaved
// with it).  The terms are read from LDS in register blocks of SB, the next
// block's reads issued before the current block's adds, so the dependent f64
// adds, not the LDS latency, set the pace of the sequential MINPACK sums.
template <int SB, bool TWO>
__device__ __forceinline__ void seq_sums(const double *a, const double *b, int n, double &s, double &t)
{
    int q = 0;
    if (n >= SB) {
        double ca[SB], cb[SB];
#pragma unroll
        for (int i = 0; i < SB; ++i) {
            ca[i] = a[i];
            if (TWO) cb[i] = b[i];
        }
        for (q = SB; q + SB <= n; q += SB) {
            double na[SB], nb[SB];
#pragma unroll
            for (int i = 0; i < SB; ++i) {
                na[i] = a[q + i];
                if (TWO) nb[i] = b[q + i];
            }
#pragma unroll
            for (int i = 0; i < SB; ++i) {
                s = s + ca[i];
                if (TWO) t = t + cb[i];
            }
#pragma unroll
            for (int i = 0; i < SB; ++i) {
                ca[i] = na[i];
                if (TWO) cb[i] = nb[i];
            }
        }
#pragma unroll
        for (int i = 0; i < SB; ++i) {
            s = s + ca[i];
            if (TWO) t = t + cb[i];
        }
    }
    for (; q < n; ++q) {
        s = s + a[q];
        if (TWO) t = t + b[q];
    }
}

// One block: U = {valid, acnorm, aj, Jn0} (k_fit_pass's round-0 form computes
// Jn_i = RN(J_i / aj) itself, as the B sweep does).  MINPACK's enorm is a
// sequential sum: every thread squares its samples into LDS and checks the
// range, then one thread adds the squares in order (register blocks, the
// next block's reads ahead of the adds) - sqrt(sum_seq t^2) is MINPACK's enorm
// while every component is 0 or inside (RDWARF, agiant) (fa_add's argument);
// MINPACK's branchy enorm otherwise.
__global__ __launch_bounds__(256) void k_fit_prep(const double *__restrict__ T64, int nbin, int nsw,
                                                  double *__restrict__ U)
{
    extern __shared__ double sq[];   // [nsw]
    const double agiant = kRgiant / (double)nbin;
    int ok = 1;
    for (int i = threadIdx.x; i < nsw; i += blockDim.x) {
        const double a = fabs(T64[i]);
        ok &= (a == 0.0 || (a > kRdwarf && a < agiant)) ? 1 : 0;
        sq[i] = a * a;
    }
    const bool in_range = __syncthreads_and(ok) != 0;
    if (threadIdx.x != 0) return;
    double acn;
    if (in_range) {
        double s2 = 0.0, unused = 0.0;
        seq_sums<16, false>(sq, nullptr, nsw, s2, unused);
        acn = s2 != 0.0 ? sqrt(s2) : 0.0;   // MINPACK: sqrt(s2 (1 + 0)) with no small / large components
    } else {
        Enorm e;
        en_zero(e);
        for (int i = 0; i < nsw; ++i) en_add(e, T64[i], agiant);
        acn = en_fin(e);
    }
    const double J0 = T64[0];
    double ajnorm = acn, Jn0 = J0;   // lm_outer
    if (ajnorm != 0.0) {
        if (J0 < 0.0) ajnorm = -ajnorm;
        Jn0 = J0 / ajnorm;
        Jn0 = Jn0 + 1.0;
    }
    // the fast B sweep's conditions on aj as well (x = 1 is in range)
    const bool valid = acn != 0.0 && Jn0 != 0.0 && x_in_fast_range(ajnorm);
    U[0] = valid ? 1.0 : 0.0;
    U[1] = acn;
    U[2] = valid ? ajnorm : 1.0;
    U[3] = Jn0;
}

// one fit-cube row in either layout (d_ofs)
struct RowRef {
    const float *D;
    size_t k;
    int ldD, tiled;
    __device__ __forceinline__ float operator[](int i) const { return D[d_ofs(k, i, ldD, tiled)]; }
};

__device__ __forceinline__ void tail_sweep_a(const RowRef &p, const double *__restrict__ T64, int nbin,
                                             double xa, double agiant, double (*buf)[TAIL_CH], int lane,
                                             double &fnorm, double &acnorm, double &f0, double &J0)
{
    const double eps = sqrt(DBL_EPSILON);
    double h = eps * fabs(xa);
    if (h == 0.0) h = eps;
    const double xh = xa + h;
    Enorm eF, eJ;
    en_zero(eF);
    en_zero(eJ);
    for (int c0 = 0; c0 < nbin; c0 += TAIL_CH) {
        const int n = min(TAIL_CH, nbin - c0);
        bool okF = true, okJ = true;   // every component 0 or inside (RDWARF, agiant)
        for (int q = lane; q < n; q += 64) {
            const double t = T64[c0 + q];
            const double pv = (double)p[c0 + q];
            const double u = xa * t;
            const double f = u - pv;
            const double uh = xh * t;
            const double wa = uh - pv;
            const double d = wa - f;
            const double J = d / h;
            buf[0][q] = f;
            buf[1][q] = J;
            const double af = fabs(f), aJ = fabs(J);
            okF = okF && (af == 0.0 || (af > kRdwarf && af < agiant));
            okJ = okJ && (aJ == 0.0 || (aJ > kRdwarf && aJ < agiant));
            buf[2][q] = af * af;
            buf[3][q] = aJ * aJ;
        }
        okF = __all(okF);
        okJ = __all(okJ);
        wave_sync();
        if (c0 == 0) {
            f0 = buf[0][0];
            J0 = buf[1][0];
        }
        // in range, en_add is exactly s2 += x*x, in order (the squares were
        // formed above, off the dependency chain)
        if (okF && okJ) {   // the usual case: both chains interleaved
            double sF = eF.s2, sJ = eJ.s2;
            seq_sums<8, true>(buf[2], buf[3], n, sF, sJ);
            eF.s2 = sF;
            eJ.s2 = sJ;
        } else {
            if (okF) {
                double dummy = 0.0;
                seq_sums<16, false>(buf[2], nullptr, n, eF.s2, dummy);
            } else {
                for (int q = 0; q < n; ++q) en_add(eF, buf[0][q], agiant);
            }
            if (okJ) {
                double dummy = 0.0;
                seq_sums<16, false>(buf[3], nullptr, n, eJ.s2, dummy);
            } else {
                for (int q = 0; q < n; ++q) en_add(eJ, buf[1][q], agiant);
            }
        }
        wave_sync();
    }
    fnorm = en_fin(eF);
    acnorm = en_fin(eJ);
}

__device__ __forceinline__ double tail_sweep_b(const RowRef &p, const double *__restrict__ T64, int nbin,
                                               double x, double aj, double (*buf)[TAIL_CH], int lane)
{
    const double eps = sqrt(DBL_EPSILON);
    double h = eps * fabs(x);
    if (h == 0.0) h = eps;
    const double xh = x + h;
    double sum = 0.0;
    for (int c0 = 0; c0 < nbin; c0 += TAIL_CH) {
        const int n = min(TAIL_CH, nbin - c0);
        for (int q = lane; q < n; q += 64) {
            const double t = T64[c0 + q];
            const double pv = (double)p[c0 + q];
            const double u = x * t;
            const double f = u - pv;
            const double uh = xh * t;
            const double wa = uh - pv;
            const double d = wa - f;
            const double J = d / h;
            double Jn = J / aj;
            if (c0 + q == 0) Jn = Jn + 1.0;
            buf[0][q] = Jn * f;
        }
        wave_sync();
        double dummy = 0.0;
        seq_sums<16, false>(buf[0], nullptr, n, sum, dummy);
        wave_sync();
    }
    return sum;
}

// 3 waves per SIMD for the register allocation (2 waves: 0.1 ms per C2 clean slower)
__global__ __launch_bounds__(64 * TAIL_WAVES, 3) void k_fit_tail(const float *__restrict__ D,
                                                              const double *__restrict__ T64, long P, int nbin,
                                                              int ldD, int dtiled, const int32_t *__restrict__ list,
                                                              const unsigned long long *__restrict__ nctr,
                                                              FitStateArrays S,
                                                              double *__restrict__ amp_o,
                                                              int32_t *__restrict__ info_o,
                                                              unsigned long long *__restrict__ sweeps)
{
    __shared__ double sbuf[TAIL_WAVES][4][TAIL_CH];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double(*buf)[TAIL_CH] = sbuf[wave];
    const RoundList rl(list, nctr, P);
    const long nact = rl.n();
    const double agiant = kRgiant / (double)nbin;
    unsigned long long nsw = 0;
    for (long slot = (long)blockIdx.x * TAIL_WAVES + wave; slot < nact; slot += (long)gridDim.x * TAIL_WAVES) {
        const long k = rl.at(slot);
        int st = S.mode[k];
        if (st == ST_DONE) continue;
        LmState L;
        lm_load(L, S, k);
        double xa = S.xa[k];
        // the row's samples are contiguous in runs of 32 (tiled) or whole
        const RowRef p{D, (size_t)k, ldD, dtiled};
        while (st != ST_DONE) {
            ++nsw;
            if (st == ST_B) {
                const double sum = tail_sweep_b(p, T64, nbin, L.x, L.aj, buf, lane);
                st = lm_after_b(L, sum);
            } else {
                double fnorm, acnorm, f0 = 0.0, J0 = 0.0;
                tail_sweep_a(p, T64, nbin, xa, agiant, buf, lane, fnorm, acnorm, f0, J0);
                if (st == ST_A0) {
                    L.fnorm = fnorm;
                    L.nfev = 1;
                    L.acnorm = acnorm;
                    L.f0 = f0;
                    L.J0 = J0;
                    st = lm_outer(L);
                } else {
                    L.acn2 = acnorm;
                    L.f02 = f0;
                    L.J02 = J0;
                    st = lm_after_a2(L, fnorm);
                }
            }
            if (st == ST_A2) xa = L.x2;
        }
        if (lane == 0) {
            S.mode[k] = ST_DONE;
            amp_o[k] = L.x;
            info_o[k] = L.info;
        }
    }
    if (lane == 0 && nsw) atomicAdd(sweeps, nsw);
}

// ============================================================ launchers

// sweep length: nbin rounded up to whole tile pairs (sweep_dma)
static int sweep_len(int nbin) { return ((nbin + 2 * FIT_TB - 1) / (2 * FIT_TB)) * (2 * FIT_TB); }

hipError_t launch_fit_init(hipStream_t st, const FitStateArrays &S, long P, int32_t *z32, int nz32, uint8_t *late)
{
    IC_GGL(k_fit_init, dim3(cdiv(max(P, (long)nz32), 256)), dim3(256), 0, st, S, P, z32, nz32, late);
    return hipGetLastError();
}

hipError_t launch_fit_prep(hipStream_t st, const FitStateArrays &S, const double *T64, int nbin)
{
    const int nsw = sweep_len(nbin);
    IC_GGL(k_fit_prep, dim3(1), dim3(256), sizeof(double) * nsw, st, T64, nbin, nsw, S.U);
    return hipGetLastError();
}

hipError_t launch_fit_pass(hipStream_t st, const float *D, const double *T64, long P, int nbin, int ldD,
                           int dtiled, const int32_t *list, const unsigned long long *nctr, long bound,
                           const FitStateArrays &S, bool round0)
{
    const long n = list ? bound : P;
    if (n <= 0) return hipSuccess;
    const int nsw = sweep_len(nbin);   // the row stride ldD may be longer (padding off the power-of-two stride)
    if (ldD % 4 != 0 || ldD < nsw || (dtiled && ldD % 32 != 0)) return hipErrorInvalidValue;
    if (round0 && list) return hipErrorInvalidValue;
    if (round0)
        IC_GGL(k_fit_pass<true>, dim3(cdiv(n, 64)), dim3(64), 0, st, D, T64, P, nbin, ldD, nsw, dtiled,
                           list, nctr, S, (const double *)S.U);
    else
        IC_GGL(k_fit_pass<false>, dim3(cdiv(n, 64)), dim3(64), 0, st, D, T64, P, nbin, ldD, nsw,
                           dtiled, list, nctr, S, (const double *)nullptr);
    return hipGetLastError();
}

hipError_t launch_mark_list(hipStream_t st, const int32_t *list, const unsigned long long *nctr, long P, long bound,
                            uint8_t *m, uint8_t v)
{
    if (!list || !nctr || !m) return hipErrorInvalidValue;
    if (bound <= 0) return hipSuccess;
    IC_GGL(k_mark_list, dim3(cdiv(std::min(bound, P), 256)), dim3(256), 0, st, list, nctr, P, m, v);
    return hipGetLastError();
}

hipError_t launch_fit_state(hipStream_t st, const FitStateArrays &S, long P, const int32_t *list,
                            const unsigned long long *nctr, long bound, double *amp, int32_t *info,
                            int32_t *next_list, unsigned long long *ctr, unsigned *done, int32_t *host_n,
                            uint8_t *late)
{
    const long n = list ? bound : P;
    if (n <= 0) return hipSuccess;
    if (n < kStateSmallP)
        IC_GGL(k_fit_state<256>, dim3(cdiv(n, 256)), dim3(256), 0, st, S, P, list, nctr, amp, info, next_list, ctr,
               done, host_n, late);
    else
        IC_GGL(k_fit_state<512>, dim3(cdiv(n, 512)), dim3(512), 0, st, S, P, list, nctr, amp, info, next_list, ctr,
               done, host_n, late);
    return hipGetLastError();
}

hipError_t launch_fit_tail(hipStream_t st, const float *D, const double *T64, long P, int nbin, int ldD,
                           int dtiled, const int32_t *list, const unsigned long long *nctr, long bound,
                           const FitStateArrays &S, double *amp, int32_t *info, unsigned long long *sweeps,
                           int grid_cap)
{
    const long n = list ? bound : P;
    if (n <= 0) return hipSuccess;
    const unsigned grid = cap_grid((size_t)std::min<long>(cdiv(n, TAIL_WAVES), 65536), grid_cap);
    IC_GGL(k_fit_tail, dim3(grid), dim3(64 * TAIL_WAVES), 0, st, D, T64, P, nbin, ldD, dtiled, list, nctr,
                       S, amp, info, sweeps);
    return hipGetLastError();
}

}  // namespace icgpu
