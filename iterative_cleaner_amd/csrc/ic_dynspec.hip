// ic_dynspec.hip -- opt-in dynamic spectrum (ic_get_dynspec): after a run, the
// amplitude, its error and the baseline of a free-baseline template fit to
// every dedispersed profile of the resident cube, zapped profiles masked.  The
// written definition is iterative_cleaner_amd/dynspec.py; the kernels follow it
// bit for bit.
//
// Build: as the other units (-ffp-contract=off is load-bearing: every product
// of the definition is rounded on its own before it is added).
//
// The definition's one summation rule, sum64, is made for a wave: 64 chains,
// chain l adding v[l], v[l + 64], ... in ascending order, then the halving tree
// c[l] += c[l + h], h = 32 .. 1.  Lane l is chain l, and the tree is six
// shuffles down.
//
// Kernels (launched by ic_get_dynspec / ic_dynspec_profiles only, never by a run):
//   k_dynspec_prep      once per call, one wave: mT, Stt and the f64 table t[i] =
//                       f64(T[i]) - mT from the device's template (no host read)
//   k_dynspec<NV, FULL> one wave per profile, grid-stride over the profiles,
//                       four waves per block.  A lane holds its NV = 1 .. 128
//                       samples (nbin <= 64 NV; FULL: nbin == 64 NV, no
//                       predicates) as f32 in registers: the row is read from
//                       memory once and serves both passes (the sums of x and
//                       t x, then the residual).  The table t is the same for
//                       every profile: up to NV = 32 (2048 bins) a lane keeps
//                       its 2 NV words of it in registers for the whole grid
//                       loop; at NV = 64 and 128 (4096, 8192 bins) the block
//                       stages it in LDS (32 / 64 KiB) and reads it per pass.
//   k_dynspec_long      nbin > 8192: the same chains with the row read twice
//                       (the second time from L2) and t from memory.
// Two input forms: the raw cube with the channel's integer shift (a gather at
// the dedispersed index), or rows that are already dedispersed (shift == null).
#include <algorithm>
#include <math.h>

#include "ic_wave.h"

namespace icgpu {

namespace {

constexpr int kDynWaves = 4;   // waves (profiles in flight) per block

// the halving tree of sum64 over the lanes' chains; the result is wave-uniform
__device__ __forceinline__ double dyn_tree(double c)
{
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) c = c + __shfl_down(c, (unsigned)h, 64);
    return lane_read(c, 0);
}

// source index of dedispersed bin i (sh in [0, nbin))
__device__ __forceinline__ int dyn_src(int i, int sh, int nbin)
{
    const int j = i + sh;
    return j >= nbin ? j - nbin : j;
}

__device__ __forceinline__ int dyn_shift(const int32_t *shift, long k, int nchan, int nbin)
{
    if (!shift) return 0;
    const int sh = shift[k % nchan] % nbin;
    return sh < 0 ? sh + nbin : sh;
}

// the per-profile epilogue from the three sums' inputs; lane 0 stores
__device__ __forceinline__ void dyn_store(const DynspecArgs &a, long k, int lane, double amp, double err, double base)
{
    if (lane == 0) {
        if (a.amp) a.amp[k] = amp;
        if (a.err) a.err[k] = err;
        if (a.base) a.base[k] = base;
    }
}

}  // namespace

// tt[0] = mT, tt[1] = Stt, tt[2 + i] = t_i
__global__ __launch_bounds__(64) void k_dynspec_prep(const float *__restrict__ T, int nbin, double *__restrict__ tt)
{
    const int lane = threadIdx.x;
    double c = 0.0;
    for (int i = lane; i < nbin; i += 64) c = c + (double)T[i];
    const double mT = dyn_tree(c) / (double)nbin;
    double q = 0.0;
    for (int i = lane; i < nbin; i += 64) {
        const double t = (double)T[i] - mT;
        tt[2 + i] = t;
        q = q + t * t;
    }
    const double Stt = dyn_tree(q);
    if (lane == 0) {
        tt[0] = mT;
        tt[1] = Stt;
    }
}

template <int NV, bool FULL>
__global__ __launch_bounds__(64 * kDynWaves) void k_dynspec(DynspecArgs a)
{
    constexpr bool kTReg = NV <= 32;
    __shared__ double tl[kTReg ? 1 : 64 * NV];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nbin = a.nbin;
    const double mT = a.tt[0], Stt = a.tt[1];
    const double *__restrict__ tg = a.tt + 2;
    double tv[kTReg ? NV : 1];
    if (kTReg) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int i = lane + 64 * j;
            tv[kTReg ? j : 0] = (FULL || i < nbin) ? tg[i] : 0.0;
        }
    } else {
        for (int i = threadIdx.x; i < nbin; i += 64 * kDynWaves) tl[i] = tg[i];
        __syncthreads();
    }
    const double n = (double)nbin, dof = (double)(nbin - 2), rt = sqrt(Stt);
    const long stride = (long)gridDim.x * kDynWaves;
    for (long k = (long)blockIdx.x * kDynWaves + wave; k < a.P; k += stride) {
        if (a.w[k] == 0.0f) {   // masked: the row is not read
            dyn_store(a, k, lane, 0.0, 0.0, 0.0);
            continue;
        }
        const float *__restrict__ row = a.x + (size_t)k * nbin;
        const int sh = dyn_shift(a.shift, k, a.nchan, nbin);
        float xv[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int i = lane + 64 * j;
            xv[j] = (FULL || i < nbin) ? row[dyn_src(i, sh, nbin)] : 0.0f;
        }
        double cx = 0.0, ctx = 0.0;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int i = lane + 64 * j;
            if (FULL || i < nbin) {
                const double x = (double)xv[j];
                const double t = kTReg ? tv[kTReg ? j : 0] : tl[i];
                cx = cx + x;
                ctx = ctx + t * x;
            }
        }
        const double mx = dyn_tree(cx) / n;
        const double amp = dyn_tree(ctx) / Stt;
        const double base = mx - amp * mT;
        // the f32 samples are what stays in registers between the passes: the
        // compiler must not keep their f64 conversions (twice the registers)
#pragma unroll
        for (int j = 0; j < NV; ++j) asm volatile("" : "+v"(xv[j]));
        double cr = 0.0;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int i = lane + 64 * j;
            if (FULL || i < nbin) {
                const double t = kTReg ? tv[kTReg ? j : 0] : tl[i];
                const double r = ((double)xv[j] - mx) - amp * t;
                cr = cr + r * r;
            }
        }
        const double err = sqrt(dyn_tree(cr) / dof) / rt;
        dyn_store(a, k, lane, amp, err, base);
    }
}

__global__ __launch_bounds__(64 * kDynWaves) void k_dynspec_long(DynspecArgs a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nbin = a.nbin;
    const double mT = a.tt[0], Stt = a.tt[1];
    const double *__restrict__ tg = a.tt + 2;
    const double n = (double)nbin, dof = (double)(nbin - 2), rt = sqrt(Stt);
    const long stride = (long)gridDim.x * kDynWaves;
    for (long k = (long)blockIdx.x * kDynWaves + wave; k < a.P; k += stride) {
        if (a.w[k] == 0.0f) {
            dyn_store(a, k, lane, 0.0, 0.0, 0.0);
            continue;
        }
        const float *__restrict__ row = a.x + (size_t)k * nbin;
        const int sh = dyn_shift(a.shift, k, a.nchan, nbin);
        double cx = 0.0, ctx = 0.0;
        for (int i = lane; i < nbin; i += 64) {
            const double x = (double)row[dyn_src(i, sh, nbin)];
            cx = cx + x;
            ctx = ctx + tg[i] * x;
        }
        const double mx = dyn_tree(cx) / n;
        const double amp = dyn_tree(ctx) / Stt;
        const double base = mx - amp * mT;
        double cr = 0.0;
        for (int i = lane; i < nbin; i += 64) {
            const double r = ((double)row[dyn_src(i, sh, nbin)] - mx) - amp * tg[i];
            cr = cr + r * r;
        }
        const double err = sqrt(dyn_tree(cr) / dof) / rt;
        dyn_store(a, k, lane, amp, err, base);
    }
}

// ============================================================ launchers

hipError_t launch_dynspec_prep(hipStream_t st, const float *T, int nbin, double *tt)
{
    if (!T || !tt || nbin < kDynMinBin) return hipErrorInvalidValue;
    IC_GGL(k_dynspec_prep, dim3(1), dim3(64), 0, st, T, nbin, tt);
    return hipGetLastError();
}

static unsigned dyn_grid(const DynspecArgs &a)
{
    return cap_grid(std::min<size_t>(cdiv((size_t)a.P, kDynWaves), 256 * 16), a.grid_cap);
}

template <int NV> static hipError_t launch_dynspec_nv(hipStream_t st, const DynspecArgs &a)
{
    if (a.nbin == 64 * NV)
        IC_GGL((k_dynspec<NV, true>), dim3(dyn_grid(a)), dim3(64 * kDynWaves), 0, st, a);
    else
        IC_GGL((k_dynspec<NV, false>), dim3(dyn_grid(a)), dim3(64 * kDynWaves), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_dynspec(hipStream_t st, const DynspecArgs &a)
{
    if (!a.x || !a.w || !a.tt || a.P < 1 || a.nbin < kDynMinBin || (a.shift && a.nchan < 1))
        return hipErrorInvalidValue;
    const int n = a.nbin;
    if (n <= 64) return launch_dynspec_nv<1>(st, a);
    if (n <= 128) return launch_dynspec_nv<2>(st, a);
    if (n <= 256) return launch_dynspec_nv<4>(st, a);
    if (n <= 512) return launch_dynspec_nv<8>(st, a);
    if (n <= 1024) return launch_dynspec_nv<16>(st, a);
    if (n <= 2048) return launch_dynspec_nv<32>(st, a);
    if (n <= 4096) return launch_dynspec_nv<64>(st, a);
    if (n <= kDynRegMaxBin) return launch_dynspec_nv<128>(st, a);
    IC_GGL(k_dynspec_long, dim3(dyn_grid(a)), dim3(64 * kDynWaves), 0, st, a);
    return hipGetLastError();
}

}  // namespace icgpu
