// ic_stdtemplate.hip -- cleaning against a supplied standard profile (opt-in,
// ic_set_std_template): the standard is brought onto the archive's pulse phase
// and installed where k_tscrunch leaves the template.  The written definition
// is iterative_cleaner_amd/std_template.py; the kernels follow it bit for bit.
//
// Build: as the other units (-ffp-contract=off is load-bearing: every f64
// operation below is an individually rounded IEEE op in the order written).
//
// Kernels (iteration 1 of a run with a standard set, after the template stage):
//   k_std_ccf      c[k] = sum_i f64(A[i]) * (f64(S[(i - k) mod n]) - m), one
//                  thread per lag, in ascending i
//   k_std_peak     first argmax of c, the failure test (a non-finite value, no
//                  positive peak, or a deeper trough than the peak), the parabola through the
//                  peak's neighbours -> StdAlignRec (its shift is also the
//                  device-resident delay of the `frac` rotation, launch_rotate)
//   k_std_install  T, T64 (zero tail) and T2 from the standard: as given, gathered
//                  by the record's lag (int), or the rotated copy (frac)
#include <math.h>

#include "ic_wave.h"

namespace icgpu {

// One thread per lag, the lags split over the blocks (grid-stride: a capped
// grid walks them all).  S and A sit in LDS as f32 and are converted on read:
// lane l reads S[j0 + l + i] (consecutive banks) and every lane the same A[i]
// (a broadcast).  m: the mean of f64(S), summed in ascending index on the host
// when the standard is set (it depends on S alone).
__global__ __launch_bounds__(64) void k_std_ccf(const float *__restrict__ S, const float *__restrict__ A, int nbin,
                                                double m, double *__restrict__ c)
{
    extern __shared__ float sh_std[];
    float *ss = sh_std, *as = sh_std + nbin;
    for (int i = threadIdx.x; i < nbin; i += blockDim.x) {
        ss[i] = S[i];
        as[i] = A[i];
    }
    __syncthreads();
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < nbin; k += gridDim.x * blockDim.x) {
        double acc = 0.0;
        int j = k == 0 ? 0 : nbin - k;   // (0 - k) mod nbin
        for (int i = 0; i < nbin; ++i) {
            const double a = (double)as[i];
            const double s = (double)ss[j] - m;
            const double t = a * s;
            acc = acc + t;
            j = j + 1 == nbin ? 0 : j + 1;
        }
        c[k] = acc;
    }
}

// One block.  The argmax order (larger value, then lower index) is total over
// the finite values, so the result does not depend on the block size.
constexpr int kStdPeakThreads = 256;
__global__ __launch_bounds__(kStdPeakThreads) void k_std_peak(const double *__restrict__ c, int nbin,
                                                              StdAlignRec *__restrict__ rec)
{
    __shared__ double bv[kStdPeakThreads];
    __shared__ double lv[kStdPeakThreads];   // the smallest value
    __shared__ int bi[kStdPeakThreads];
    __shared__ int nonfinite;
    if (threadIdx.x == 0) nonfinite = 0;
    __syncthreads();
    double best = 0.0, low = 0.0;
    int besti = -1;
    bool nf = false;
    for (int k = threadIdx.x; k < nbin; k += kStdPeakThreads) {
        const double v = c[k];
        if (!isfinite(v))
            nf = true;
        else {
            if (besti < 0 || v < low) low = v;
            if (besti < 0 || v > best) {   // ascending k: the first of equal values stays
                best = v;
                besti = k;
            }
        }
    }
    if (nf) atomicOr(&nonfinite, 1);
    bv[threadIdx.x] = best;
    lv[threadIdx.x] = low;
    bi[threadIdx.x] = besti;
    __syncthreads();
    for (int off = kStdPeakThreads / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            const int o = threadIdx.x + off;
            const int ia = bi[threadIdx.x], ib = bi[o];
            if (ib >= 0 && (ia < 0 || lv[o] < lv[threadIdx.x])) lv[threadIdx.x] = lv[o];
            if (ib >= 0 && (ia < 0 || bv[o] > bv[threadIdx.x] || (bv[o] == bv[threadIdx.x] && ib < ia))) {
                bv[threadIdx.x] = bv[o];
                bi[threadIdx.x] = ib;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int ks = bi[0];
        StdAlignRec r;
        r.shift = 0.0;
        r.aligned = 0;
        r.lag = 0;
        if (!nonfinite && ks >= 0 && bv[0] > 0.0 && !(-lv[0] > bv[0])) {
            const double cm = c[ks == 0 ? nbin - 1 : ks - 1], c0 = c[ks], cp = c[ks + 1 == nbin ? 0 : ks + 1];
            const double den = (cm - c0) + (cp - c0);
            const double delta = den < 0.0 ? 0.5 * (cm - cp) / den : 0.0;
            r.shift = (double)ks + delta;
            r.aligned = 1;
            r.lag = ks;
        }
        *rec = r;
    }
}

// The three products k_tscrunch leaves, in the same relation to one another:
// T[nbin], T64[ldD] = f64(T) with a zero tail, T2[2 nbin] = T64[0..nbin) twice.
// mode kAlignInt gathers S by the record's lag (0 after a failed alignment);
// kAlignFrac takes R, the rotated standard, unless the alignment failed.
__global__ __launch_bounds__(256) void k_std_install(const float *__restrict__ S, const float *__restrict__ R,
                                                     const StdAlignRec *__restrict__ rec, int mode, int nbin, int ldD,
                                                     float *__restrict__ T, double *__restrict__ T64,
                                                     double *__restrict__ T2)
{
    int lag = 0;
    bool rot = false;
    if (mode == kAlignInt) {
        lag = rec->lag;
        if (lag < 0 || lag >= nbin) lag = 0;
    } else if (mode == kAlignFrac) {
        rot = rec->aligned != 0;
    }
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < ldD; i += gridDim.x * blockDim.x) {
        if (i < nbin) {
            int j = i - lag;
            if (j < 0) j += nbin;
            const float v = rot ? R[i] : S[j];
            const double d = (double)v;
            T[i] = v;
            T64[i] = d;
            if (T2) {
                T2[i] = d;
                T2[i + nbin] = d;
            }
        } else {
            T64[i] = 0.0;
        }
    }
}

// ============================================================ launchers

size_t std_ccf_lds_bytes(int nbin) { return 2 * (size_t)nbin * sizeof(float); }

hipError_t launch_std_ccf(hipStream_t st, const float *S, const float *A, int nbin, double m, double *c, int grid_cap)
{
    const size_t shm = std_ccf_lds_bytes(nbin);
    if (!S || !A || !c || nbin < 1 || shm > kLdsBlockMax) return hipErrorInvalidValue;
    const unsigned grid = cap_grid(cdiv(nbin, 64), grid_cap);
    IC_GGL(k_std_ccf, dim3(grid), dim3(64), shm, st, S, A, nbin, m, c);
    return hipGetLastError();
}

hipError_t launch_std_peak(hipStream_t st, const double *c, int nbin, StdAlignRec *rec)
{
    if (!c || !rec || nbin < 1) return hipErrorInvalidValue;
    IC_GGL(k_std_peak, dim3(1), dim3(kStdPeakThreads), 0, st, c, nbin, rec);
    return hipGetLastError();
}

hipError_t launch_std_install(hipStream_t st, const float *S, const float *R, const StdAlignRec *rec, int mode,
                              int nbin, int ldD, float *T, double *T64, double *T2, int grid_cap)
{
    if (!S || !T || !T64 || nbin < 1 || ldD < nbin || (mode != kAlignNone && !rec) || (mode == kAlignFrac && !R) ||
        (mode != kAlignNone && mode != kAlignInt && mode != kAlignFrac))
        return hipErrorInvalidValue;
    const unsigned grid = cap_grid(cdiv(ldD, 256), grid_cap);
    IC_GGL(k_std_install, dim3(grid), dim3(256), 0, st, S, R, rec, mode, nbin, ldD, T, T64, T2);
    return hipGetLastError();
}

}  // namespace icgpu
