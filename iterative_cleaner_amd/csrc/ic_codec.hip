// ic_codec.hip -- input preparation and the sample codec: pscrunch
// (k_pscrunch), the PSRFITS int16 decode (k_decode_q, k_decode_q_scalar) and
// encode (k_encode_q), the residual formed and encoded in one pass
// (k_residual_q), with their launchers.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see Makefile).
// -ffp-contract=off is load-bearing: every f64/f32 operation below must be an
// individually rounded IEEE op in the order written, so that results equal
// numpy / scipy (MINPACK) bit-for-bit.  Explicit fma() is never used on an
// exact path.
#include <algorithm>
#include <math.h>

#include "ic_fftdiag.h"

namespace icgpu {

// pscrunch on the device: raw = f32(pol0 + pol1), float4 grid-stride
__global__ __launch_bounds__(256) void k_pscrunch(float *__restrict__ raw, const float *__restrict__ pol1, size_t n)
{
    const size_t n4 = n / 4;
    float4 *r4 = (float4 *)raw;
    const float4 *p4 = (const float4 *)pol1;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        float4 a = r4[i];
        const float4 b = p4[i];
        a.x = a.x + b.x;
        a.y = a.y + b.y;
        a.z = a.z + b.z;
        a.w = a.w + b.w;
        r4[i] = a;
    }
    for (size_t i = 4 * n4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        raw[i] = raw[i] + pol1[i];
}

// PSRFITS fold-mode decode on the device (psrfits.py decode + archive.py
// pscrunch): q [nsub][nsum][nchan][nbin] int16, scl / offs [nsub][nsum][nchan],
// raw [nsub][nchan][nbin] = f32(f32(q0) * scl0 + offs0) (nsum 1) or the f32 sum
// of the two polarisations' decoded values (nsum 2).  Multiply, add and
// polarisation add are three separate IEEE roundings whatever -ffp-contract says.
__device__ __forceinline__ float q_decode(int q, float scl, float offs)
{
    return __fadd_rn(__fmul_rn((float)q, scl), offs);
}

// two samples of one 32-bit word (the first in the low half), native order
template <bool BE>
__device__ __forceinline__ void q_pair(uint32_t w, int &lo, int &hi)
{
    if (BE) w = ((w & 0x00ff00ffu) << 8) | ((w >> 8) & 0x00ff00ffu);
    lo = (int)(int16_t)(w & 0xffffu);
    hi = (int)(int16_t)(w >> 16);
}

template <bool BE>
__device__ __forceinline__ void q_decode8(const uint4 v, float scl, float offs, float *o)
{
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int lo, hi;
        q_pair<BE>(w[j], lo, hi);
        o[2 * j] = q_decode(lo, scl, offs);
        o[2 * j + 1] = q_decode(hi, scl, offs);
    }
}

// nbin % 8 == 0: a lane takes 8 consecutive samples of one profile (one 16-byte
// load per polarisation, two 16-byte stores); gpp = nbin / 8 groups per
// profile, I wide enough for NSUM * ngroups
template <bool BE, int NSUM, typename I>
__global__ __launch_bounds__(256) void k_decode_q(const int16_t *__restrict__ q, const float *__restrict__ scl,
                                                  const float *__restrict__ offs, float *__restrict__ raw, I ngroups,
                                                  I gpp, I nchan)
{
    const uint4 *q4 = (const uint4 *)q;
    float4 *r4 = (float4 *)raw;
    for (I g = (I)blockIdx.x * 256 + threadIdx.x; g < ngroups; g += (I)gridDim.x * 256) {
        const I p = g / gpp;                                         // output profile s * nchan + c
        const I pq = NSUM == 2 ? p + (p / nchan) * nchan : p;        // (s, pol 0, c) in q's profile order
        const I gq = pq * gpp + (g - p * gpp);
        float a[8];
        q_decode8<BE>(q4[gq], scl[pq], offs[pq], a);
        if (NSUM == 2) {
            float b[8];
            q_decode8<BE>(q4[gq + nchan * gpp], scl[pq + nchan], offs[pq + nchan], b);
#pragma unroll
            for (int j = 0; j < 8; ++j) a[j] = __fadd_rn(a[j], b[j]);
        }
        r4[2 * (size_t)g] = make_float4(a[0], a[1], a[2], a[3]);
        r4[2 * (size_t)g + 1] = make_float4(a[4], a[5], a[6], a[7]);
    }
}

// any nbin: one sample per lane and step, the profile index per sample
template <bool BE, int NSUM>
__global__ __launch_bounds__(256) void k_decode_q_scalar(const int16_t *__restrict__ q, const float *__restrict__ scl,
                                                         const float *__restrict__ offs, float *__restrict__ raw,
                                                         size_t n, size_t nbin, size_t nchan)
{
    const uint16_t *qu = (const uint16_t *)q;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const size_t p = i / nbin;
        const size_t pq = NSUM == 2 ? p + (p / nchan) * nchan : p;
        const size_t iq = pq * nbin + (i - p * nbin);
        float a = 0.0f;
#pragma unroll
        for (int k = 0; k < NSUM; ++k) {
            uint32_t w = qu[iq + k * nchan * nbin];
            if (BE) w = ((w & 0xffu) << 8) | (w >> 8);
            const float d = q_decode((int)(int16_t)w, scl[pq + k * nchan], offs[pq + k * nchan]);
            a = k == 0 ? d : __fadd_rn(a, d);
        }
        raw[i] = a;
    }
}

// PSRFITS fold-mode encode on the device (psrfits.py quantise), the decode in
// reverse: in [nprof][nbin] f32 -> q [nprof][nbin] int16, scl / offs [nprof].
// Per profile, with mn / mx its minimum and maximum (NaN if any sample is NaN,
// numpy's rule):
//   offs = f32(0.5 * (f64(mx) + f64(mn)))
//   scl  = f32((f64(mx) - f64(mn)) / 65534), 1 unless scl > 0 and finite
//   q    = clamp(rint((f64(d) - f64(offs)) / f64(scl)), -32767, 32767), NaN -> 0
// every step its own IEEE operation (an f64 subtraction and a true division per
// sample, round half to even), so the bits are the host's.  The comparisons
// skip NaN samples and a flag carries them, because the hardware's min / max
// return the other operand.
__device__ __forceinline__ int q_encode(float d, double offs, double scl)
{
    const double x = __ddiv_rn(__dsub_rn((double)d, offs), scl);
    if (x != x) return 0;
    const double r = rint(x);          // +-inf clamp like any large value
    return (int)(r < -32767.0 ? -32767.0 : (r > 32767.0 ? 32767.0 : r));
}

// two samples into one 32-bit word (the first in the low half), BE: each
// sample's bytes swapped (q_pair in reverse)
template <bool BE>
__device__ __forceinline__ uint32_t q_pack(int lo, int hi)
{
    uint32_t w = ((uint32_t)lo & 0xffffu) | ((uint32_t)hi << 16);
    if (BE) w = ((w & 0x00ff00ffu) << 8) | ((w >> 8) & 0x00ff00ffu);
    return w;
}

__device__ __forceinline__ void q_minmax(float x, float &mn, float &mx, int &nan)
{
    nan |= x != x;
    mn = x < mn ? x : mn;
    mx = x > mx ? x : mx;
}

// The block's (256 lanes) minimum, maximum and NaN flag from every lane's own,
// reduced in the wave by shuffles and across the four waves through LDS, then
// the profile's scl / offs by the rule above: the same values in every lane.
// Two barriers: the second frees r for the block's next profile.
// A row of zeros of both signs: the comparisons keep the zero met first (a tie
// keeps the lane's own, the lower lane's, the lower wave's), which for
// k_encode_q's lanes, taking the samples in order, is sample 0's.  A kernel
// whose lanes take them in another order passes `first`, sample 0 as stored
// where the first barrier publishes it, and gets the same sign.
struct QReduce {
    float mn[4], mx[4];
    int nan[4];
};
__device__ __forceinline__ void q_scale_block(float mn, float mx, int nan, QReduce &r, float &fs, float &fo,
                                              const float *first = nullptr)
{
    const int tid = threadIdx.x, wave = tid >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float a = __shfl_xor(mn, off), b = __shfl_xor(mx, off);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
        nan |= __shfl_xor(nan, off);
    }
    if ((tid & 63) == 0) {
        r.mn[wave] = mn;
        r.mx[wave] = mx;
        r.nan[wave] = nan;
    }
    __syncthreads();
    mn = r.mn[0];
    mx = r.mx[0];
    nan = r.nan[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
        mn = r.mn[w] < mn ? r.mn[w] : mn;
        mx = r.mx[w] > mx ? r.mx[w] : mx;
        nan |= r.nan[w];
    }
    if (first && mn == 0.0f && mx == 0.0f) mn = mx = *first;
    __syncthreads();               // the next profile writes r again
    if (nan) mn = mx = NAN;
    fo = (float)__dmul_rn(0.5, __dadd_rn((double)mx, (double)mn));
    fs = (float)__ddiv_rn(__dsub_rn((double)mx, (double)mn), 65534.0);
    if (!(fs > 0.0f && isfinite(fs))) fs = 1.0f;
}

// eight samples into one 16-byte store
template <bool BE>
__device__ __forceinline__ uint4 q_encode8(const float4 a, const float4 b, double o, double s)
{
    return make_uint4(q_pack<BE>(q_encode(a.x, o, s), q_encode(a.y, o, s)),
                      q_pack<BE>(q_encode(a.z, o, s), q_encode(a.w, o, s)),
                      q_pack<BE>(q_encode(b.x, o, s), q_encode(b.y, o, s)),
                      q_pack<BE>(q_encode(b.z, o, s), q_encode(b.w, o, s)));
}
// one sample as its 2 stored bytes
template <bool BE>
__device__ __forceinline__ uint16_t q_encode1(float d, double o, double s)
{
    uint32_t w = (uint32_t)q_encode(d, o, s) & 0xffffu;
    if (BE) w = ((w & 0xffu) << 8) | (w >> 8);
    return (uint16_t)w;
}

// One 256-lane block per profile, grid-stride over the profiles.  Pass 1: the
// block's minimum and maximum (16-byte loads when V4: nbin % 4 == 0), reduced
// by q_scale_block; lane 0 stores scl / offs.  Pass 2 reads the
// profile again (at most 32 KB, just read) and writes the samples, 8 per lane
// in one 16-byte store when V8 (nbin % 8 == 0), else one by one.
template <bool BE, bool V4, bool V8>
__global__ __launch_bounds__(256) void k_encode_q(const float *__restrict__ in, int nprof, int nbin,
                                                  int16_t *__restrict__ q, float *__restrict__ scl,
                                                  float *__restrict__ offs)
{
    __shared__ QReduce red;
    const int tid = threadIdx.x;
    for (int p = blockIdx.x; p < nprof; p += gridDim.x) {
        const float *src = in + (size_t)p * nbin;
        float mn = INFINITY, mx = -INFINITY;
        int nan = 0;
        if (V4) {
            const float4 *s4 = (const float4 *)src;
            for (int i = tid; i < nbin / 4; i += 256) {
                const float4 v = s4[i];
                q_minmax(v.x, mn, mx, nan);
                q_minmax(v.y, mn, mx, nan);
                q_minmax(v.z, mn, mx, nan);
                q_minmax(v.w, mn, mx, nan);
            }
        } else {
            for (int i = tid; i < nbin; i += 256) q_minmax(src[i], mn, mx, nan);
        }
        float fs, fo;
        q_scale_block(mn, mx, nan, red, fs, fo);
        if (tid == 0) {
            scl[p] = fs;
            offs[p] = fo;
        }
        const double o = (double)fo, s = (double)fs;
        if (V8) {
            const float4 *s4 = (const float4 *)src;
            uint4 *dst = (uint4 *)(q + (size_t)p * nbin);
            for (int g = tid; g < nbin / 8; g += 256) dst[g] = q_encode8<BE>(s4[2 * g], s4[2 * g + 1], o, s);
        } else {
            uint16_t *dst = (uint16_t *)q + (size_t)p * nbin;
            for (int i = tid; i < nbin; i += 256) dst[i] = q_encode1<BE>(src[i], o, s);
        }
    }
}

// The residual of the last iteration encoded in one pass (ic_get_residual_quantised
// with integer shifts): k_residual's row, formed once from the fit cube D (either
// layout) or, D == nullptr (fit_mode 1), from f32(raw - base); held in LDS in the
// dispersed frame, j = (i + shift) mod nbin, between q_scale_block and the
// quantise pass, so no f32 residual reaches memory.  One 256-lane block per
// profile, grid-stride; LDS: nbin floats (dynamic, nbin <= kResidualQMaxBin).
// V4 (nbin % 4 == 0, D / raw 16-byte aligned): a lane loads 4 bins at once,
// fit-cube bins i (their LDS stores then land 4 dwords apart, a 4-way bank
// conflict that stays far below the row's HBM time) or raw bins j.
// V8 (nbin % 8 == 0, q 16-byte aligned): every row of q starts 16-byte aligned.
// Otherwise a row starts on any 2-byte boundary (an odd nbin: every other row
// off a 4-byte one): up to 7 single samples bring it to a 16-byte boundary of
// q, whole 16-byte stores follow, single samples finish the row.
template <bool BE, bool V4, bool V8>
__global__ __launch_bounds__(256, 6) void k_residual_q(const float *__restrict__ D, const float *__restrict__ raw,
                                                    const float *__restrict__ base, const double *__restrict__ T64,
                                                    const double *__restrict__ amp, const int32_t *__restrict__ info,
                                                    const int32_t *__restrict__ shift, size_t P, int nchan, int nbin,
                                                    int ldD, int dtiled, PulseRegion pr, int16_t *__restrict__ q,
                                                    float *__restrict__ scl, float *__restrict__ offs)
{
    // all LDS in the dynamic region, whose base is then 16-byte aligned: the
    // row, padded to whole float4s, then the reduction's words
    extern __shared__ __attribute__((aligned(16))) float q_row[];
    QReduce &red = *(QReduce *)(q_row + ((nbin + 3) & ~3));
    const int tid = threadIdx.x;
    for (size_t k = blockIdx.x; k < P; k += gridDim.x) {
        const int sh = shift[k % nchan];
        const bool ok = fit_ok(info[k]);
        const double a = amp[k];
        float mn = INFINITY, mx = -INFINITY;
        int nan = 0;
        if (!ok) {   // no solution: the row is zero
            for (int j = tid; j < nbin; j += 256) q_row[j] = 0.0f;
            mn = mx = 0.0f;
        } else if (D) {
            if (V4) {
                for (int i4 = 4 * tid; i4 < nbin; i4 += 1024) {
                    const float4 pv = *(const float4 *)(D + d_ofs(k, i4, ldD, dtiled));
                    const float p[4] = {pv.x, pv.y, pv.z, pv.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int i = i4 + e;
                        int j = i + sh;
                        if (j >= nbin) j -= nbin;
                        const float v = residual_sample(a, T64[i], p[e], i, pr);
                        q_minmax(v, mn, mx, nan);
                        q_row[j] = v;
                    }
                }
            } else {
                for (int i = tid; i < nbin; i += 256) {
                    int j = i + sh;
                    if (j >= nbin) j -= nbin;
                    const float v = residual_sample(a, T64[i], D[d_ofs(k, i, ldD, dtiled)], i, pr);
                    q_minmax(v, mn, mx, nan);
                    q_row[j] = v;
                }
            }
        } else {
            const float b = base[k];
            const float *src = raw + k * nbin;
            if (V4) {
                for (int j4 = 4 * tid; j4 < nbin; j4 += 1024) {
                    const float4 xv = *(const float4 *)(src + j4);
                    const float x[4] = {xv.x, xv.y, xv.z, xv.w};
                    float v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        int i = j4 + e - sh;
                        if (i < 0) i += nbin;
                        v[e] = residual_sample(a, T64[i], x[e] - b, i, pr);
                        q_minmax(v[e], mn, mx, nan);
                    }
                    *(float4 *)(q_row + j4) = make_float4(v[0], v[1], v[2], v[3]);
                }
            } else {
                for (int j = tid; j < nbin; j += 256) {
                    int i = j - sh;
                    if (i < 0) i += nbin;
                    const float v = residual_sample(a, T64[i], src[j] - b, i, pr);
                    q_minmax(v, mn, mx, nan);
                    q_row[j] = v;
                }
            }
        }
        float fs, fo;
        q_scale_block(mn, mx, nan, red, fs, fo, q_row);   // its barriers also publish q_row
        if (tid == 0) {
            scl[k] = fs;
            offs[k] = fo;
        }
        const double o = (double)fo, s = (double)fs;
        int16_t *dst = q + k * nbin;
        if (V8) {
            const float4 *r4 = (const float4 *)q_row;
            for (int g = tid; g < nbin / 8; g += 256) ((uint4 *)dst)[g] = q_encode8<BE>(r4[2 * g], r4[2 * g + 1], o, s);
        } else {
            int head = (int)((16 - ((uintptr_t)dst & 15)) & 15) / 2;   // samples before q's next 16-byte boundary
            if (head > nbin) head = nbin;
            const int ng = (nbin - head) / 8;
            for (int g = tid; g < ng; g += 256) {
                const float *r = q_row + head + 8 * g;
                *(uint4 *)(dst + head + 8 * g) = q_encode8<BE>(make_float4(r[0], r[1], r[2], r[3]),
                                                               make_float4(r[4], r[5], r[6], r[7]), o, s);
            }
            // the head and what the whole stores left: fewer than 15 samples
            for (int t = tid; t < nbin - 8 * ng; t += 256) {
                const int j = t < head ? t : t + 8 * ng;
                ((uint16_t *)dst)[j] = q_encode1<BE>(q_row[j], o, s);
            }
        }
        __syncthreads();               // the next profile writes q_row again
    }
}

// ============================================================ launchers

hipError_t launch_pscrunch(hipStream_t st, float *raw, const float *pol1, size_t n, int grid_cap)
{
    const unsigned grid = cap_grid(std::min<unsigned>(cdiv(n / 4 + 1, 256), 8192), grid_cap);
    IC_GGL(k_pscrunch, dim3(grid), dim3(256), 0, st, raw, pol1, n);
    return hipGetLastError();
}

namespace {
template <bool BE, int NSUM>
void decode_q_dispatch(hipStream_t st, const int16_t *q, const float *scl, const float *offs, size_t P, int nchan,
                       int nbin, float *raw, int grid_cap)
{
    const size_t n = P * (size_t)nbin;
    if (nbin % 8 == 0 && (((uintptr_t)q | (uintptr_t)raw) & 15) == 0) {
        const size_t ng = n / 8;
        const dim3 grid(cap_grid(std::min<size_t>(cdiv(ng, 256), 8192), grid_cap));
        if (ng * NSUM < ((size_t)1 << 31))
            IC_GGL((k_decode_q<BE, NSUM, uint32_t>), grid, dim3(256), 0, st, q, scl, offs, raw, (uint32_t)ng,
                   (uint32_t)(nbin / 8), (uint32_t)nchan);
        else
            IC_GGL((k_decode_q<BE, NSUM, size_t>), grid, dim3(256), 0, st, q, scl, offs, raw, ng, (size_t)(nbin / 8),
                   (size_t)nchan);
    } else {
        const dim3 grid(cap_grid(std::min<size_t>(cdiv(n, 256), 65536), grid_cap));
        IC_GGL((k_decode_q_scalar<BE, NSUM>), grid, dim3(256), 0, st, q, scl, offs, raw, n, (size_t)nbin,
               (size_t)nchan);
    }
}
}  // namespace

hipError_t launch_decode_q(hipStream_t st, const int16_t *q, const float *scl, const float *offs, int nsub, int nchan,
                           int nbin, int nsum, bool big_endian, float *raw, int grid_cap)
{
    if (nsub < 1 || nchan < 1 || nbin < 1 || (nsum != 1 && nsum != 2)) return hipErrorInvalidValue;
    const size_t P = (size_t)nsub * nchan;
    if (nsum == 2) {
        if (big_endian) decode_q_dispatch<true, 2>(st, q, scl, offs, P, nchan, nbin, raw, grid_cap);
        else decode_q_dispatch<false, 2>(st, q, scl, offs, P, nchan, nbin, raw, grid_cap);
    } else {
        if (big_endian) decode_q_dispatch<true, 1>(st, q, scl, offs, P, nchan, nbin, raw, grid_cap);
        else decode_q_dispatch<false, 1>(st, q, scl, offs, P, nchan, nbin, raw, grid_cap);
    }
    return hipGetLastError();
}

namespace {
template <bool BE>
void encode_q_dispatch(hipStream_t st, const float *in, int nprof, int nbin, int16_t *q, float *scl, float *offs,
                       int grid_cap)
{
    // a block per profile; 16384 blocks of four waves cover the 256 CUs many times
    const dim3 grid(cap_grid(std::min<size_t>((size_t)nprof, 16384), grid_cap));
    const bool v4 = nbin % 4 == 0 && ((uintptr_t)in & 15) == 0;
    const bool v8 = v4 && nbin % 8 == 0 && ((uintptr_t)q & 15) == 0;
    if (v8) IC_GGL((k_encode_q<BE, true, true>), grid, dim3(256), 0, st, in, nprof, nbin, q, scl, offs);
    else if (v4) IC_GGL((k_encode_q<BE, true, false>), grid, dim3(256), 0, st, in, nprof, nbin, q, scl, offs);
    else IC_GGL((k_encode_q<BE, false, false>), grid, dim3(256), 0, st, in, nprof, nbin, q, scl, offs);
}
}  // namespace

hipError_t launch_encode_q(hipStream_t st, const float *in, int nprof, int nbin, bool big_endian, int16_t *q,
                           float *scl, float *offs, int grid_cap)
{
    if (nprof < 1 || nbin < 1) return hipErrorInvalidValue;
    if (big_endian) encode_q_dispatch<true>(st, in, nprof, nbin, q, scl, offs, grid_cap);
    else encode_q_dispatch<false>(st, in, nprof, nbin, q, scl, offs, grid_cap);
    return hipGetLastError();
}

namespace {
template <bool BE>
void residual_q_dispatch(hipStream_t st, const ResidualQArgs &a, size_t P)
{
    const dim3 grid(cap_grid(std::min<size_t>(P, 16384), a.grid_cap));
    const size_t lds = (((size_t)a.nbin + 3) & ~(size_t)3) * sizeof(float) + sizeof(QReduce);
    const PulseRegion pr{a.pr_on != 0, a.pr_start, a.pr_end, a.pr_factor};
    const bool v4 = a.nbin % 4 == 0 && ((uintptr_t)(a.D ? a.D : a.raw) & 15) == 0 && (!a.D || a.ldD % 4 == 0);
    const bool v8 = v4 && a.nbin % 8 == 0 && ((uintptr_t)a.q & 15) == 0;
#define IC_RESQ(V4, V8)                                                                                        \
    IC_GGL((k_residual_q<BE, V4, V8>), grid, dim3(256), lds, st, a.D, a.raw, a.base, a.T64, a.amp, a.info,     \
           a.shift, P, a.nchan, a.nbin, a.ldD, a.dtiled, pr, a.q, a.scl, a.offs)
    if (v8) IC_RESQ(true, true);
    else if (v4) IC_RESQ(true, false);
    else IC_RESQ(false, false);
#undef IC_RESQ
}
}  // namespace

hipError_t launch_residual_q(hipStream_t st, const ResidualQArgs &a)
{
    if (a.nsub < 1 || a.nchan < 1 || a.nbin < 1 || a.nbin > kResidualQMaxBin) return hipErrorInvalidValue;
    if (!a.D && (!a.raw || !a.base)) return hipErrorInvalidValue;
    const size_t P = (size_t)a.nsub * a.nchan;
    if (a.big_endian) residual_q_dispatch<true>(st, a, P);
    else residual_q_dispatch<false>(st, a, P);
    return hipGetLastError();
}

}  // namespace icgpu
