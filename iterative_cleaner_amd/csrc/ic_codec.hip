// ic_codec.hip -- input preparation and the sample codec: pscrunch
// (k_pscrunch), the PSRFITS int16 decode (k_decode_q, k_decode_q_scalar) and
// encode (k_encode_q), with their launchers.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see Makefile).
// -ffp-contract=off is load-bearing: every f64/f32 operation below must be an
// individually rounded IEEE op in the order written, so that results equal
// numpy / scipy (MINPACK) bit-for-bit.  Explicit fma() is never used on an
// exact path.
#include <algorithm>
#include <math.h>

#include "ic_wave.h"

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

// One 256-lane block per profile, grid-stride over the profiles.  Pass 1: the
// block's minimum and maximum (16-byte loads when V4: nbin % 4 == 0), reduced
// in the wave by shuffles and across the four waves through LDS; every lane
// then derives the same scl / offs and lane 0 stores them.  Pass 2 reads the
// profile again (at most 32 KB, just read) and writes the samples, 8 per lane
// in one 16-byte store when V8 (nbin % 8 == 0), else one by one.
template <bool BE, bool V4, bool V8>
__global__ __launch_bounds__(256) void k_encode_q(const float *__restrict__ in, int nprof, int nbin,
                                                  int16_t *__restrict__ q, float *__restrict__ scl,
                                                  float *__restrict__ offs)
{
    __shared__ float s_mn[4], s_mx[4];
    __shared__ int s_nan[4];
    const int tid = threadIdx.x, wave = tid >> 6;
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
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float a = __shfl_xor(mn, off), b = __shfl_xor(mx, off);
            mn = a < mn ? a : mn;
            mx = b > mx ? b : mx;
            nan |= __shfl_xor(nan, off);
        }
        if ((tid & 63) == 0) {
            s_mn[wave] = mn;
            s_mx[wave] = mx;
            s_nan[wave] = nan;
        }
        __syncthreads();
        mn = s_mn[0];
        mx = s_mx[0];
        nan = s_nan[0];
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            mn = s_mn[w] < mn ? s_mn[w] : mn;
            mx = s_mx[w] > mx ? s_mx[w] : mx;
            nan |= s_nan[w];
        }
        __syncthreads();               // the next profile writes s_* again
        if (nan) mn = mx = NAN;
        const float fo = (float)__dmul_rn(0.5, __dadd_rn((double)mx, (double)mn));
        float fs = (float)__ddiv_rn(__dsub_rn((double)mx, (double)mn), 65534.0);
        if (!(fs > 0.0f && isfinite(fs))) fs = 1.0f;
        if (tid == 0) {
            scl[p] = fs;
            offs[p] = fo;
        }
        const double o = (double)fo, s = (double)fs;
        if (V8) {
            const float4 *s4 = (const float4 *)src;
            uint4 *dst = (uint4 *)(q + (size_t)p * nbin);
            for (int g = tid; g < nbin / 8; g += 256) {
                const float4 a = s4[2 * g], b = s4[2 * g + 1];
                dst[g] = make_uint4(q_pack<BE>(q_encode(a.x, o, s), q_encode(a.y, o, s)),
                                    q_pack<BE>(q_encode(a.z, o, s), q_encode(a.w, o, s)),
                                    q_pack<BE>(q_encode(b.x, o, s), q_encode(b.y, o, s)),
                                    q_pack<BE>(q_encode(b.z, o, s), q_encode(b.w, o, s)));
            }
        } else {
            uint16_t *dst = (uint16_t *)q + (size_t)p * nbin;
            for (int i = tid; i < nbin; i += 256) {
                uint32_t w = (uint32_t)q_encode(src[i], o, s) & 0xffffu;
                if (BE) w = ((w & 0xffu) << 8) | (w >> 8);
                dst[i] = (uint16_t)w;
            }
        }
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

}  // namespace icgpu
