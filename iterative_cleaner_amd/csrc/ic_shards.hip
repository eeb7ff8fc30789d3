// ic_shards.hip -- pack / unpack kernels of the shard exchanges (row and
// channel shards), with their launchers.
#include <algorithm>
#include <float.h>
#include <math.h>

#include "ic_wave.h"

namespace icgpu {

// ============================================================ shard exchanges

// owner rank of subint row s / channel c (world <= 64: linear scan)
__device__ __forceinline__ int geom_row_owner(const ShardGeom &g, int s)
{
    int r = 0;
    while (r + 1 < g.world && s >= g.row0[r + 1]) ++r;
    return r;
}
__device__ __forceinline__ int geom_chan_owner(const ShardGeom &g, int c)
{
    int r = 0;
    while (r + 1 < g.world && c >= g.chan0[r + 1]) ++r;
    return r;
}

// Send blocks to row owners.  Destination d receives, for its rows
// [row0[d], row0[d+1]) x my nchan_loc channels, the fields back to back:
// std, mean, fft (f64), ptp (f32)  — or, in valid mode, valid (u8).
// Blocks are padded to 8 bytes (shard_block_bytes); d's block starts after
// the blocks of d' < d.
__global__ __launch_bounds__(256) void k_pack_rows(ShardGeom g, int nchan_loc, const double *__restrict__ std_d,
                                                   const double *__restrict__ mean_d, const double *__restrict__ fft_d,
                                                   const double *__restrict__ ptp_d, const uint8_t *__restrict__ valid,
                                                   unsigned char *__restrict__ send)
{
    const size_t P = (size_t)g.nsub * nchan_loc;
    const size_t esz = valid ? 1 : 32;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < P; k += (size_t)gridDim.x * blockDim.x) {
        const int s = (int)(k / nchan_loc);
        const int d = geom_row_owner(g, s);
        const size_t n_d = (size_t)(g.row0[d + 1] - g.row0[d]) * nchan_loc;   // elements in d's block
        const size_t e = k - (size_t)g.row0[d] * nchan_loc;                   // element within it
        size_t off = 0;
        for (int q = 0; q < d; ++q) off += shard_block_bytes((size_t)(g.row0[q + 1] - g.row0[q]) * nchan_loc, esz);
        unsigned char *blk = send + off;
        if (valid) {
            blk[e] = valid[k];
        } else {
            ((double *)blk)[e] = std_d[k];
            ((double *)blk)[n_d + e] = mean_d[k];
            ((double *)blk)[2 * n_d + e] = fft_d[k];
            ((double *)blk)[3 * n_d + e] = ptp_d[k];
        }
    }
}

// Owned rows from the per-source blocks (source p sent rows_own x nchan_p
// elements per field, after the padded blocks of sources p' < p).
__global__ __launch_bounds__(256) void k_assemble_rows(ShardGeom g, const unsigned char *__restrict__ recv,
                                                       double *__restrict__ std_r, double *__restrict__ mean_r,
                                                       double *__restrict__ fft_r, double *__restrict__ ptp_r,
                                                       uint8_t *__restrict__ valid_r)
{
    const int rows = g.row0[g.rank + 1] - g.row0[g.rank];
    const size_t n = (size_t)rows * g.nchan_g;
    const size_t esz = valid_r ? 1 : 32;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (size_t)gridDim.x * blockDim.x) {
        const int r = (int)(k / g.nchan_g), c = (int)(k % g.nchan_g);
        const int p = geom_chan_owner(g, c);
        const int np = g.chan0[p + 1] - g.chan0[p];
        const size_t n_p = (size_t)rows * np;
        const size_t e = (size_t)r * np + (c - g.chan0[p]);
        size_t off = 0;
        for (int q = 0; q < p; ++q) off += shard_block_bytes((size_t)rows * (g.chan0[q + 1] - g.chan0[q]), esz);
        const unsigned char *blk = recv + off;
        if (valid_r) {
            valid_r[k] = blk[e];
        } else {
            std_r[k] = ((const double *)blk)[e];
            mean_r[k] = ((const double *)blk)[n_p + e];
            fft_r[k] = ((const double *)blk)[2 * n_p + e];
            ptp_r[k] = ((const double *)blk)[3 * n_p + e];
        }
    }
}

// gathered row statistics: rank p's slot (8 * rows_pad doubles) holds med
// [4][rows_p] then mad [4][rows_p] of its rows_p owned rows
__global__ __launch_bounds__(256) void k_unpack_rowstats(ShardGeom g, int rows_pad, const double *__restrict__ recv,
                                                         double *__restrict__ row_med, double *__restrict__ row_mad)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;   // q * nsub + s
    if (k >= 4 * g.nsub) return;
    const int q = k / g.nsub, s = k % g.nsub;
    const int p = geom_row_owner(g, s);
    const int rows_p = g.row0[p + 1] - g.row0[p];
    const int r = s - g.row0[p];
    const double *slot = recv + (size_t)p * 8 * rows_pad;
    row_med[k] = slot[q * rows_p + r];
    row_mad[k] = slot[4 * rows_p + q * rows_p + r];
}

// gathered detrended row statistics (ic_shard_enable_detrend): rank p's slot
// (rows_pad * (8 + 16 ms) doubles) holds med [4][rows_p], mad [4][rows_p], then
// the coefficients [4][rows_p][ms][4] of its rows_p owned rows.  One entry per
// (diagnostic, subint, piece): its four coefficients, and the piece 0 entry its
// row's median and MAD
__global__ __launch_bounds__(256) void k_unpack_rowtrends(ShardGeom g, int rows_pad, int ms,
                                                          const double *__restrict__ recv,
                                                          double *__restrict__ row_med, double *__restrict__ row_mad,
                                                          double *__restrict__ row_coef)
{
    const size_t n = (size_t)4 * g.nsub * ms;
    const size_t slot_n = (size_t)rows_pad * (8 + 16 * (size_t)ms);
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (size_t)gridDim.x * blockDim.x) {
        const int m = (int)(k % ms);
        const int qs = (int)(k / ms);   // q * nsub + s
        const int q = qs / g.nsub, s = qs % g.nsub;
        const int p = geom_row_owner(g, s);
        const int rows_p = g.row0[p + 1] - g.row0[p];
        const int r = s - g.row0[p];
        const double *slot = recv + (size_t)p * slot_n;
        const double *src = slot + 8 * (size_t)rows_p + (((size_t)q * rows_p + r) * ms + m) * 4;
        double *dst = row_coef + k * 4;
        dst[0] = src[0];
        dst[1] = src[1];
        dst[2] = src[2];
        dst[3] = src[3];
        if (m == 0) {
            row_med[qs] = slot[q * rows_p + r];
            row_mad[qs] = slot[4 * rows_p + q * rows_p + r];
        }
    }
}

// Window positions gathered from the row owners (blocks of `blk` ints per
// rank) -> win[nsub] on every rank; flags (optional): moved per subint and the
// moves counter flags[nsub], as k_window does unsharded.
__global__ __launch_bounds__(256) void k_unpack_windows(ShardGeom g, int blk, const int32_t *__restrict__ recv,
                                                        int32_t *__restrict__ win, int32_t *__restrict__ flags)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= g.nsub) return;
    const int p = geom_row_owner(g, s);
    const int w = recv[(size_t)p * blk + (s - g.row0[p])];
    if (flags) {
        const int moved = win[s] != w;
        flags[s] = moved;
        if (moved) atomicAdd(&flags[g.nsub], 1);
    }
    win[s] = w;
}

// fscrunch rows gathered from the row owners: rank p's block (blk floats) holds
// F rows [rows_pad][nbin] then wf [rows_pad] -> F[nsub][nbin], wf[nsub]
__global__ __launch_bounds__(256) void k_unpack_fscrunch(ShardGeom g, int rows_pad, long blk, int nbin,
                                                         const float *__restrict__ recv, float *__restrict__ F,
                                                         float *__restrict__ wf)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int s = blockIdx.y;
    if (i >= nbin) return;
    const int p = geom_row_owner(g, s);
    const float *b = recv + (size_t)p * blk;
    const int t = s - g.row0[p];
    F[(size_t)s * nbin + i] = b[(size_t)t * nbin + i];
    if (i == 0) wf[s] = b[(size_t)rows_pad * nbin + t];
}

__global__ void k_sum_i32(const int32_t *__restrict__ gathered, int world, int n, int32_t *__restrict__ buf)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int32_t a = 0;
    for (int r = 0; r < world; ++r) a += gathered[(size_t)r * n + i];
    buf[i] = a;
}

// ============================================================ launchers

hipError_t launch_unpack_windows(hipStream_t st, const ShardGeom &g, int blk, const int32_t *recv, int32_t *win,
                                 int32_t *flags)
{
    IC_GGL(k_unpack_windows, dim3(cdiv(g.nsub, 256)), dim3(256), 0, st, g, blk, recv, win, flags);
    return hipGetLastError();
}

hipError_t launch_unpack_fscrunch(hipStream_t st, const ShardGeom &g, int rows_pad, long blk, int nbin,
                                  const float *recv, float *F, float *wf)
{
    const int bs = bin_block(nbin);
    IC_GGL(k_unpack_fscrunch, dim3(cdiv(nbin, bs), g.nsub), dim3(bs), 0, st, g, rows_pad, blk, nbin,
                       recv, F, wf);
    return hipGetLastError();
}

hipError_t launch_pack_rows(hipStream_t st, const ShardGeom &g, int nchan_loc, const double *std_d,
                            const double *mean_d, const double *fft_d, const double *ptp_d, const uint8_t *valid,
                            unsigned char *send, int grid_cap)
{
    const size_t P = (size_t)g.nsub * nchan_loc;
    if (P == 0) return hipSuccess;
    const unsigned grid = cap_grid(std::min<unsigned>(cdiv(P, 256), 4096), grid_cap);
    IC_GGL(k_pack_rows, dim3(grid), dim3(256), 0, st, g, nchan_loc, std_d, mean_d, fft_d, ptp_d, valid, send);
    return hipGetLastError();
}

hipError_t launch_assemble_rows(hipStream_t st, const ShardGeom &g, const unsigned char *recv, double *std_r,
                                double *mean_r, double *fft_r, double *ptp_r, uint8_t *valid_r, int grid_cap)
{
    const size_t n = (size_t)(g.row0[g.rank + 1] - g.row0[g.rank]) * g.nchan_g;
    if (n == 0) return hipSuccess;
    const unsigned grid = cap_grid(std::min<unsigned>(cdiv(n, 256), 4096), grid_cap);
    IC_GGL(k_assemble_rows, dim3(grid), dim3(256), 0, st, g, recv, std_r, mean_r, fft_r, ptp_r, valid_r);
    return hipGetLastError();
}

hipError_t launch_unpack_rowstats(hipStream_t st, const ShardGeom &g, int rows_pad, const double *recv,
                                  double *row_med, double *row_mad)
{
    IC_GGL(k_unpack_rowstats, dim3(cdiv(4 * (size_t)g.nsub, 256)), dim3(256), 0, st, g, rows_pad, recv,
                       row_med, row_mad);
    return hipGetLastError();
}

hipError_t launch_unpack_rowtrends(hipStream_t st, const ShardGeom &g, int rows_pad, int ms, const double *recv,
                                   double *row_med, double *row_mad, double *row_coef, int grid_cap)
{
    if (ms < 1 || ms > kMaxPieces) return hipErrorInvalidValue;
    const size_t n = (size_t)4 * g.nsub * ms;
    if (n == 0) return hipSuccess;
    const unsigned grid = cap_grid(std::min<size_t>(cdiv(n, 256), 4096), grid_cap);
    IC_GGL(k_unpack_rowtrends, dim3(grid), dim3(256), 0, st, g, rows_pad, ms, recv, row_med, row_mad, row_coef);
    return hipGetLastError();
}

hipError_t launch_sum_i32(hipStream_t st, const int32_t *gathered, int world, int n, int32_t *buf)
{
    IC_GGL(k_sum_i32, dim3(cdiv(n, 64)), dim3(64), 0, st, gathered, world, n, buf);
    return hipGetLastError();
}

}  // namespace icgpu
