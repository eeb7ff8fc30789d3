// ic_wave.h -- device-only wave primitives, included by every kernel unit
// (ic_template.hip, ic_codec.hip, ic_fit.hip, ic_diag.hip, ic_rotate.hip,
// ic_linestats.hip, ic_shards.hip): the
// wave-level LDS ordering, the DPP / readlane trees and their functors, the
// round list of the exact fit (read by the fit, the diagnostics and the
// rotation), the LDS address cast and the 4-float vector type of the 16-byte
// loads.  All forced inline: a unit gets no function of its own from here.
#pragma once
#include <stdint.h>

#include "ic_internal.h"

namespace icgpu {

typedef float fv4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t lds_u32(const void *p)
{
    return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void *)p;
}

// LDS ordering between lanes of ONE wave: DS instructions of a wave execute in
// order, so only compiler reordering must be prevented (no s_barrier).
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- cross-lane trees on DPP + readlane (VALU latency, no LDS crossbar) ----
// Level m of an xor-butterfly pairs lane groups [0,m) and [m,2m).  Within a
// row of 16 that is quad_perm (m = 1, 2), row_half_mirror (m = 4) and
// row_mirror (m = 8): after level m every lane of a group of m holds the same
// value, so a mirror delivers the partner group's value.  The last two levels
// combine lanes 0, 16, 32, 48 read into scalars, in tree order.  The result is
// wave-uniform.  (IEEE add/max/min are commutative: a lane adding its partner's
// value gets the same bits as the partner adding its own.)
constexpr int kDppXor1 = 0xB1, kDppXor2 = 0x4E, kDppHalfMirror = 0x141, kDppMirror = 0x140;

template <int CTRL>
__device__ __forceinline__ float dpp(float v)
{
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xf, 0xf, true));
}
template <int CTRL>
__device__ __forceinline__ int dpp(int v)
{
    return __builtin_amdgcn_mov_dpp(v, CTRL, 0xf, 0xf, true);
}
// (every lane reads an in-range lane for these controls, so the f64 form needs
// no `old` operand: mov_dpp saves the two zeroing moves per level)
template <int CTRL>
__device__ __forceinline__ double dpp(double v)
{
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ float lane_read(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
__device__ __forceinline__ int lane_read(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ double lane_read(double v, int l)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l),
                            __builtin_amdgcn_readlane(__double2loint(v), l));
}

// tree over lanes [0, ACT) (ACT a power of two <= 64), uniform result
template <int ACT, typename T, typename Op>
__device__ __forceinline__ T wave_tree(T v, Op op)
{
    if (ACT >= 2) v = op(v, dpp<kDppXor1>(v));
    if (ACT >= 4) v = op(v, dpp<kDppXor2>(v));
    if (ACT >= 8) v = op(v, dpp<kDppHalfMirror>(v));
    if (ACT >= 16) v = op(v, dpp<kDppMirror>(v));
    if (ACT == 64) return op(op(lane_read(v, 0), lane_read(v, 16)), op(lane_read(v, 32), lane_read(v, 48)));
    if (ACT == 32) return op(lane_read(v, 0), lane_read(v, 16));
    return lane_read(v, 0);
}

struct OpAdd {
    template <typename T>
    __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct OpMaxF {
    __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); }
    __device__ __forceinline__ double operator()(double a, double b) const { return fmax(a, b); }
};
struct OpMinF {
    __device__ __forceinline__ float operator()(float a, float b) const { return fminf(a, b); }
    __device__ __forceinline__ double operator()(double a, double b) const { return fmin(a, b); }
};
struct OpOr {
    __device__ __forceinline__ int operator()(int a, int b) const { return a | b; }
};

// A round's input list.  k_fit_state writes the survivors of a round into the
// P-entry list buffer partitioned by request: A requests from the front
// (list[0 .. nA)), B requests from the end down (list[P - 1 - j], j < nB), so
// that the next round's waves hold one kind each (a wave with both runs both
// sweep bodies; round 0's unanswered B requests and the profiles one stage
// behind after them would otherwise spread over most waves).  Both counts
// share one 64-bit word, [63:32] nB and [31:0] nA, so that one atomic per
// block returns both list offsets; the blocks that finished are counted in a
// word of their own (k_fit_state).
__host__ __device__ constexpr unsigned long long rl_pack(unsigned long long nB, unsigned long long nA)
{
    return (nB << 32) | nA;
}
struct RoundList {
    const int32_t *list;
    long nA, nB, P;
    __device__ __forceinline__ RoundList(const int32_t *l, const unsigned long long *ctr, long P_) : list(l), P(P_)
    {
        if (!l) {
            nA = P_;
            nB = 0;
        } else {
            const unsigned long long v = *ctr;
            nA = (long)(v & 0xffffffffull);
            nB = (long)(v >> 32);
        }
    }
    __device__ __forceinline__ long n() const { return nA + nB; }
    __device__ __forceinline__ long at(long s) const
    {
        if (!list) return s;
        return s < nA ? (long)list[s] : (long)list[P - 1 - (s - nA)];
    }
};

}  // namespace icgpu
