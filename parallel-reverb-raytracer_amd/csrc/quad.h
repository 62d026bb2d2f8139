// quad.h — data movement and votes inside a quad (lanes 4k .. 4k+3) or a pair of lanes by DPP quad_perm moves, never through memory.
// Shared by the trace stages (traversal.h) and the binning stages (attenuation.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// ---- DPP helpers: data movement inside a quad (lanes 4k .. 4k+3) --------------------------------
template <int CTRL> __device__ __forceinline__ uint32_t dpp_u(uint32_t v)
{
    return (uint32_t) __builtin_amdgcn_mov_dpp((int) v, CTRL, 0xF, 0xF, true);
}
template <int CTRL> __device__ __forceinline__ float dpp_f(float v) { return __uint_as_float(dpp_u<CTRL>(__float_as_uint(v))); }
template <int CTRL> __device__ __forceinline__ unsigned long long dpp_u64(unsigned long long v)
{
    return ((unsigned long long) dpp_u<CTRL>((uint32_t) (v >> 32)) << 32) | dpp_u<CTRL>((uint32_t) v);
}
#define QP_SWAP1 0xB1     // quad_perm [1,0,3,2]
#define QP_SWAP2 0x4E     // quad_perm [2,3,0,1]
#define QP_BCAST(k) ((k) * 0x55)
#define QP_PAIR_LO 0xA0   // quad_perm [0,0,2,2]: both lanes of a pair read its even lane
#define QP_PAIR_HI 0xF5   // quad_perm [1,1,3,3]: ... its odd lane
template <int K> __device__ __forceinline__ float quad_bcast_f(float v) { return dpp_f<QP_BCAST(K)>(v); }
template <int K> __device__ __forceinline__ uint32_t quad_bcast_u(uint32_t v) { return dpp_u<QP_BCAST(K)>(v); }

// does `pred` hold in any lane of this lane's quad?  Two DPP ORs (a 64-bit ballot masked per quad costs 64-bit VALU compares)
__device__ __forceinline__ bool quad_any(bool pred)
{
    uint32_t p = pred ? 1u : 0u;
    p |= (uint32_t) __builtin_amdgcn_mov_dpp((int) p, 0xB1, 0xF, 0xF, true);      // quad_perm [1,0,3,2]
    p |= (uint32_t) __builtin_amdgcn_mov_dpp((int) p, 0x4E, 0xF, 0xF, true);      // quad_perm [2,3,0,1]
    return p != 0;
}

// 4-bit mask of `pred` over this lane's quad
__device__ __forceinline__ uint32_t quad_ballot(bool pred)
{
    const unsigned long long m = __builtin_amdgcn_ballot_w64(pred);   // the condition mask itself, no 0/1 round trip through a VGPR
    return (uint32_t) (m >> (threadIdx.x & 60u)) & 0xFu;
}

}  // namespace
