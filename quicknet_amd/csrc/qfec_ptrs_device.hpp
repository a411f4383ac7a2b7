// qfec_ptrs_device.hpp -- what the kernels on tables of shard addresses share (qfec_ptrs.hip: encode,
// reconstruct; qfec_plan.hip: k_plan_apply_ptrs): reading an address out of the lane that loaded it,
// saying that it is global memory, and a wave's share of its group's shards.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

namespace qfec {

// v of lane l; l is wave-uniform
__device__ __forceinline__ uint64_t lane_value(uint64_t v, uint32_t l) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)l);
    return ((uint64_t)hi << 32) | lo;
}

// a table entry is an address in global memory: said so, the accesses are global_load / global_store
// and not the flat forms an address of unknown kind gets
typedef __attribute__((address_space(1))) uint8_t global_u8;
__device__ __forceinline__ const uint8_t* as_row(uint64_t p) { return (const uint8_t*)reinterpret_cast<const global_u8*>(p); }
__device__ __forceinline__ uint8_t* as_out(uint64_t p) { return (uint8_t*)reinterpret_cast<global_u8*>(p); }

// recon_column_by_e's row addresses: lane s of the wave holds the address of shard s
struct LaneRows {
    uint64_t mine;
    __device__ __forceinline__ uint8_t* operator()(uint8_t*, uint32_t l) const { return as_out(lane_value(mine, l)); }
};

// A wave's share of its group's shards.  vec(off): the lane's whole column of W bytes at byte off;
// byte(b): byte b.  Every access lies inside [0, block): a column ends at vcols * W <= block, the
// tail at tail0 + tailn = block, the byte span at min(slab end, block); the wpg slabs reach block.
// Args: PtrsArgs or PlanPtrsArgs (block, vcols, wpg, tail0, tailn of PtrsGeom).
template <int W, class Args, class Vec, class Byte>
__device__ __forceinline__ void run_slab(const Args& a, uint32_t slab, int lane, bool aligned, Vec&& vec,
                                         Byte&& byte) {
    if (aligned) {
        const uint32_t col = slab * 64u + lane;
        if (col < a.vcols) vec((uint64_t)col * W);
        if (slab + 1 == a.wpg && (uint32_t)lane < a.tailn) byte((uint64_t)a.tail0 + lane);
    } else {
        const uint32_t end = std::min((slab + 1) * 64u * W, a.block);
#pragma unroll 1
        for (uint32_t b = slab * 64u * W + lane; b < end; b += 64) byte((uint64_t)b);
    }
}

// the wave's group and slab; false past the last group
template <class Args>
__device__ __forceinline__ bool wave_item(const Args& a, uint64_t* g, uint32_t* slab) {
    const uint32_t wid = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    *g = wid / a.wpg;
    *slab = wid - (uint32_t)*g * a.wpg;
    return *g < a.groups;
}

}  // namespace qfec
