// Small helpers that more than one of the kernel files use. What only one file uses stays in that file.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pbsk {

// inclusive prefix sum over the 64 lanes of a wave (the block-wide scans of scan.hip and k_ring_control build on it)
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t n = __shfl_up(v, d, 64);
        if (lane >= d) v += n;
    }
    return v;
}

// four dwords in one load at any 4-byte alignment (k_pack's sources, the SHA-256 block requests)
typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

// Chunk data is read through GLOBAL-address-space pointers, never generic ones. A generic pointer compiles to flat_load,
// which counts in lgkmcnt as well as vmcnt; the producer's `s_waitcnt lgkmcnt(0)` in front of every s_barrier (its LDS
// writes must have landed) then also waits for the block it requested a moment ago, i.e. the FIFO's prefetch distance
// collapses to less than one step and the step time follows the slowest of the wave's 320 outstanding requests
// (rounds 3-5 shipped that; the address space is not inferred through the lambdas and the page select). global_load
// counts in vmcnt only.
#define PBSK_GLOBAL __attribute__((address_space(1)))
typedef const PBSK_GLOBAL u32x4_a4 *gvec4_ptr;
typedef const PBSK_GLOBAL uint32_t *gword_ptr;

// host side: raises the dynamic LDS that a launch of `kernel` may ask for to `bytes` (launch_pair, launch_ring_round)
template <typename K>
static hipError_t allow_lds(K kernel, size_t bytes) {
    return hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)bytes);
}

}  // namespace pbsk
