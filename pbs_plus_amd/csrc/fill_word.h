// The synthetic corpus generator (twin of oracle_fill): a pure function of (seed, kind, stream offset), whoever writes
// the bytes: k_fill (misc_kernels.hip) and the page ring's refill k_ring_fill (ring_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pbsk {

__device__ __forceinline__ uint64_t splitmix64(uint64_t seed, uint64_t idx) {
    uint64_t z = seed + (idx + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// kind 4: 16-byte blocks from two ChaCha quarter-rounds over {block index, seed}: adds / xors / rotates only (24 full-rate
// VALU ops per 16 bytes; splitmix64's two 64-bit multiplies cost ~6 ops per BYTE at quarter rate). The page ring's refill
// runs inside the timed region on the few CUs the SHA service leaves free, so the generator has to be cheap.
__device__ __forceinline__ uint4 chacha2_block(uint64_t q, uint64_t seed) {
    uint32_t x0 = (uint32_t)q ^ 0x61707865u, x1 = (uint32_t)(q >> 32) ^ 0x3320646eu;
    uint32_t x2 = (uint32_t)seed ^ 0x79622d32u, x3 = (uint32_t)(seed >> 32) ^ 0x6b206574u;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        x0 += x1; x3 = __builtin_rotateleft32(x3 ^ x0, 16);
        x2 += x3; x1 = __builtin_rotateleft32(x1 ^ x2, 12);
        x0 += x1; x3 = __builtin_rotateleft32(x3 ^ x0, 8);
        x2 += x3; x1 = __builtin_rotateleft32(x1 ^ x2, 7);
    }
    return make_uint4(x0, x1, x2, x3);
}

__device__ __forceinline__ uint64_t fill_word(uint64_t widx, uint64_t seed, uint32_t kind) {
    switch (kind) {
    case 0: return splitmix64(seed, widx);
    case 4: {
        const uint4 b = chacha2_block(widx >> 1, seed);
        return (widx & 1u) ? ((uint64_t)b.w << 32) | b.z : ((uint64_t)b.y << 32) | b.x;
    }
    case 1: return 0;
    case 2: return splitmix64(seed, widx & 511u);
    default: {
        const uint64_t g = widx >> 13;
        const uint64_t r = splitmix64(seed ^ 0xA5A5A5A55A5A5A5Aull, g);
        if ((((r >> 32) * 10u) >> 32) < 3u) return 0;
        return splitmix64(seed, widx);
    }
    }
}

}  // namespace pbsk
