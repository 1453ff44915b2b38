// What the two frame kernels of the zstd decoder share (zstd.hip: k_zstd_frames, one frame per segment, nothing verified;
// zstd_checksum.hip: k_zstd_frames2, checksums and whole streams): a segment's descriptor, the plan, the lanes' policy.
#pragma once

#include "engine_internal.h"
#include "zstd_decode.h"

namespace pbsk {
namespace zstd {

struct Desc {  // one frame: where it lies in src, and its room in dst (src_len = kSkip: no frame, the result says so)
    uint64_t src_off, src_len, dst_off, room;
};
constexpr uint64_t kSkip = ~0ull;

struct Plan {
    const uint8_t *src;
    const Desc *desc;  // nframe
    uint8_t *dst;
    uint8_t *lit;      // gridDim.x * kLitMax
    uint64_t *res;     // nframe: status << 32 | bytes decoded
    uint32_t nframe;
    uint32_t stride;   // = gridDim.x
};

struct WaveLanes {
    static __device__ __forceinline__ int lane() {
        int x = (int)threadIdx.x;
        asm volatile("" : "+v"(x));  // taken anew at every use: lane tests hoisted to the kernel's entry cost an SGPR pair each
        return x;
    }
    static __device__ __forceinline__ int lanes() { return 64; }
    static __device__ __forceinline__ void sync() { __syncthreads(); }
    static __device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
};

// zstd.hip: pl.stride workgroups of k_zstd_frames over descriptors the caller has made on the device (the AES leg of the
// restore, aes_gcm.hip: the frames of the encrypted-compressed blobs, decrypted into scratch)
hipError_t launch_frames(const Plan &pl, hipStream_t st);
// zstd_checksum.hip: pl.stride workgroups of k_zstd_frames2 with `flags` (PBSGPU_ZSTD_F_*, not 0)
hipError_t launch_frames2(const Plan &pl, uint32_t flags, hipStream_t st);
// zstd_checksum.hip: XXH64(base + ranges[i], seed) into out[i], i < n; ranges and out on the device. Enqueued, nothing
// synchronised.
hipError_t launch_xxh64_ranges(const uint8_t *base, const pbsgpu_segment *ranges, uint32_t n, uint64_t seed, uint64_t *out,
                               int num_cus, hipStream_t st);

}  // namespace zstd
}  // namespace pbsk
