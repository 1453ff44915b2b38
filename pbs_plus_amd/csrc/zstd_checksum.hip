// The content checksum of zstd frames on the device, and whole zstd streams (pbsgpu_xxh64_many_device,
// pbsgpu_zstd_decode2_device, the checksum of pbsgpu_zstd_encode2_device; include/pbsgpu.h).
//
// The format lives in xxh64.h and zstd_stream.h, once, for these kernels and for the CPU build that runs under
// sanitizers. This file adds the cooperation between lanes:
//   k_xxh64_ranges  XXH64 of many ranges: one wave (a workgroup of 64) carries sixteen ranges, four lanes each, because
//                   the stripe loop is four independent serial chains: lane j of a quad takes word j of every 32-byte
//                   stripe, the quad's first lane merges, walks the tail and writes the hash. Workgroups stride over the
//                   ranges. The quads of a wave walk ranges of different lengths; they meet at the syncs behind the loop.
//   k_zstd_frames2  k_zstd_frames (zstd.hip) with the flags of pbsgpu_zstd_decode2_device: one wave per segment, the same
//                   State in LDS, pbsz::decode2 in place of decode_frame. The checksum of a frame runs INSIDE the wave, on
//                   its first four lanes, over the output the wave has just stored (sync() with its fences makes it
//                   loadable), so the verdict is the kernel's own and nothing is read back in between.
// Memory instructions: global_* and ds_* only, no scratch (tests/test_zstd_checksum_surface.py).
#include <algorithm>

#include "zstd_frames.h"
#include "zstd_stream.h"

using namespace pbse;

namespace pbsk {
namespace zstd {

struct QuadLanes {  // four lanes per range; the sixteen quads of the wave reach every sync together
    static __device__ __forceinline__ int lane() { return (int)(threadIdx.x & 3u); }
    static __device__ __forceinline__ int lanes() { return 4; }
    static __device__ __forceinline__ void sync() { __syncthreads(); }
    static __device__ __forceinline__ uint32_t uni(uint32_t v) { return v; }  // alike within a quad only
};

__global__ __launch_bounds__(64) void k_xxh64_ranges(const uint8_t *base, const pbsgpu_segment *ranges, uint32_t n, uint64_t seed,
                                                     uint64_t *out) {
    __shared__ uint64_t box[16][5];
    const uint32_t quad = threadIdx.x >> 2;
    for (uint32_t r0 = blockIdx.x * 16u; r0 < n; r0 += gridDim.x * 16u) {  // (r0 is the wave's: every lane makes every round)
        const uint32_t r = r0 + quad;
        pbsgpu_segment sg{0, 0};  // a quad behind the last range hashes nothing and writes nothing
        if (r < n) sg = ranges[r];
        const uint64_t h = pbsz::xxh64<QuadLanes>(base + sg.offset, sg.length, seed, box[quad]);
        if (r < n && (threadIdx.x & 3u) == 0) out[r] = h;
    }
}

// a value of the plan from LDS, known to be the same in all lanes; a pointer among them points to global memory
__device__ __forceinline__ uint32_t held(const uint32_t &v) { return WaveLanes::uni(v); }
template <class T>
__device__ __forceinline__ T *held(T *const &v) {
    const uint64_t a = (uint64_t)(uintptr_t)v;
    const uint64_t u = (uint64_t)WaveLanes::uni((uint32_t)a) | (uint64_t)WaveLanes::uni((uint32_t)(a >> 32)) << 32;
    return (T *)(__attribute__((address_space(1))) T *)(uintptr_t)u;
}

// The frame decoder inside leaves no scalar register free (k_zstd_frames: 0 spilled, none to spare), and this kernel holds
// more around it: the walk and the flags. So what k_zstd_frames holds in scalar registers across a frame, the plan, lies
// in LDS here, next to the walk (zstd_stream.h: Walk), and is read where it is used.
__global__ __launch_bounds__(64) void k_zstd_frames2(Plan plan, uint32_t flags) {
    __shared__ pbsz::State st;
    __shared__ pbsz::Walk w;
    __shared__ Plan pl;
    __shared__ uint32_t fl;
    if (WaveLanes::lane() == 0) {
        pl = plan;
        fl = flags;
    }
    __syncthreads();
    for (uint32_t f = blockIdx.x; f < held(pl.nframe); f += held(pl.stride)) {
        pbsz::walk_begin<WaveLanes>(w, held(fl));
        int r;
        do {  // the segment's place is read anew for every frame
            const Desc d = held(pl.desc)[f];  // (a uniform address: scalar loads)
            r = pbsz::walk_step<WaveLanes>(st, held(pl.src) + d.src_off, (uint32_t)d.src_len, held(pl.dst) + d.dst_off, (uint32_t)d.room,
                                           held(pl.lit) + (uint64_t)blockIdx.x * pbsz::kLitMax, w);
        } while (r == pbsz::MORE);
        if (WaveLanes::lane() == 0) held(pl.res)[f] = (uint64_t)(uint32_t)r << 32 | (r == pbsz::OK ? w.out : 0u);
        __syncthreads();  // State, the walk and the literal buffer go to the next segment
    }
}

hipError_t launch_frames2(const Plan &pl, uint32_t flags, hipStream_t st) {
    static_assert(PBSGPU_ZSTD_F_CHECKSUM == pbsz::F_CHECKSUM && PBSGPU_ZSTD_F_STREAM == pbsz::F_STREAM &&
                      PBSGPU_ZSTD_BAD_CHECKSUM == pbsz::BAD_CHECKSUM,
                  "the header's names for what zstd_stream.h decides");
    hipLaunchKernelGGL(k_zstd_frames2, dim3(pl.stride), dim3(64), 0, st, pl, flags);
    return hipGetLastError();
}

hipError_t launch_xxh64_ranges(const uint8_t *base, const pbsgpu_segment *ranges, uint32_t n, uint64_t seed, uint64_t *out,
                               int num_cus, hipStream_t st) {
    if (n == 0) return hipSuccess;
    const uint32_t grid = std::min<uint32_t>((n + 15) / 16, (uint32_t)num_cus * 8);
    hipLaunchKernelGGL(k_xxh64_ranges, dim3(grid), dim3(64), 0, st, base, ranges, n, seed, out);
    return hipGetLastError();
}

}  // namespace zstd
}  // namespace pbsk

extern "C" {

int pbsgpu_xxh64_many_device(pbsgpu_engine *e, const void *dptr, uint64_t nbytes, const pbsgpu_segment *segs, uint32_t nseg,
                             uint64_t seed, uint64_t *out) {
    if (!e || (!dptr && nbytes) || (nseg && (!segs || !out))) return PBSGPU_E_INVALID;
    if (!pbsp::ranges_ok(segs, nseg, nbytes)) return PBSGPU_E_INVALID;
    if (nseg == 0) return PBSGPU_OK;
    if (nbytes && !is_device_pointer(dptr)) return PBSGPU_E_INVALID;
    CHK(set_device(e));
    AuxLease lease(e);
    Slot *s = lease.s;
    const pbsgpu_segment *ranges = nullptr;
    CHK(put_table(s, segs, nseg, &ranges));
    uint64_t *hashes = s->take<uint64_t>(nseg);
    CHK(s->taken());
    HIPCHK(pbsk::zstd::launch_xxh64_ranges(static_cast<const uint8_t *>(dptr), ranges, nseg, seed, hashes, e->num_cus, s->stream));
    return fetch_result(s, out, hashes, (size_t)nseg * 8);  // the call's one synchronisation
}

}  // extern "C"
