// The small kernels that belong to no step of the hot path: publication into mapped host memory (k_publish*), the
// synthetic generator (k_fill), payload-stream assembly (k_pack). (Decomposition and the other kernel files: kernels.h.)
#include <algorithm>

#include "fill_word.h"
#include "kernel_util.h"
#include "kernels.h"

namespace pbsk {

// =====================================================================================
// small device -> host publication without the copy engines
// =====================================================================================
// hipMemcpyAsync(D2H) rides an SDMA queue that HIP streams share: a copy that has to wait for the kernel in front of
// it on ITS stream (e.g. "scalars after the 0.4 s SHA launch") parks at the head of that queue and every later copy
// of every other stream — another batch's segment-table upload, a stream window's record readback — waits behind it
// (measured: 380-430 ms stalls of a 3 KB readback while another stream's SHA kernel ran). Results that a host thread
// waits for are therefore WRITTEN by a kernel straight into mapped pinned host memory.
__global__ __launch_bounds__(256) void k_publish(uint32_t *dst, const uint32_t *src, uint64_t nwords) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nwords; i += stride) dst[i] = src[i];
}

// count-dependent form: publishes recs[0 .. *nrec) (12 words each, capped at cap records)
__global__ __launch_bounds__(256) void k_publish_records(uint32_t *dst, const uint32_t *src, const uint32_t *nrec,
                                                         uint64_t cap) {
    const uint64_t n = min((uint64_t)*nrec, cap) * (sizeof(pbsgpu_record) / 4);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dst[i] = src[i];
}

hipError_t launch_publish(void *dst_host_mapped, const void *src, uint64_t nbytes, hipStream_t st) {
    if (nbytes == 0) return hipSuccess;
    const uint64_t nwords = (nbytes + 3) / 4;
    unsigned blocks = (unsigned)std::min<uint64_t>((nwords + 255) / 256, 64);
    hipLaunchKernelGGL(k_publish, dim3(blocks), dim3(256), 0, st, (uint32_t *)dst_host_mapped, (const uint32_t *)src, nwords);
    return hipGetLastError();
}

hipError_t launch_publish_records(pbsgpu_record *dst_host_mapped, const pbsgpu_record *src, const uint32_t *nrec,
                                  uint64_t cap, hipStream_t st) {
    if (cap == 0) return hipSuccess;
    unsigned blocks = (unsigned)std::min<uint64_t>((cap * 12 + 255) / 256, 64);
    hipLaunchKernelGGL(k_publish_records, dim3(blocks), dim3(256), 0, st, (uint32_t *)dst_host_mapped, (const uint32_t *)src,
                       nrec, cap);
    return hipGetLastError();
}

// =====================================================================================
// synthetic corpus generator (twin of oracle_fill)
// =====================================================================================

__global__ __launch_bounds__(256) void k_fill(uint64_t *dst, uint64_t w0, uint64_t nwords, uint64_t seed,
                                              uint32_t kind, uint8_t *tail_dst, uint32_t tail_bytes) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nwords; i += stride)
        dst[i] = fill_word(w0 + i, seed, kind);
    if (blockIdx.x == 0 && threadIdx.x == 0 && tail_bytes) {
        const uint64_t w = fill_word(w0 + nwords, seed, kind);
        for (uint32_t b = 0; b < tail_bytes; ++b) tail_dst[b] = (uint8_t)(w >> (8 * b));
    }
}

hipError_t launch_fill(void *dptr, uint64_t stream_off, uint64_t nbytes, uint64_t seed, uint32_t kind,
                       hipStream_t st) {
    if (nbytes == 0) return hipSuccess;
    const uint64_t nwords = nbytes / 8;
    const uint32_t tail = (uint32_t)(nbytes & 7u);
    uint64_t blocks = (nwords + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    if (blocks == 0) blocks = 1;
    hipLaunchKernelGGL(k_fill, dim3((unsigned)blocks), dim3(256), 0, st, (uint64_t *)dptr, stream_off >> 3, nwords,
                       seed, kind, (uint8_t *)dptr + nwords * 8, tail);
    return hipGetLastError();
}

// =====================================================================================
// payload-stream assembly (pxar v2 split archive, .ppxar): [start marker] { [header 16 B][content] }* [tail]
// =====================================================================================
// One work item = one <= 4 MiB piece of one file (table built on the host, which knows the file
// list). A workgroup copies its piece with 16-byte stores to the (arbitrarily aligned) destination;
// sources are read as 4-byte-aligned dwords and funnel-shifted (v_alignbyte) into place.
__device__ __forceinline__ uint32_t load_shifted(const uint8_t *src) {  // 4 bytes at any alignment
    const uint32_t o = (uint32_t)((uintptr_t)src & 3u);
    const uint32_t *a = reinterpret_cast<const uint32_t *>(src - o);
    const uint32_t lo = a[0];
    if (o == 0) return lo;
    return __builtin_amdgcn_alignbyte(a[1], lo, o);
}

__global__ __launch_bounds__(256) void k_pack(const uint8_t *src_base, uint8_t *dst, const PackItem *items,
                                              uint32_t nitems) {
    const uint32_t it = blockIdx.x;
    if (it >= nitems) return;
    const PackItem w = items[it];
    uint8_t *d = dst + w.dst_off;
    if (w.kind != 0) {  // 16-byte header / marker: {type u64 LE, size u64 LE}
        if (threadIdx.x < 16) {
            const uint64_t v = (threadIdx.x < 8) ? w.src_off /* type */ : w.len /* size field */;
            d[threadIdx.x] = (uint8_t)(v >> (8 * (threadIdx.x & 7)));
        }
        return;
    }
    const uint8_t *sp = src_base + w.src_off;
    const uint64_t n = w.len;
    // head: bytes until the destination is 16-byte aligned
    uint64_t head = (16 - ((uintptr_t)d & 15u)) & 15u;
    if (head > n) head = n;
    if (threadIdx.x < head) d[threadIdx.x] = sp[threadIdx.x];
    const uint64_t body = (n - head) / 16;
    const uint8_t *sb = sp + head;
    uint8_t *db = d + head;
    for (uint64_t i = threadIdx.x; i < body; i += blockDim.x) {
        const uint8_t *q = sb + i * 16;
        uint4 v;
        if ((((uintptr_t)q) & 3u) == 0) {
            const u32x4_a4 t = *reinterpret_cast<const u32x4_a4 *>(q);
            v = make_uint4(t.x, t.y, t.z, t.w);
        } else {
            v = make_uint4(load_shifted(q), load_shifted(q + 4), load_shifted(q + 8), load_shifted(q + 12));
        }
        *reinterpret_cast<uint4 *>(db + i * 16) = v;
    }
    const uint64_t done = head + body * 16;
    const uint64_t tail = n - done;
    if (threadIdx.x < tail) d[done + threadIdx.x] = sp[done + threadIdx.x];
}

hipError_t launch_pack(const uint8_t *src_base, uint8_t *dst, const PackItem *items, uint32_t nitems, hipStream_t st) {
    if (nitems == 0) return hipSuccess;
    hipLaunchKernelGGL(k_pack, dim3(nitems), dim3(256), 0, st, src_base, dst, items, nitems);
    return hipGetLastError();
}

}  // namespace pbsk
