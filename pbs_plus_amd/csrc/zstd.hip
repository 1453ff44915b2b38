// Zstandard frames on the device (pbsgpu_zstd_decode_device, include/pbsgpu.h): the chunks of a datastore
// written by the stock client are zstd frames, one per blob.
//
// The format lives in zstd_decode.h, once, for this kernel and for the CPU build that is fuzzed. This file adds what that
// header leaves open, the cooperation between lanes:
//   k_zstd_frames  one wave (a workgroup of 64) per frame, workgroups striding over the frames. The wave's State — the
//                  8 KiB Huffman table, 5 KiB of FSE tables, the batch of 64 resolved sequences, the build scratch — is
//                  the workgroup's LDS (16 244 bytes: ten workgroups fit a CU's 160 KiB). All 64 lanes walk decode_frame
//                  together. Lane 0 does what is serial by nature (table builds; the FSE chain of the sequences with its
//                  states, extra bits and repeat offsets, and every bound check) and leaves its results in LDS; the four
//                  Huffman streams of a literals section run on lanes 0-3 into the workgroup's 128 KiB literal buffer in
//                  global memory; literal runs, matches, raw and RLE blocks are copied and filled by all lanes.
//   sync()         a workgroup barrier with its release/acquire fences: a match reads bytes that other lanes of the wave
//                  stored a few instructions earlier, and a wave's loads are not ordered behind its own earlier stores
//                  to other lanes' addresses without the wait the fence brings. decode_block places it before a match
//                  whose source reaches into bytes stored since the last one, not before every match.
// Memory instructions: global_* and ds_* only (the pointers come from the kernel arguments; State is __shared__), no
// scratch, no dynamically indexed private arrays (tests/test_zstd_surface.py).
#include <algorithm>
#include <cstring>
#include <vector>

#include "zstd_frames.h"

using namespace pbse;

namespace pbsk {
namespace zstd {

// (Desc, Plan, WaveLanes: zstd_frames.h, shared with k_zstd_frames2 of zstd_checksum.hip)

__global__ __launch_bounds__(64) void k_zstd_frames(Plan pl) {
    __shared__ pbsz::State st;
    uint8_t *lit = pl.lit + (uint64_t)blockIdx.x * pbsz::kLitMax;
    for (uint32_t f = blockIdx.x; f < pl.nframe; f += pl.stride) {
        const Desc d = pl.desc[f];  // (a uniform address: scalar loads)
        uint32_t decoded = 0;
        int r = (int)kNotDecoded;
        if (d.src_len != kSkip)
            r = pbsz::decode_frame<WaveLanes>(st, pl.src + d.src_off, (uint32_t)d.src_len, pl.dst + d.dst_off, (uint32_t)d.room, lit,
                                              &decoded);
        if (threadIdx.x == 0) pl.res[f] = (uint64_t)(uint32_t)r << 32 | decoded;
        __syncthreads();  // State and the literal buffer go to the next frame
    }
}

// ---- the zstd leg of the restore (pbsgpu_blob_decode2_device; planned and enqueued by blob.hip) -------------------------
//   k_zr_select  per distinct blob: a blob of the compressed kind whose computed CRC is the stored one becomes a frame for
//                k_zstd_frames, into its planned room; every other blob is skipped there (kNotDecoded)
//   k_zr_ranges  per distinct blob, after the decode: the range the SHA-256 pass hashes
//   k_zr_copy    the entries whose bytes do not lie where the frame was decoded: clipped ones, fan-out, scratch -> dst
//   k_zr_status  per entry of a decoded blob: frame, size, digest
typedef const __attribute__((address_space(1))) uint32_t *zword_ptr;

__global__ __launch_bounds__(256) void k_zr_select(RestorePlan pl, Desc *desc) {
    const uint32_t u = blockIdx.x * 256 + threadIdx.x;
    if (u >= pl.nu) return;
    const uint32_t hk = pl.info[2 * (uint64_t)u], stored = pl.info[2 * (uint64_t)u + 1];
    const bool take = hk == (PBSGPU_BLOB_HEADER_SIZE | PBSGPU_BLOB_COMPRESSED << 8) && pl.crcs[u] == stored;
    const pbsgpu_segment b = pl.blobs[u];
    const RestoreJob job = pl.jobs[u];
    desc[u] = Desc{b.offset + PBSGPU_BLOB_HEADER_SIZE, take ? b.length - PBSGPU_BLOB_HEADER_SIZE : kSkip, job.place, job.room};
}

__global__ __launch_bounds__(256) void k_zr_ranges(RestorePlan pl) {
    const uint32_t u = blockIdx.x * 256 + threadIdx.x;
    if (u >= pl.nu) return;
    const uint64_t res = pl.res[u];
    pl.sha[u] = pbsgpu_segment{pl.jobs[u].place, (res >> 32) == PBSGPU_ZSTD_OK ? (uint32_t)res : 0u};
}

// blockIdx.y strides over the copies, x over a copy's bytes
__global__ __launch_bounds__(256) void k_zr_copy(RestorePlan pl) {
    for (uint32_t i = blockIdx.y; i < pl.ncopy; i += gridDim.y) {
        const RestoreCopy c = pl.copies[i];
        if (pl.res[c.u] != (uint64_t)c.size) continue;  // status OK and exactly the entry's size
        const uint8_t *from = pl.dst + c.from;
        uint8_t *to = pl.dst + c.to;
        for (uint32_t k = blockIdx.x * 256 + threadIdx.x; k < c.len; k += gridDim.x * 256) to[k] = from[k];
    }
}

__global__ __launch_bounds__(256) void k_zr_status(RestorePlan pl) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= pl.nidx) return;
    const uint32_t u = pl.ents[2 * (uint64_t)i], size = pl.ents[2 * (uint64_t)i + 1];
    const uint64_t res = pl.res[u];
    const uint32_t zs = (uint32_t)(res >> 32);
    if (zs == kNotDecoded) return;  // blob.hip's status stands
    uint8_t r;
    if (zs == PBSGPU_ZSTD_BAD_FRAME || zs == PBSGPU_ZSTD_UNSUPPORTED) {
        r = PBSGPU_BLOB_BAD_DATA;
    } else if (zs != PBSGPU_ZSTD_OK || (uint32_t)res != size) {
        r = PBSGPU_BLOB_BAD_SIZE;
    } else {
        r = PBSGPU_BLOB_OK;
        if (pl.recs) {
            const zword_ptr want = (zword_ptr)(pl.recs + 48ull * i + 8), got = (zword_ptr)(pl.digs + 32ull * u);
            uint32_t diff = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) diff |= want[j] ^ got[j];
            if (diff) r = PBSGPU_BLOB_BAD_DIGEST;
        }
    }
    pl.status[i] = r;
}

hipError_t launch_restore_frames(const RestorePlan &pl, void *desc, hipStream_t st) {
    static_assert(kLitBytes == pbsz::kLitMax, "the literal scratch blob.hip plans for");
    static_assert(kDescBytes == sizeof(Desc), "the frame descriptors blob.hip makes room for");
    hipLaunchKernelGGL(k_zr_select, dim3((pl.nu + 255) / 256), dim3(256), 0, st, pl, static_cast<Desc *>(desc));
    Plan fp{};
    fp.src = pl.src;
    fp.desc = static_cast<const Desc *>(desc);
    fp.dst = pl.dst;
    fp.lit = pl.lit;
    fp.res = pl.res;
    fp.nframe = pl.nu;
    fp.stride = pl.stride;
    hipLaunchKernelGGL(k_zstd_frames, dim3(pl.stride), dim3(64), 0, st, fp);
    hipLaunchKernelGGL(k_zr_ranges, dim3((pl.nu + 255) / 256), dim3(256), 0, st, pl);
    return hipGetLastError();
}

hipError_t launch_frames(const Plan &pl, hipStream_t st) {
    hipLaunchKernelGGL(k_zstd_frames, dim3(pl.stride), dim3(64), 0, st, pl);
    return hipGetLastError();
}

hipError_t launch_restore_copy(const RestorePlan &pl, uint32_t longest, int num_cus, hipStream_t st) {
    const uint32_t gx = std::max<uint32_t>(1, std::min<uint32_t>((longest + 4095) / 4096, (uint32_t)num_cus * 8));
    hipLaunchKernelGGL(k_zr_copy, dim3(gx, std::min<uint32_t>(pl.ncopy, 1024)), dim3(256), 0, st, pl);
    return hipGetLastError();
}

hipError_t launch_restore_status(const RestorePlan &pl, hipStream_t st) {
    hipLaunchKernelGGL(k_zr_status, dim3((pl.nidx + 255) / 256), dim3(256), 0, st, pl);
    return hipGetLastError();
}

}  // namespace zstd
}  // namespace pbsk

namespace {

using pbsk::zstd::Desc;
using pbsk::zstd::Plan;

int zstd_decode(pbsgpu_engine *e, const void *src, uint64_t nbytes, const pbsgpu_segment *frames, uint32_t nframe,
                const pbsgpu_segment *out, void *dst, uint64_t dst_cap, uint8_t *status, uint64_t *decoded, uint32_t flags) {
    if (!e || (flags & ~(uint32_t)(PBSGPU_ZSTD_F_CHECKSUM | PBSGPU_ZSTD_F_STREAM))) return PBSGPU_E_INVALID;
    if (nframe == 0) return PBSGPU_OK;
    if (!frames || !out || !status || (!src && nbytes) || (!dst && dst_cap)) return PBSGPU_E_INVALID;
    uint64_t lo = ~0ull, hi = 0;  // the part of dst the call may write
    for (uint32_t i = 0; i < nframe; ++i) {
        if ((frames[i].length | out[i].length) >> 32) return PBSGPU_E_INVALID;  // a chunk is 16 MiB at the most
        if (frames[i].length > nbytes || frames[i].offset > nbytes - frames[i].length) return PBSGPU_E_INVALID;
        if (out[i].length > dst_cap || out[i].offset > dst_cap - out[i].length) return PBSGPU_E_INVALID;
        if (out[i].length) {
            lo = std::min(lo, out[i].offset);
            hi = std::max(hi, out[i].offset + out[i].length);
        }
    }
    std::vector<uint32_t> order;
    for (uint32_t i = 0; i < nframe; ++i)
        if (out[i].length) order.push_back(i);
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return out[a].offset < out[b].offset; });
    for (size_t k = 1; k < order.size(); ++k)
        if (out[order[k - 1]].offset + out[order[k - 1]].length > out[order[k]].offset) return PBSGPU_E_INVALID;
    if (hi > lo && pbsp::overlaps(static_cast<const uint8_t *>(dst) + lo, hi - lo, src, nbytes))
        return PBSGPU_E_INVALID;  // a destination inside the source
    CHK(set_device(e));
    if ((nbytes && !is_device_pointer(src)) || (hi > lo && !is_device_pointer(dst))) return PBSGPU_E_INVALID;
    AuxLease lease(e);
    Slot *s = lease.s;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(nframe, (uint64_t)e->num_cus * 4);
    std::vector<Desc> desc(nframe);
    for (uint32_t i = 0; i < nframe; ++i) desc[i] = Desc{frames[i].offset, frames[i].length, out[i].offset, out[i].length};
    Plan pl{};
    CHK(put_table(s, desc.data(), nframe, &pl.desc));
    pl.res = s->take<uint64_t>(nframe);
    pl.lit = s->bulk((size_t)grid * pbsz::kLitMax);
    CHK(s->taken());
    pl.src = static_cast<const uint8_t *>(src);
    pl.dst = static_cast<uint8_t *>(dst);
    pl.nframe = nframe;
    pl.stride = grid;
    if (flags) {  // checksums verified, whole streams: k_zstd_frames2 (zstd_checksum.hip)
        HIPCHK(pbsk::zstd::launch_frames2(pl, flags, s->stream));
    } else {
        hipLaunchKernelGGL(pbsk::zstd::k_zstd_frames, dim3(grid), dim3(64), 0, s->stream, pl);
        HIPCHK(hipGetLastError());
    }
    std::vector<uint64_t> back(nframe);
    CHK(fetch_result(s, back.data(), pl.res, (size_t)nframe * 8));  // the call's one synchronisation
    for (uint32_t i = 0; i < nframe; ++i) {
        status[i] = (uint8_t)(back[i] >> 32);
        if (decoded) decoded[i] = (uint32_t)back[i];
    }
    return PBSGPU_OK;
}

}  // namespace

extern "C" {

int pbsgpu_zstd_decode_device(pbsgpu_engine *eng, const void *src, uint64_t nbytes, const pbsgpu_segment *frames,
                              uint32_t nframe, const pbsgpu_segment *out, void *dst, uint64_t dst_cap, uint8_t *status,
                              uint64_t *decoded) {
    return zstd_decode(eng, src, nbytes, frames, nframe, out, dst, dst_cap, status, decoded, 0);
}

int pbsgpu_zstd_decode2_device(pbsgpu_engine *eng, const void *src, uint64_t nbytes, const pbsgpu_segment *frames,
                               uint32_t nframe, const pbsgpu_segment *out, void *dst, uint64_t dst_cap, uint8_t *status,
                               uint64_t *decoded, uint32_t flags) {
    return zstd_decode(eng, src, nbytes, frames, nframe, out, dst, dst_cap, status, decoded, flags);
}

}  // extern "C"
