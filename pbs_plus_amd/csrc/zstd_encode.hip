// Zstandard frames written on the device (pbsgpu_zstd_encode_device, the zstd leg of pbsgpu_blob_encode2_device;
// include/pbsgpu.h).
//
// The format lives in zstd_encode.h, once, for these kernels and for the CPU build that runs under sanitizers. This file
// adds the cooperation between lanes and the assembly of the blocks into frames:
//   k_zenc_blocks    one wave (a workgroup of 64) per 128 KiB block; the workgroups take the blocks of all chunks of a round
//                    from a counter, one at a time. Blocks are independent (no match reaches before its block), so any
//                    wave takes any block, and a block of a chunk that is not to be encoded (Job::out == kNoJob: the fused
//                    upload's known records) costs the read of its job. The wave's State — the 16 KiB hash
//                    table, histogram, Huffman code, the three predefined FSE encoding tables, the batch of 64 positions —
//                    is the workgroup's LDS (about 20 KiB: seven workgroups fit a CU's 160 KiB). The block's literals
//                    (128 KiB) and sequences (kSeqCap * 8 = 192 KiB) lie in the workgroup's part of the slot's scratch; its
//                    compressed form goes to the BLOCK's 128 KiB of scratch, because the frame it belongs to is put
//                    together later. Per block: type and size. A chunk may lie in two parts (a ring chunk in two pages):
//                    the one block that holds the seam is put together in the workgroup's scratch first.
//                    With pbsgpu_engine_options::zstd_seq_tables the same loop runs as k_zenc_tblocks, in a translation unit
//                    of its own (zstd_encode_tables.hip), on a State that adds the per-block sequence tables. With
//                    pbsgpu_engine_options::zstd_window_log either runs with the long-range match finder, as
//                    k_zenc_wblocks or k_zenc_wtblocks (zstd_encode_window.hip).
//   k_zenc_assemble  one workgroup of 256 per chunk: a prefix over its blocks' sizes (wave 0), then the frame header, the
//                    block headers and the payloads (content for raw blocks, one byte for RLE, the compressed form) to
//                    their places in the room. It records the frame's length and the status; for the blob call the
//                    verdict instead: a frame that is not strictly shorter than its chunk is not written.
//   sync()           a workgroup barrier with its fences, wherever lanes read what other lanes stored.
// The host plans rounds of whole chunks (zstd_plan.h) so that the per-block scratch stays bounded (kRoundBlocks blocks,
// 256 MiB), and enqueues them back to back on one stream: nothing is read back in between.
// No scratch memory, no spills, no dynamically indexed private arrays (tests/test_zstd_encode_surface.py).
#include <algorithm>
#include <cstring>
#include <vector>

#include "zstd_encode_blocks.h"
#include "zstd_frames.h"

using namespace pbse;
namespace ze = pbsz::enc;

namespace pbsk {
namespace zenc {

__global__ __launch_bounds__(64) void k_zenc_blocks(Plan pl) {
    __shared__ ze::State st;
    encode_blocks(pl, st);
}

__global__ __launch_bounds__(256) void k_zenc_assemble(Plan pl) {
    __shared__ uint64_t s_total;
    const uint32_t t = threadIdx.x;
    for (uint32_t c = pl.c0 + blockIdx.x; c < pl.c1; c += gridDim.x) {
        const Job j = pl.jobs[c];
        if (j.out == kNoJob) continue;
        const uint32_t nb = (uint32_t)(((uint64_t)j.len + pbsz::kBlockMax - 1) / pbsz::kBlockMax);  // 0: the empty frame
        const uint32_t hb = ze::header_bytes(j.len);
        const uint32_t fb = j.first - pl.b0;
        if (t < 64) {  // where each block goes: 3 + payload bytes each, behind the frame header
            uint64_t carry = hb;
            for (uint32_t g = 0; g < nb; g += 64) {
                const uint32_t k = g + t;
                const uint32_t sz = k < nb ? 3u + (pl.bres[fb + k] >> 2) : 0u;
                uint32_t incl = sz;  // (64 blocks: below 2^32)
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const uint32_t u = __shfl_up(incl, d, 64);
                    if ((int)t >= d) incl += u;
                }
                if (k < nb) pl.boff[fb + k] = carry + incl - sz;
                carry += __shfl(incl, 63, 64);
            }
            if (t == 0) s_total = nb ? carry : (uint64_t)hb + 3;
        }
        __syncthreads();
        const uint64_t flen = s_total + (pl.sums ? 4u : 0u);  // with the content checksum behind the last block
        const bool write = pl.blob ? flen < j.len : flen <= j.room;
        const uint32_t status = pl.blob ? (write ? PBSGPU_BLOB_COMPRESSED : PBSGPU_BLOB_UNCOMPRESSED)
                                        : (write ? PBSGPU_ZSTD_OK : PBSGPU_ZSTD_BAD_SIZE);
        if (write) {
            uint8_t *d = pl.dst + j.dst_off;
            if (t == 0) {
                ze::frame_header(j.len, d, pl.sums != nullptr);
                if (nb == 0) ze::block_header(d + hb, 1, ze::B_RAW, 0);
                if (pl.sums) {
                    const uint32_t low = (uint32_t)pl.sums[j.out];
                    for (uint32_t i = 0; i < 4; ++i) d[flen - 4 + i] = (uint8_t)(low >> (8 * i));
                }
            }
            for (uint32_t k = 0; k < nb; ++k) {
                const uint32_t r = pl.bres[fb + k], type = r & 3u, size = r >> 2;
                const uint32_t at = k * pbsz::kBlockMax;
                const uint32_t bn = j.len - at < pbsz::kBlockMax ? j.len - at : pbsz::kBlockMax;
                uint8_t *o = d + pl.boff[fb + k];
                if (t == 0) {
                    ze::block_header(o, k + 1 == nb ? 1u : 0u, type, type == ze::B_COMPRESSED ? size : bn);
                    if (type == ze::B_RLE) o[3] = pl.src[chunk_byte(j, at)];
                }
                if (type == ze::B_RAW) {
#pragma unroll 8
                    for (uint32_t i = t; i < size; i += 256) o[3 + i] = pl.src[chunk_byte(j, at + i)];
                } else if (type == ze::B_COMPRESSED) {
                    const uint8_t *from = pl.blkout + (uint64_t)(fb + k) * pbsz::kBlockMax;
#pragma unroll 8
                    for (uint32_t i = t; i < size; i += 256) o[3 + i] = from[i];
                }
            }
        }
        if (t == 0) pl.res[j.out] = (write || pl.blob ? flen : 0ull) | (uint64_t)status << 56;
        __syncthreads();  // s_total goes to the next chunk
    }
}

constexpr uint32_t kRoundBlocks = 2048;  // 256 MiB of per-block scratch

static size_t pad64(size_t n) { return (n + 63) & ~(size_t)63; }

int prepare(pbsgpu_engine *e, std::vector<Job> &jobs, bool two_parts, Prep &p) {
    const uint32_t n = (uint32_t)jobs.size();
    if (!ze::plan_blocks(n, [&](uint32_t c) { return jobs[c].len; }, pbsz::kBlockMax, kRoundBlocks, p.bp))
        return PBSGPU_E_INVALID;  // 512 TiB in one call
    for (uint32_t c = 0; c < n; ++c) jobs[c].first = p.bp.first[c];
    p.grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(p.bp.most, (uint64_t)e->num_cus * 4));
    p.two_parts = two_parts;
    p.jobs_bytes = pad64((size_t)n * sizeof(Job));
    p.bchunk_bytes = pad64((size_t)p.bp.nblocks * 4);
    p.res_bytes = pad64((size_t)n * 8);
    p.blkout_bytes = pad64((size_t)p.bp.most * pbsz::kBlockMax);
    p.bplace_bytes = pad64((size_t)p.bp.most * 12 + (p.bp.cuts.size() - 1) * 4);
    p.window_log = e->opt.zstd_window_log;  // the engine's: a slot's size is stable
    // the long-range match finder reads both parts in place and stages nothing; its table takes the staged block's place
    p.work_bytes = (size_t)p.grid * (p.window_log ? kWindowWork : (two_parts ? 2 : 1) * (size_t)pbsz::kBlockMax + (size_t)ze::kSeqCap * 8);
    return PBSGPU_OK;
}

int carve(Slot *s, const Prep &p, const std::vector<Job> &jobs, Room &room) {
    room.jobs = reinterpret_cast<Job *>(s->take<uint8_t>(p.jobs_bytes));
    room.bchunk = reinterpret_cast<uint32_t *>(s->take<uint8_t>(p.bchunk_bytes));
    room.res = reinterpret_cast<uint64_t *>(s->take<uint8_t>(p.res_bytes));
    room.bplace = reinterpret_cast<uint64_t *>(s->take<uint8_t>(p.bplace_bytes));
    room.blkout = s->bulk(p.blkout_bytes);
    room.work = s->bulk(p.work_bytes);
    CHK(s->taken());
    CHK(staged_h2d(*s, room.jobs, jobs.data(), jobs.size() * sizeof(Job), s->stream));
    if (p.bp.nblocks) CHK(staged_h2d(*s, room.bchunk, p.bp.bchunk.data(), (size_t)p.bp.nblocks * 4, s->stream));
    return PBSGPU_OK;
}

// the rounds, back to back on st; nothing synchronised
int launch(pbsgpu_engine *e, hipStream_t st, const Prep &p, const Room &room, const uint8_t *src, uint8_t *dst, bool blob,
           const uint64_t *sums) {
    Plan pl{};
    pl.sums = sums;
    pl.src = src;
    pl.jobs = room.jobs;
    pl.bchunk = room.bchunk;
    pl.blkout = room.blkout;
    pl.boff = room.bplace;
    pl.bres = reinterpret_cast<uint32_t *>(room.bplace + p.bp.most);
    pl.lit = room.work;
    pl.seqs = reinterpret_cast<uint64_t *>(room.work + (size_t)p.grid * pbsz::kBlockMax);
    pl.stage = p.two_parts && !p.window_log ? room.work + (size_t)p.grid * (pbsz::kBlockMax + (size_t)ze::kSeqCap * 8) : nullptr;
    pl.window_log = p.window_log;  // (the window kernels: kWindowWork bytes per workgroup from pl.lit on, nothing staged)
    pl.dst = dst;
    pl.res = room.res;
    pl.blob = blob ? 1u : 0u;
    uint32_t *counters = pl.bres + p.bp.most;  // one per round
    HIPCHK(hipMemsetAsync(counters, 0, (p.bp.cuts.size() - 1) * 4, st));
    for (size_t r = 0; r + 1 < p.bp.cuts.size(); ++r) {
        pl.next = counters + r;
        pl.c0 = p.bp.cuts[r];
        pl.c1 = p.bp.cuts[r + 1];
        pl.b0 = p.bp.block_begin(pl.c0);
        pl.b1 = p.bp.block_begin(pl.c1);
        if (pl.c0 == pl.c1) continue;
        if (pl.b1 > pl.b0) {
            const uint32_t grid = std::min<uint32_t>(p.grid, pl.b1 - pl.b0);
            if (p.window_log) {  // the engine's options: the long-range match finder, without or with tables
                HIPCHK(launch_blocks_window(pl, grid, e->opt.zstd_seq_tables != 0, st));
            } else if (e->opt.zstd_seq_tables) {  // per-block tables and repeat codes
                HIPCHK(launch_blocks_tables(pl, grid, st));
            } else {
                hipLaunchKernelGGL(k_zenc_blocks, dim3(grid), dim3(64), 0, st, pl);
                HIPCHK(hipGetLastError());
            }
        }
        hipLaunchKernelGGL(k_zenc_assemble, dim3(std::min<uint32_t>(pl.c1 - pl.c0, (uint32_t)e->num_cus * 8)), dim3(256), 0, st, pl);
        HIPCHK(hipGetLastError());
    }
    return PBSGPU_OK;
}

// The frames of jobs[0, n), every one of them, enqueued on the slot's stream, nothing synchronised.
// *res_dev = per chunk, frame length | status << 56 (blob: the kind, and nothing written unless compressed).
int enqueue(pbsgpu_engine *e, Slot *s, const uint8_t *src, uint8_t *dst, std::vector<Job> &jobs, bool blob, uint64_t **res_dev,
            const uint64_t *sums) {
    for (uint32_t c = 0; c < jobs.size(); ++c) {
        jobs[c].src1_off = 0;
        jobs[c].a = jobs[c].len;
        jobs[c].out = c;
    }
    Prep p;
    CHK(prepare(e, jobs, false, p));
    Room room;
    CHK(carve(s, p, jobs, room));
    CHK(launch(e, s->stream, p, room, src, dst, blob, sums));
    *res_dev = room.res;
    return PBSGPU_OK;
}

}  // namespace zenc
}  // namespace pbsk

namespace {

int zstd_encode(pbsgpu_engine *e, const void *src, uint64_t nbytes, const pbsgpu_segment *chunks, uint32_t n,
                const pbsgpu_segment *out, void *dst, uint64_t dst_cap, uint8_t *status, uint64_t *frame_len, uint32_t flags) {
    if (!e || (flags & ~(uint32_t)PBSGPU_ZSTD_F_CHECKSUM)) return PBSGPU_E_INVALID;
    if (n == 0) return PBSGPU_OK;
    if (!chunks || !out || !status || (!src && nbytes) || (!dst && dst_cap)) return PBSGPU_E_INVALID;
    uint64_t lo = ~0ull, hi = 0;  // the part of dst the call may write
    for (uint32_t i = 0; i < n; ++i) {
        if (chunks[i].length >> 32) return PBSGPU_E_INVALID;  // a chunk is 16 MiB at the most
        if (chunks[i].length > nbytes || chunks[i].offset > nbytes - chunks[i].length) return PBSGPU_E_INVALID;
        if (out[i].length > dst_cap || out[i].offset > dst_cap - out[i].length) return PBSGPU_E_INVALID;
        if (out[i].length) {
            lo = std::min(lo, out[i].offset);
            hi = std::max(hi, out[i].offset + out[i].length);
        }
    }
    std::vector<uint32_t> order;
    for (uint32_t i = 0; i < n; ++i)
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
    std::vector<pbsk::zenc::Job> jobs(n);
    for (uint32_t i = 0; i < n; ++i) jobs[i] = pbsk::zenc::Job{chunks[i].offset, 0, out[i].offset, out[i].length, (uint32_t)chunks[i].length, 0, 0, 0};
    uint64_t *sums = nullptr;
    if (flags & PBSGPU_ZSTD_F_CHECKSUM) {  // XXH64 of every chunk's source bytes, on the same stream, in front of the frames
        const pbsgpu_segment *ranges = nullptr;
        CHK(put_table(s, chunks, n, &ranges));
        sums = s->take<uint64_t>(n);
        CHK(s->taken());
        HIPCHK(pbsk::zstd::launch_xxh64_ranges(static_cast<const uint8_t *>(src), ranges, n, 0, sums, e->num_cus, s->stream));
    }
    uint64_t *res = nullptr;
    CHK(pbsk::zenc::enqueue(e, s, static_cast<const uint8_t *>(src), static_cast<uint8_t *>(dst), jobs, false, &res, sums));
    std::vector<uint64_t> back(n);
    CHK(fetch_result(s, back.data(), res, (size_t)n * 8));  // the call's one synchronisation
    for (uint32_t i = 0; i < n; ++i) {
        status[i] = (uint8_t)(back[i] >> 56);
        if (frame_len) frame_len[i] = back[i] & ((1ull << 56) - 1);
    }
    return PBSGPU_OK;
}

}  // namespace

extern "C" {

int pbsgpu_zstd_encode_device(pbsgpu_engine *eng, const void *src, uint64_t src_bytes, const pbsgpu_segment *chunks, uint32_t n,
                              const pbsgpu_segment *out, void *dst, uint64_t dst_cap, uint8_t *status, uint64_t *frame_len) {
    return zstd_encode(eng, src, src_bytes, chunks, n, out, dst, dst_cap, status, frame_len, 0);
}

int pbsgpu_zstd_encode2_device(pbsgpu_engine *eng, const void *src, uint64_t src_bytes, const pbsgpu_segment *chunks, uint32_t n,
                               const pbsgpu_segment *out, void *dst, uint64_t dst_cap, uint8_t *status, uint64_t *frame_len,
                               uint32_t flags) {
    return zstd_encode(eng, src, src_bytes, chunks, n, out, dst, dst_cap, status, frame_len, flags);
}

}  // extern "C"
